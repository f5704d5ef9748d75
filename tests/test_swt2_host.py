"""Host tests of the 2-D stationary transform: the float64 reference of tests/_swt2_ref.py (the checker of tests/test_gpu_swt2.py) and
the host logic of ``ptwt_amd.swt2`` / ``iswt2`` that needs no device — argument errors, exports, the C ABI's new symbols."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ptwt_amd
from oracle import fwt_oracle as O
from ptwt_amd import _engine
from ptwt_amd._wavelets import host_taps
from tests import _golden as G
from tests import _swt2_ref as R2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bank(name):
    return [np.asarray(t, dtype=np.float64) for t in host_taps(name)]


@pytest.mark.parametrize("name", ["haar", "db4", "sym8"])
def test_reference_round_trip(name):
    dec_lo, dec_hi, rec_lo, rec_hi = _bank(name)
    x = np.random.default_rng(11).standard_normal((16, 32))
    coeffs = R2.swt2(x, dec_lo, dec_hi, level=3)
    assert len(coeffs) == 4 and all(t.shape == x.shape for c in coeffs[1:] for t in c) and coeffs[0].shape == x.shape
    # norm-wise, as every 1e-12 bound of the suite (tests._golden.relerr)
    assert G.relerr(R2.iswt2(coeffs, rec_lo, rec_hi), x) < 1e-12


def test_reference_round_trip_odd_extents():
    """The identity is the 1-D identity along each axis: it holds for any extents and any level."""
    dec_lo, dec_hi, rec_lo, rec_hi = _bank("db2")
    x = np.random.default_rng(12).standard_normal((5, 7))
    assert G.relerr(R2.iswt2(R2.swt2(x, dec_lo, dec_hi, level=2), rec_lo, rec_hi), x) < 1e-12
    assert len(R2.swt2(x, dec_lo, dec_hi)) == 1  # level=None on odd extents: no level


def test_haar_level_closed_form():
    dec_lo, dec_hi, _, _ = _bank("haar")
    x = np.array([[1.0, 2.0, 4.0, 7.0], [0.0, -3.0, 5.0, 2.0], [6.0, 1.0, -2.0, 3.0], [8.0, -1.0, 0.0, 4.0]])
    ca, (ch, cv, cd) = R2.swt2(x, dec_lo, dec_hi, level=1)
    right, down = np.roll(x, -1, 1), np.roll(x, -1, 0)
    diag = np.roll(down, -1, 1)
    # haar: lo[n] = (x[n] + x[n + 1]) / sqrt 2, hi[n] = (x[n] - x[n + 1]) / sqrt 2, periodic
    assert np.abs(ca - (x + right + down + diag) / 2).max() < 1e-14
    assert np.abs(ch - ((x + right) - (down + diag)) / 2).max() < 1e-14  # high-pass down the rows (axis -2)
    assert np.abs(cv - ((x - right) + (down - diag)) / 2).max() < 1e-14  # high-pass along the row (axis -1)
    assert np.abs(cd - ((x - right) - (down - diag)) / 2).max() < 1e-14
    assert abs(ca[0, 0] - (1.0 + 2.0 + 0.0 - 3.0) / 2) < 1e-14 and abs(ch[3, 3] - ((4.0 + 8.0) - (7.0 + 1.0)) / 2) < 1e-14


@pytest.mark.parametrize("dilation", [1, 2, 3])
def test_levels_are_transposes_with_reversed_taps(dilation):
    g = np.random.default_rng(13)
    taps = [g.standard_normal(4) for _ in range(4)]
    rev = [t[::-1] for t in taps]
    h, w, scale = 8, 6, 0.37
    a = R2.level_matrix(h, w, taps, dilation, scale, inverse=False)
    s = R2.level_matrix(h, w, rev, dilation, scale, inverse=True)
    assert a.shape == (4 * h * w, h * w) and s.shape == (h * w, 4 * h * w)
    assert np.abs(a.T - s).max() < 1e-14
    # and the other way round: the synthesis level's transpose is the analysis level with reversed taps
    assert np.abs(R2.level_matrix(h, w, taps, dilation, scale, inverse=True).T - R2.level_matrix(h, w, rev, dilation, scale, inverse=False)).max() < 1e-14


def test_torch_reference_equals_numpy_reference():
    dec_lo, dec_hi, rec_lo, rec_hi = _bank("db3")
    x = np.random.default_rng(14).standard_normal((2, 12, 20))
    want = R2.swt2(x, dec_lo, dec_hi, level=2)
    got = R2.t_swt2(torch.from_numpy(x), dec_lo, dec_hi, level=2)
    assert np.abs(got[0].numpy() - want[0]).max() < 1e-13
    for gd, wd in zip(got[1:], want[1:]):
        for gt, wt in zip(gd, wd):
            assert np.abs(gt.numpy() - wt).max() < 1e-13
    coeffs = [torch.from_numpy(np.random.default_rng(15).standard_normal((12, 20)))] + \
        [tuple(torch.from_numpy(np.random.default_rng(16 + 3 * i + k).standard_normal((12, 20))) for k in range(3)) for i in range(2)]
    want_y = R2.iswt2([coeffs[0].numpy()] + [tuple(t.numpy() for t in c) for c in coeffs[1:]], rec_lo, rec_hi)
    assert np.abs(R2.t_iswt2(coeffs, rec_lo, rec_hi).numpy() - want_y).max() < 1e-13
    # axes: the transform over (1, 3) of a 4-D array is the transform over the last two axes of the moved array
    x4 = np.random.default_rng(17).standard_normal((2, 8, 3, 12))
    a = R2.swt2(x4, dec_lo, dec_hi, level=1, axes=(1, 3))
    b = R2.swt2(np.moveaxis(x4, (1, 3), (-2, -1)), dec_lo, dec_hi, level=1)
    assert np.abs(np.moveaxis(a[1][0], (1, 3), (-2, -1)) - b[1][0]).max() < 1e-14
    t = R2.t_swt2(torch.from_numpy(x4), dec_lo, dec_hi, level=1, axes=(1, 3))
    assert np.abs(t[1][0].numpy() - a[1][0]).max() < 1e-13 and np.abs(t[1][1].numpy() - a[1][1]).max() < 1e-13


def test_band_names_match_wavedec2():
    """cH / cV / cD as ``wavedec2`` names them: on separable inputs that excite one band only, the band that carries the energy is the
    same in the decimated oracle and in the stationary reference."""
    dec_lo, dec_hi, _, _ = _bank("haar")
    const, alt = np.ones(8), np.array([1.0, -1.0] * 4)
    for u, v in ((alt, const), (const, alt), (alt, alt)):
        x = np.outer(u, v)
        dec = O.wavedec2(x, "haar", mode="periodic", level=1)[1]
        sta = R2.swt2(x, dec_lo, dec_hi, level=1)[1]
        e_dec = [float(np.sum(np.asarray(t) ** 2)) for t in dec]
        e_sta = [float(np.sum(t ** 2)) for t in sta]
        assert int(np.argmax(e_dec)) == int(np.argmax(e_sta))
        assert sorted(e_dec)[1] < 1e-20 and sorted(e_sta)[1] < 1e-20  # one band only
    # u varies down the rows (axes[0]): horizontal band, index 0
    assert int(np.argmax([np.sum(t ** 2) for t in R2.swt2(np.outer(alt, const), dec_lo, dec_hi, level=1)[1]])) == 0


def test_exports():
    assert "swt2" in ptwt_amd.__all__ and "iswt2" in ptwt_amd.__all__
    assert callable(ptwt_amd.swt2) and callable(ptwt_amd.iswt2)


def test_header_and_library_have_the_symbols():
    with open(os.path.join(ROOT, "include", "mifwt.h")) as f:
        text = f.read()
    _engine.load_library()
    lib = ctypes.CDLL(_engine.LIB_PATH)  # a handle of its own: binding argument types here leaves the package's handle as it is
    lib.mifwt_swt2_supported.restype = ctypes.c_int
    lib.mifwt_swt2_supported.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_int64] * 4
    lib.mifwt_abi_version.restype = ctypes.c_int
    for sym in ("mifwt_swt2_supported", "mifwt_swt2_fwd", "mifwt_swt2_inv"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, text), sym
        assert hasattr(lib, sym), sym
    assert lib.mifwt_abi_version() == 3
    # the support query is host code: unrolled even lengths up to 20, float32 / float64
    assert [lib.mifwt_swt2_supported(0, flen, 3, 5, 7, 4) for flen in (2, 8, 20, 22, 34, 7)] == [1, 1, 1, 0, 0, 0]
    assert lib.mifwt_swt2_supported(1, 8, 1, 1, 1, 64) == 1 and lib.mifwt_swt2_supported(2, 8, 3, 5, 7, 4) == 0


def test_argument_errors_come_before_device_work():
    """Every argument error is raised on CPU tensors: the device check comes last."""
    x = torch.zeros(2, 8, 8)
    with pytest.raises(ValueError, match="not supported"):
        ptwt_amd.swt2(x.half(), "haar", level=1)
    with ptwt_amd.half_storage():
        with pytest.raises(ValueError, match="Input dtype torch.float16 not supported"):
            ptwt_amd.swt2(x.half(), "haar", level=1)
        with pytest.raises(ValueError, match="Input dtype torch.float16 not supported"):
            ptwt_amd.iswt2([x.half(), (x.half(), x.half(), x.half())], "haar")
    with pytest.raises(ValueError):
        ptwt_amd.swt2(x, "haar", level=1, axes=(-1, -1))
    with pytest.raises(ValueError):
        ptwt_amd.swt2(x, "haar", level=1, axes=(-1,))
    with pytest.raises(ValueError, match="First element"):
        ptwt_amd.iswt2([(x, x, x)], "haar")
    with pytest.raises(ValueError, match="First element"):
        ptwt_amd.iswt2([], "haar")
    with pytest.raises(ValueError, match="3-tuple of tensors"):
        ptwt_amd.iswt2([x, (x, x)], "haar")
    with pytest.raises(ValueError, match="3-tuple of tensors"):
        ptwt_amd.iswt2([x, x], "haar")
    with pytest.raises(ValueError, match="Unexpected input type"):
        ptwt_amd.iswt2([x, (x, None, x)], "haar")
    with pytest.raises(ValueError, match="same dtype"):
        ptwt_amd.iswt2([x, (x, x.double(), x)], "haar")
    with pytest.raises(ValueError, match=r"\(2, 8, 6\).*\(2, 8, 8\)"):
        ptwt_amd.iswt2([x, (x, x[..., :6], x)], "haar")
    # valid arguments on the CPU: the engine's device error, and only then
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.swt2(x, "haar", level=1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.iswt2([x, (x, x, x)], "haar")
    # no level: nothing to run, the input comes back
    out = ptwt_amd.swt2(torch.zeros(3, 5), "haar")
    assert len(out) == 1 and out[0].shape == (3, 5)
    assert len(ptwt_amd.swt2(x, "haar", level=0)) == 1
