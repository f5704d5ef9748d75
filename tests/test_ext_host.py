"""Host tests (no GPU) of the smooth / antisymmetric / antireflect modes: the torch reference tests/_ext_ref.py against the oracle in
the five modes the oracle has (which pins pads and alignment to the PyWavelets goldens the oracle carries), its extension against
``numpy.pad`` in the three new ones, its adjoint against autograd; the argument errors of the new modes; the launches a level takes
(recorded, not made); the C ABI (header, exported symbols, ``mifwt_ext_supported``).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ptwt_amd
from oracle import fwt_oracle as O
from ptwt_amd import _engine, _ext
from ptwt_amd._wavelets import host_taps
from tests import _ext_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mifwt_ext_supported", "mifwt_ext_kernel_id", "mifwt_ext_fwd", "mifwt_ext_adj", "mifwt_ext_axis_fwd", "mifwt_ext_axis_adj")


# ---- the reference -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.OLD_MODES)
@pytest.mark.parametrize("wavelet", ["haar", "db2", "db4", "bior3.5"])
def test_reference_matches_the_oracle_in_the_old_modes(mode, wavelet):
    bank = host_taps(wavelet)
    g = np.random.default_rng(len(bank[0]))
    for n in (32, 33):  # 1-D, even and odd
        x = g.standard_normal((3, n))
        ca, cd = R.dwt_axis(torch.from_numpy(x), bank[0], bank[1], mode, -1)
        ea, ed = O.dwt_axis(x, bank[0], bank[1], mode, -1)
        assert ca.shape == ea.shape == (3, (n + len(bank[0]) - 1) // 2)
        assert R.relerr(ca, torch.from_numpy(ea)) < 1e-13 and R.relerr(cd, torch.from_numpy(ed)) < 1e-13
        rec = R.idwt_axis(ca, cd, bank[2], bank[3], -1)
        assert R.relerr(rec, torch.from_numpy(O.idwt_axis(ea, ed, bank[2], bank[3], -1))) < 1e-13
    for shape in ((2, 32, 41), (2, 35, 30)):  # 2-D, two levels
        x = g.standard_normal(shape)
        got = R.wavedecn(torch.from_numpy(x), bank, mode, 2, 2)
        want = O.wavedec2(x, wavelet, mode=mode, level=2)
        assert R.relerr(got[0], torch.from_numpy(want[0])) < 1e-13
        for det, (h, v, d) in zip(got[1:], want[1:]):  # bands 1, 2, 3 = 'ad' (V), 'da' (H), 'dd' (D)
            for a, b in zip(det, (v, h, d)):
                assert a.shape == b.shape and R.relerr(a, torch.from_numpy(b)) < 1e-13
        assert R.relerr(R.waverecn(got, bank, 2), torch.from_numpy(O.waverec2(want, wavelet))) < 1e-13


@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_extend_matches_numpy(n):
    g = np.random.default_rng(n)
    x = g.standard_normal((2, n))
    xt = torch.from_numpy(x)
    for pl, pr in ((0, 0), (1, 2), (7, 3), (20, 20)):
        got = R.extend(xt, "antireflect", pl, pr, -1).numpy()
        assert np.abs(got - np.pad(x, ((0, 0), (pl, pr)), mode="reflect", reflect_type="odd")).max() < 1e-13
        got = R.extend(xt, "smooth", pl, pr, -1).numpy()
        for row in range(2):
            ends = (x[row, 0] - pl * (x[row, 1] - x[row, 0]), x[row, -1] + pr * (x[row, -1] - x[row, -2]))
            assert np.abs(got[row] - np.pad(x[row], (pl, pr), mode="linear_ramp", end_values=ends)).max() < 1e-13
        got = R.extend(xt, "antisymmetric", pl, pr, -1).numpy()
        reps = 2 * (max(pl, pr) // (2 * n) + 2)
        tiled = np.tile(np.concatenate([x, -x[:, ::-1]], -1), (1, reps))
        start = (reps // 2) * 2 * n - pl
        assert np.abs(got - tiled[:, start:start + n + pl + pr]).max() == 0.0
        # and the two old mirrors against numpy as well
        assert np.abs(R.extend(xt, "symmetric", pl, pr, -1).numpy() - np.pad(x, ((0, 0), (pl, pr)), mode="symmetric")).max() == 0.0
        assert np.abs(R.extend(xt, "reflect", pl, pr, -1).numpy() - np.pad(x, ((0, 0), (pl, pr)), mode="reflect")).max() == 0.0


def test_extension_of_one_sample():
    """The project's convention for N = 1: smooth and antireflect repeat the sample, antisymmetric alternates its sign."""
    x = torch.tensor([[1.5]], dtype=torch.float64)
    assert R.extend(x, "smooth", 3, 4, -1).tolist() == [[1.5] * 8]
    assert R.extend(x, "antireflect", 3, 4, -1).tolist() == [[1.5] * 8]
    assert R.extend(x, "antisymmetric", 3, 4, -1).tolist() == [[-1.5, 1.5, -1.5, 1.5, -1.5, 1.5, -1.5, 1.5]]


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 13])
def test_fold_is_the_transpose(mode, n):
    """The E^T fold of the adjoint reference equals autograd through ``extend``; ``adj_axis`` equals autograd through ``dwt_axis``."""
    g = torch.Generator().manual_seed(n)
    pl, pr = 9, 12
    x = torch.randn(2, n, generator=g, dtype=torch.float64, requires_grad=True)
    t = torch.randn(2, n + pl + pr, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad((R.extend(x, mode, pl, pr, -1) * t).sum(), x)
    assert R.relerr(t @ R.ext_matrix(n, mode, pl, pr), want) < 1e-13
    for wavelet in ("db2", "db10"):
        lo, hi = host_taps(wavelet)[:2]
        m = (n + len(lo) - 1) // 2
        ga, gd = torch.randn(2, m, generator=g, dtype=torch.float64), torch.randn(2, m, generator=g, dtype=torch.float64)
        ca, cd = R.dwt_axis(x, lo, hi, mode, -1)
        (want,) = torch.autograd.grad((ca * ga).sum() + (cd * gd).sum(), x)
        assert R.relerr(R.adj_axis(ga, gd, lo, hi, mode, n, -1), want) < 1e-12


def test_linear_ramp_has_no_details_in_the_reference():
    x = torch.arange(37, dtype=torch.float64)[None] * 0.25 - 3.0
    for wavelet in ("db2", "db4"):
        lo, hi = host_taps(wavelet)[:2]
        for mode in ("smooth", "antireflect"):
            assert float(R.dwt_axis(x, lo, hi, mode, -1)[1].norm()) < 1e-12 * float(x.norm())
        assert float(R.dwt_axis(x, lo, hi, "symmetric", -1)[1].norm()) > 1e-3 * float(x.norm())


@pytest.mark.parametrize("mode", R.NEW_MODES)
def test_reference_round_trip_is_the_input(mode):
    """The padded synthesis inverts a level of any extension: the reference's round trip gives the input back (one sample more on an
    odd axis), which is what the GPU round trips are compared with."""
    for shape, ndim, wavelet in (((3, 131), 1, "db4"), ((2, 13, 10), 2, "bior3.5"), ((1, 9, 8, 12), 3, "db2")):
        bank = host_taps(wavelet)
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
        rec = R.waverecn(R.wavedecn(x, bank, mode, ndim, 3), bank, ndim)
        assert R.relerr(rec[(slice(None),) + tuple(slice(0, n) for n in shape[1:])], x) < 1e-10


# ---- argument errors --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.NEW_MODES)
def test_cpu_tensor_is_refused(mode):
    x = torch.randn(2, 13, 10)
    for call in (lambda: ptwt_amd.wavedec(x, "db2", mode=mode), lambda: ptwt_amd.wavedec2(x, "db2", mode=mode),
                 lambda: ptwt_amd.wavedec3(x, "db2", mode=mode), lambda: ptwt_amd.fswavedec2(x, "db2", mode=mode)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            call()


@pytest.mark.parametrize("mode", R.NEW_MODES)
def test_float16_is_refused(mode):
    x = torch.randn(2, 16, 16).half()
    with pytest.raises(ValueError, match="not supported"):
        ptwt_amd.wavedec2(x, "db2", mode=mode)
    with ptwt_amd.half_storage():
        with pytest.raises(ValueError, match="Input dtype .* not supported"):
            ptwt_amd.wavedec2(x, "db2", mode=mode)
        with pytest.raises(ValueError, match="Input dtype .* not supported"):
            ptwt_amd.WaveletPacket2D(x, "db2", mode=mode, maxlevel=1)


@pytest.mark.parametrize("mode", R.NEW_MODES)
def test_learnable_and_device_taps_are_refused(mode):
    x = torch.randn(2, 16, 16)
    bank = tuple(torch.tensor(t, dtype=torch.float32) for t in host_taps("db2"))
    learnable = tuple(t.clone().requires_grad_(True) for t in bank)
    with pytest.raises(NotImplementedError, match="learnable"):
        ptwt_amd.wavedec2(x, learnable, mode=mode)
    with pytest.raises(NotImplementedError, match="learnable"):
        ptwt_amd.wavedec(x, learnable, mode=mode)
    ptwt_amd.set_device_taps("always")
    try:
        with pytest.raises(NotImplementedError, match="device-resident"):
            ptwt_amd.wavedec2(x, bank, mode=mode)
    finally:
        ptwt_amd.set_device_taps("auto")
    with pytest.raises(RuntimeError, match="ROCm device"):  # (tensor taps that need no gradient are read on the host: accepted)
        ptwt_amd.wavedec2(x, bank, mode=mode)


def test_unknown_modes_keep_their_errors():
    x = torch.randn(2, 16, 16)
    with pytest.raises(ValueError, match="Padding mode not supported: bogus"):
        ptwt_amd.wavedec2(x, "db2", mode="bogus")
    with pytest.raises(ValueError, match="Padding mode not supported: bogus"):
        ptwt_amd.waverec2((x, (x, x, x)), "db2", mode="bogus")
    with pytest.raises(ValueError):
        ptwt_amd.MatrixWavedec("db2", level=1, odd_coeff_padding_mode="smooth")(torch.randn(2, 15))
    assert _engine.MODE_IDS == {"zero": 0, "constant": 1, "reflect": 2, "periodic": 3, "symmetric": 4}


def test_negative_level_is_refused():
    with pytest.raises(ValueError, match="Level value"):
        ptwt_amd.wavedec2(torch.randn(2, 16, 16), "db2", mode="smooth", level=-1)


# ---- launches, recorded ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def recorded(monkeypatch):
    seen = []
    monkeypatch.setattr(_engine, "_require_gpu", lambda t: None)
    monkeypatch.setattr(_engine, "_run", lambda tag, kid, extent, anchor, entry, args, **kw: seen.append((kid, args)) or 0)
    _ext._plans.clear()
    yield seen
    _ext._plans.clear()


@pytest.mark.parametrize("mode", R.NEW_MODES)
def test_short_extents_raise_nothing_and_levels_take_one_launch(mode, recorded):
    """Unlike "reflect", the new modes have no pad check: an axis of 2 samples under db10 is a level.  One fused launch per 1-D or 2-D
    level; a 3-D level is the fused launch plus one axis launch."""
    kids = lambda: [k for k, _ in recorded]  # noqa: E731
    out = ptwt_amd.wavedec(torch.zeros(3, 2), "db10", mode=mode, level=2)
    assert [tuple(t.shape) for t in out] == [(3, 14), (3, 14), (3, 10)] and kids() == [42, 42]
    with pytest.raises(RuntimeError):
        ptwt_amd.wavedec(torch.zeros(3, 2), "db10", mode="reflect", level=1)
    del recorded[:]
    out = ptwt_amd.wavedec2(torch.zeros(3, 13, 10), "db4", mode=mode, level=3)
    assert tuple(out[0].shape) == (3, 7, 7) and kids() == [42, 42, 42]
    del recorded[:]
    out = ptwt_amd.wavedec3(torch.zeros(2, 9, 8, 12), "db2", mode=mode, level=2)
    assert tuple(out[0].shape) == (2, 4, 4, 5) and kids() == [42, 44, 42, 44]
    del recorded[:]
    ptwt_amd.fswavedec3(torch.zeros(2, 9, 8, 12), "db2", mode=mode, level=1)
    ptwt_amd.fswavedec2(torch.zeros(2, 9, 8, 12), "db2", mode=mode, level=1)
    assert kids() == [42, 44, 42]
    # the mode reaches the launch as the C ABI's ext_mode
    assert all(args[1] == _ext.MODES[mode] for k, args in recorded if k == 42)
    assert all(args[0] == _ext.MODES[mode] for k, args in recorded if k == 44)


def test_axis_route_for_long_filters_and_permuted_axes(recorded):
    kids = lambda: [k for k, _ in recorded]  # noqa: E731
    g = np.random.default_rng(24)
    bank = tuple(tuple(g.standard_normal(24)) for _ in range(4))
    ptwt_amd.wavedec(torch.zeros(3, 40), bank, mode="smooth", level=1)
    assert kids() == [44]
    del recorded[:]
    ptwt_amd.wavedec2(torch.zeros(3, 40, 30), bank, mode="antireflect", level=1)
    assert kids() == [44, 44, 44]
    del recorded[:]
    ptwt_amd.wavedec2(torch.zeros(13, 10, 3), "db2", mode="antisymmetric", level=1, axes=(0, 1))  # samples not contiguous
    assert kids() == [44, 44, 44]
    del recorded[:]
    ptwt_amd.wavedec3(torch.zeros(2, 9, 8, 12), bank, mode="smooth", level=1)
    assert kids() == [44] * 7
    del recorded[:]
    # the adjoint mirrors it
    lo, hi = bank[:2]
    _ext.level_adj(torch.zeros(3, 4, 31, 26), lo, hi, "smooth", (40, 30))
    _ext.level_adj(torch.zeros(3, 4, 8, 6), *host_taps("db2")[:2], "smooth", (13, 10))
    _ext.level_adj(torch.zeros(2, 8, 6, 5, 7), *host_taps("db2")[:2], "smooth", (9, 8, 12))
    _ext.level_adj(torch.zeros(3, 2, 8), *host_taps("db2")[:2], "smooth", (13,))
    assert kids() == [45, 45, 45, 43, 45, 43, 43]
    del recorded[:]
    _ext.FORCE_AXIS = True
    try:
        _ext.level_fwd(torch.zeros(3, 13, 10), *host_taps("db2")[:2], "smooth")
        _ext.level_adj(torch.zeros(3, 4, 8, 6), *host_taps("db2")[:2], "smooth", (13, 10))
    finally:
        _ext.FORCE_AXIS = False
    assert kids() == [44, 44, 44, 45, 45, 45]
    assert _ext.AXIS_PASS_CELLS == set()


@pytest.mark.parametrize("order", ["3d-first", "2d-first"])
def test_level_plans_are_keyed_by_every_stride_set(order, recorded):
    """The fused launch inside a 3-D level (planes of its own temporary) and a 2-D level on a tensor of the folded shape have the same
    signal geometry and different band strides: each must get the descriptor of ITS buffers, whichever runs first — and so must a
    level on a row-pitched slice."""
    lo, hi = host_taps("db2")[:2]
    wide = torch.zeros(18, 8, 15)
    calls = {"3d": lambda: _ext.level_fwd(torch.zeros(2, 9, 8, 12), lo, hi, "smooth"),
             "2d": lambda: _ext.level_fwd(torch.zeros(18, 8, 12), lo, hi, "smooth"),
             "slice": lambda: _ext.level_fwd(wide[..., :12], lo, hi, "smooth")}
    want = {"3d": (35, 7, 1), "2d": (140, 7, 1), "slice": (140, 7, 1)}  # band strides: planes [4, 18, 5, 7] against a buffer [18, 4, 5, 7]
    sig = {"3d": (96, 12, 1), "2d": (96, 12, 1), "slice": (120, 15, 1)}
    for which in (("3d", "2d", "slice") if order == "3d-first" else ("slice", "2d", "3d")):
        del recorded[:]
        calls[which]()
        fused = [args for kid, args in recorded if kid == _ext.KID_FWD]
        assert len(fused) == 1
        d = fused[0][0]._obj
        assert (tuple(d.approx_stride[:3]), tuple(d.detail_stride[:3])) == (want[which], want[which]), (order, which)
        assert tuple(d.sig_stride[:3]) == sig[which]
        assert (d.batch, tuple(d.sig_extent[:2]), tuple(d.coef_extent[:2])) == (18, (8, 12), (5, 7))
    assert _ext._plans in _engine._routing_caches


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_header_and_library_export_the_symbols():
    with open(os.path.join(ROOT, "include", "mifwt.h")) as f:
        header = f.read()
    lib = _engine.load_library()
    for sym in SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert getattr(lib, sym) is not None
        assert sym not in _engine._ENTRIES and sym in _engine.EXT_ENTRIES
    for name, kid in (("MIFWT_KID_EXT_FWD", 42), ("MIFWT_KID_EXT_ADJ", 43), ("MIFWT_KID_EXT_AXIS_FWD", 44), ("MIFWT_KID_EXT_AXIS_ADJ", 45)):
        assert re.search(r"#define %s %d\b" % (name, kid), header)
    for name, value in (("MIFWT_EXT_SMOOTH", 0), ("MIFWT_EXT_ANTISYMMETRIC", 1), ("MIFWT_EXT_ANTIREFLECT", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), header)
    assert lib.mifwt_abi_version() == 3
    assert "#define MIFWT_ABI_VERSION 3" in header


def _desc(dtype, flen, sig, coef=None, last=1):
    nd = len(sig)
    coef = [(n + flen - 1) // 2 for n in sig] if coef is None else coef
    ss, cs = [last], [last]
    for n, m in zip(reversed(sig), reversed(coef)):
        ss.insert(0, ss[0] * n)
        cs.insert(0, cs[0] * m)
    d = _engine.LevelDesc()
    d.ndim, d.dtype, d.mode, d.filt_len, d.batch = nd, _engine._DTYPE_IDS[dtype], 0, flen, 1
    for a in range(nd):
        d.sig_extent[a], d.coef_extent[a] = sig[a], coef[a]
    for a in range(nd + 1):
        d.sig_stride[a], d.approx_stride[a], d.detail_stride[a] = ss[a], cs[a], cs[a]
    return d


def test_ext_supported_answers_on_the_host():
    lib = _ext._lib()  # (the entries with their argument types, _engine.EXT_ENTRIES)

    def ask(d, direction, mode=0):
        return lib.mifwt_ext_supported(ctypes.byref(d), mode, direction), lib.mifwt_ext_kernel_id(ctypes.byref(d), mode, direction)

    for direction, kid in ((0, 42), (1, 43)):
        for mode in (0, 1, 2):
            assert ask(_desc(torch.float32, 20, [1, 1]), direction, mode) == (1, kid)
        assert ask(_desc(torch.float64, 2, [7]), direction) == (1, kid)
        assert ask(_desc(torch.float32, 22, [1, 1]), direction) == (0, -2)
        assert ask(_desc(torch.float16, 8, [16, 16]), direction) == (0, -2)
        assert ask(_desc(torch.float32, 8, [16, 16], last=2), direction) == (0, -2)
        assert ask(_desc(torch.float32, 8, [4, 5, 6]), direction) == (0, -2)
        assert ask(_desc(torch.float32, 8, [13, 10], coef=[7, 5]), direction) == (-1, -1)  # (the periodized extents)
        assert ask(_desc(torch.float32, 7, [13, 10]), direction) == (-1, -1)
        assert ask(_desc(torch.float32, 8, [13, 10]), direction, 3) == (-1, -1)
    assert lib.mifwt_ext_supported(ctypes.byref(_desc(torch.float32, 8, [16, 16])), 0, 2) == -1
    # outside the envelope the fused entries launch nothing (null pointers never reach a kernel: the refusal comes first for valid ones)
    d = _desc(torch.float32, 22, [4, 4])
    buf = (ctypes.c_float * 1024)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    det = (ctypes.c_void_p * 3)(p, p, p)
    taps = (ctypes.c_double * 22)()
    before = [_engine.launch_count(k) for k in (42, 43)]
    assert lib.mifwt_ext_fwd(ctypes.byref(d), 0, p, p, det, taps, taps, None) == -2
    assert lib.mifwt_ext_adj(ctypes.byref(d), 0, p, det, p, taps, taps, None) == -2
    assert [_engine.launch_count(k) for k in (42, 43)] == before
    # a null descriptor, then a null data or tap pointer on a served descriptor: each is refused before any launch
    assert (lib.mifwt_ext_supported(None, 0, 0), lib.mifwt_ext_kernel_id(None, 0, 1)) == (-1, -1)
    assert lib.mifwt_ext_fwd(None, 0, p, p, det, taps, taps, None) == -1
    assert lib.mifwt_ext_adj(None, 0, p, det, p, taps, taps, None) == -1
    ok = _desc(torch.float32, 8, [4, 4])
    null_det = (ctypes.c_void_p * 3)(p, None, p)
    for args in ((None, p, det, taps, taps), (p, None, det, taps, taps), (p, p, None, taps, taps), (p, p, null_det, taps, taps),
                 (p, p, det, None, taps), (p, p, det, taps, None)):
        assert lib.mifwt_ext_fwd(ctypes.byref(ok), 0, *args, None) == -1, args
    for args in ((None, det, p, taps, taps), (p, None, p, taps, taps), (p, null_det, p, taps, taps), (p, det, None, taps, taps),
                 (p, det, p, None, taps), (p, det, p, taps, None)):
        assert lib.mifwt_ext_adj(ctypes.byref(ok), 0, *args, None) == -1, args
    assert [_engine.launch_count(k) for k in (42, 43)] == before
    # the axis entries: a null data, stride or tap pointer (-1); float16 with valid pointers is outside their envelope (-2, nothing launched)
    st = (ctypes.c_int64 * 3)(8, 1, 1)
    before = [_engine.launch_count(k) for k in (44, 45)]
    for entry in (lib.mifwt_ext_axis_fwd, lib.mifwt_ext_axis_adj):
        good = [p, st, p, st, p, st, taps, taps]
        for hole in range(len(good)):
            assert entry(0, 0, 8, 1, 8, 1, *[None if i == hole else v for i, v in enumerate(good)], None) == -1, hole
        assert entry(0, 2, 8, 1, 8, 1, *good, None) == -2
        assert entry(3, 0, 8, 1, 8, 1, *good, None) == -1
    assert [_engine.launch_count(k) for k in (44, 45)] == before
