"""mra / imra without a GPU: the reference of tests/_mra_ref.py pinned to the reference library's stationary goldens and to the oracle,
perfect reconstruction of the components, the cascade of one-input stages against the definition and three wrong engines that the
bounds of tests/test_gpu_mra.py reject, the envelope of the launch, the errors of ``mra``, ``imra`` on CPU tensors, the composed route
on the oracle level engine, and the C ABI surface."""
import importlib
import os
import re

import pytest
import torch

import ptwt_amd
from oracle import fwt_oracle as O
from ptwt_amd import _engine
from tests import _golden as G
from tests import _mra_ref as R
from tests._oracle_engine import OracleLevelEngine

M = importlib.import_module("ptwt_amd.mra")  # (the package attribute of that name is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANKS = ("haar", "db4", "bior2.2", "db10")
F64_TOL = 1e-12  # the float64 bound of tests/test_gpu_mra.py


@pytest.fixture()
def oracle_engine(monkeypatch):
    from ptwt_amd import stationary_transform as st
    from tests import _oracle_engine as oe

    monkeypatch.setattr(_engine, "ENGINE", OracleLevelEngine())
    monkeypatch.setattr(st, "_level_fwd", oe.swt_level_fwd)
    monkeypatch.setattr(st, "_level_inv", oe.swt_level_inv)


def _x(n, rows=3, seed=0):
    return torch.randn(rows, n, dtype=torch.float64, generator=torch.Generator().manual_seed(seed + n))


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def test_reference_stationary_levels_match_the_goldens():
    """analysis / synthesis of the reference on every last-axis case of ptwt_ref_swt.npz (24 wraps, 2 - 102 taps)."""
    z, idx = G.load("ptwt_ref_swt.npz")
    seen = 0
    for case in idx:
        if case["kw"]:
            continue
        bank = R.bank_of(case["wavelet"])
        k = case["key"]
        x = torch.from_numpy(z[k + "_x"])
        level = case["ncoef"] - 1
        coeffs = R.analysis(x, bank, level, "swt")
        for i, t in enumerate(coeffs):
            assert G.relerr(t.numpy(), z["%s_c%d" % (k, i)]) < 1e-12, (case, i)
        rec = R.synthesis([torch.from_numpy(z["%s_c%d" % (k, i)]) for i in range(level + 1)], bank, "swt")
        assert G.relerr(rec.numpy(), z[k + "_rec"]) < 1e-12, case
        seen += 1
    assert seen == 27


@pytest.mark.parametrize("mode", ["reflect", "zero", "symmetric"])
def test_reference_padded_levels_match_the_oracle(mode):
    for wavelet in BANKS:
        for n in (37, 64):
            x = _x(n)
            want = O.wavedec(x.numpy(), wavelet, mode=mode, level=2)
            bank = R.bank_of(wavelet)
            got = R.analysis(x, bank, 2, "dwt", mode)
            for a, b in zip(got, want):
                assert a.shape == b.shape and G.relerr(a.numpy(), b) < 1e-13
            assert G.relerr(R.synthesis(got, bank, "dwt", mode).numpy(), O.waverec(want, wavelet)) < 1e-13


def test_reference_smooth_extension_is_the_line_through_the_end_samples():
    x = torch.tensor([[1.0, 3.0, 4.0, 9.0]], dtype=torch.float64)
    assert R.extend(x, "smooth", 3, 2).tolist() == [[-5.0, -3.0, -1.0, 1.0, 3.0, 4.0, 9.0, 14.0, 19.0]]
    line = torch.arange(10, dtype=torch.float64)[None] * 0.5 + 2.0
    _, det = R.dwt_pad(line, *R.bank_of("db4")[:2], "smooth")
    assert float(det.abs().max()) < 1e-12  # (two vanishing moments and more: a line has no detail anywhere, borders included)


# ---- the components add up -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", BANKS)
def test_stationary_components_sum_to_the_signal(wavelet):
    for n in (5, 6, 37, 64, 1000):
        for level in (3, 4):
            x = _x(n)
            parts = R.mra(x, wavelet, level, "swt")
            assert len(parts) == level + 1 and all(p.shape == x.shape for p in parts)
            assert float((sum(parts) - x).norm()) <= 1e-12 * float(x.norm()), (n, level)


@pytest.mark.parametrize("mode", ["reflect", "zero", "periodization", "smooth"])
@pytest.mark.parametrize("wavelet", BANKS)
def test_decimated_components_sum_to_the_signal(wavelet, mode):
    for n in (37, 64, 1001):
        x = _x(n)
        parts = R.mra(x, wavelet, 3, "dwt", mode)
        assert len(parts) == 4 and all(p.shape == x.shape for p in parts)
        assert float((sum(parts) - x).norm()) <= 1e-12 * float(x.norm()), n


def test_reference_level_zero_and_axis():
    x = _x(16).reshape(3, 4, 4)
    assert R.mra(x, "haar", 0)[0] is x
    a = R.mra(x, "db4", 2, "swt", axis=1)
    b = R.mra(x.transpose(1, 2), "db4", 2, "swt")
    assert all(torch.equal(p, q.transpose(1, 2)) for p, q in zip(a, b))


# ---- the cascade, and engines the comparison must reject ---------------------------------------------------------------------------------
def _worst(got, want, scale):
    return max(R.relerr(g, w, scale) for g, w in zip(got, want))


@pytest.mark.parametrize("wavelet", BANKS)
def test_cascade_of_one_input_stages_is_the_definition(wavelet):
    bank = R.bank_of(wavelet)
    for n, level in ((37, 3), (64, 4), (5, 3)):
        x = _x(n)
        coeffs = R.analysis(x, bank, level, "swt")
        assert _worst(R.swt_cascade(coeffs, bank), R.components(coeffs, bank, n, "swt"), float(x.norm())) < F64_TOL


@pytest.mark.parametrize("wrong", R.WRONG)
@pytest.mark.parametrize("wavelet", BANKS)
def test_wrong_engines_are_rejected(wavelet, wrong):
    """rec_hi on every stage / the 0.5 dropped / the dilations in the wrong order: each is off by far more than the float32 bound."""
    bank = R.bank_of(wavelet)
    x = _x(64)
    coeffs = R.analysis(x, bank, 3, "swt")
    want = R.components(coeffs, bank, 64, "swt")
    got = R.swt_cascade(coeffs, bank, wrong)
    assert _worst(got, want, 0.0) > 1e-2, (wavelet, wrong)


# ---- the envelope ----------------------------------------------------------------------------------------------------------------------
def test_envelope_of_the_launch():
    assert M.tile() == 2048
    for dtype in (torch.float32, torch.float64):
        for flen in range(2, 21, 2):
            d = M.max_depth(dtype, flen, "swt")
            assert (2 ** d - 1) * (flen - 1) <= 2048 < (2 ** (d + 1) - 1) * (flen - 1), (flen, d)
            assert M.max_depth(dtype, flen, "dwt") == 32
        assert M.max_depth(dtype, 8) == 8 and M.max_depth(dtype, 20) == 6 and M.max_depth(dtype, 2) == 11
        assert M.max_depth(dtype, 22) == 0 and M.max_depth(dtype, 22, "dwt") == 0 and M.max_depth(dtype, 7) == 0
    assert M.max_depth(torch.float16, 8) == 0 and M.max_depth(torch.bfloat16, 8, "dwt") == 0 and M.max_depth(torch.complex64, 8) == 0
    with pytest.raises(ValueError):
        M.max_depth(torch.float32, 8, "cwt")


def test_entries_refuse_before_a_launch():
    """Every refusal of the two launch entries comes before anything is enqueued: callable without a device."""
    lib = M._lib()
    band = (_engine.MraBand * 1)()
    band[0].x, band[0].row_stride, band[0].index, band[0].depth, band[0].detail = 64, 8, 0, 1, 1
    taps = _engine._taps_array([0.5, 0.5])
    out = 64  # (never dereferenced: every call below is refused)
    assert lib.mifwt_mra_swt(0, 2, 1, 8, band, 1, None, 8, 8, taps, taps, None) == -1
    assert lib.mifwt_mra_swt(0, 3, 1, 8, band, 1, out, 8, 8, taps, taps, None) == -1
    assert lib.mifwt_mra_swt(0, 22, 1, 8, band, 1, out, 8, 8, taps, taps, None) == -2
    assert lib.mifwt_mra_swt(2, 2, 1, 8, band, 1, out, 8, 8, taps, taps, None) == -2
    assert lib.mifwt_mra_swt(7, 2, 1, 8, band, 1, out, 8, 8, taps, taps, None) == -1
    assert lib.mifwt_mra_swt(0, 2, 1, 8, band, 0, out, 8, 8, taps, taps, None) == -1
    band[0].depth = 12  # haar takes 11
    assert lib.mifwt_mra_swt(0, 2, 1, 8, band, 1, out, 8, 8, taps, taps, None) == -2
    band[0].depth = 0
    assert lib.mifwt_mra_swt(0, 2, 1, 8, band, 1, out, 8, 8, taps, taps, None) == -1
    band[0].depth = 2
    import ctypes

    def lens(*v):
        return (ctypes.c_int64 * len(v))(*v)

    assert lib.mifwt_mra_dwt(0, 2, 1, 1, lens(8, 4, 3), 2, band, 1, out, 8, 8, taps, taps, None) == -1  # 4 is not 2 * 3 or one less
    assert lib.mifwt_mra_dwt(0, 4, 0, 1, lens(8, 5, 3), 2, band, 1, out, 8, 8, taps, taps, None) == -1  # 5 is not 2 * 3 - 2 or one less
    assert lib.mifwt_mra_dwt(0, 2, 1, 1, lens(8, 4), 1, band, 1, out, 8, 8, taps, taps, None) == -1  # a band deeper than the table
    assert lib.mifwt_mra_dwt(0, 2, 1, 1, None, 1, band, 1, out, 8, 8, taps, taps, None) == -1


def test_c_abi_surface():
    with open(os.path.join(ROOT, "include", "mifwt.h")) as f:
        header = f.read()
    lib = _engine.load_library()
    for name in _engine.MRA_ENTRIES:
        assert re.search(r"\b%s\(" % name, header), name
        getattr(lib, name)
    assert "#define MIFWT_KID_MRA_SWT 63" in header and "#define MIFWT_KID_MRA_DWT 64" in header
    assert (M.KID_MRA_SWT, M.KID_MRA_DWT) == (63, 64)
    with open(os.path.join(ROOT, "__graft_entry__.py")) as f:
        entry = f.read()
    assert all('"%s"' % name in entry for name in _engine.MRA_ENTRIES)


# ---- the public calls --------------------------------------------------------------------------------------------------------------------
def test_errors_of_mra(oracle_engine):
    x = _x(32)
    with pytest.raises(ValueError, match="transform"):
        ptwt_amd.mra(x, "haar", 2, transform="cwt")
    with pytest.raises(ValueError):
        ptwt_amd.mra(x.to(torch.int32), "haar", 2)  # the analysis call's dtype check
    with pytest.raises(ValueError):
        ptwt_amd.mra(x.to(torch.int32), "haar", 2, transform="dwt", mode="reflect")
    with pytest.raises(ValueError):
        ptwt_amd.mra(x, "haar", 2, transform="dwt", mode="no such mode")
    with pytest.raises(RuntimeError):
        ptwt_amd.mra(_x(5), "db4", 1, transform="dwt", mode="reflect")  # the pad check of wavedec
    with pytest.raises(ValueError):
        ptwt_amd.mra(x, "haar", 2, axis=(0, 1))
    assert "mra" in ptwt_amd.__all__ and "imra" in ptwt_amd.__all__ and "ptwt_amd.mra" in M.__name__ and "mra" in ptwt_amd.__doc__


def test_level_zero_gives_the_data(oracle_engine):
    x = _x(33)  # an odd length: swt's default level is 0
    for parts in (ptwt_amd.mra(x, "db4"), ptwt_amd.mra(x, "db4", 0), ptwt_amd.mra(x, "db4", 0, transform="dwt", mode="reflect")):
        assert len(parts) == 1 and parts[0] is x


@pytest.mark.parametrize("transform,mode", [("swt", "periodization"), ("dwt", "reflect"), ("dwt", "zero")])
def test_composed_route_on_the_oracle_engine(oracle_engine, transform, mode):
    """The definition written with the public calls, on CPU tensors through the numpy level stand-ins: the reference's components."""
    for n, axis in ((64, -1), (37 if transform == "dwt" else 24, 0)):
        x = _x(n, rows=3)
        data = x if axis == -1 else x.t().contiguous()
        parts = ptwt_amd.mra(data, "db4", 2, axis=axis, transform=transform, mode=mode)
        want = R.mra(data, "db4", 2, transform, mode, axis=axis)
        assert len(parts) == 3
        for p, w in zip(parts, want):
            assert p.shape == data.shape and p.dtype == data.dtype
            assert R.relerr(p, w, float(x.norm())) < F64_TOL
        assert R.relerr(ptwt_amd.imra(parts), data) < F64_TOL
        again = M._composed(data, "db4", 2, axis, transform, mode)
        assert all(torch.equal(p, q) for p, q in zip(parts, again))


def test_composed_route_is_differentiable(oracle_engine):
    x = _x(32).requires_grad_(True)
    parts = ptwt_amd.mra(x, "db2", 2)
    w = [torch.cos(0.3 * torch.arange(p.numel(), dtype=torch.float64) + i).reshape(p.shape) for i, p in enumerate(parts)]
    (g,) = torch.autograd.grad(sum((a * p).sum() for a, p in zip(w, parts)), x)
    xr = x.detach().clone().requires_grad_(True)
    (gr,) = torch.autograd.grad(sum((a * p).sum() for a, p in zip(w, R.mra(xr, "db2", 2))), xr)
    assert R.relerr(g, gr) < 1e-10


def test_imra_on_cpu_tensors():
    parts = [torch.full((2, 3), float(v)) for v in (1e8, 1.0, -1e8)]
    assert torch.equal(ptwt_amd.imra(parts), (parts[0] + parts[1]) + parts[2])  # left to right: 0 in float32, not 1
    assert torch.equal(ptwt_amd.imra([parts[1]]), parts[1])
    assert torch.equal(ptwt_amd.imra(tuple(parts[:2])), parts[0] + parts[1])
    with pytest.raises(ValueError):
        ptwt_amd.imra([])
    with pytest.raises(ValueError):
        ptwt_amd.imra([parts[0], torch.zeros(3, 2)])
    with pytest.raises(ValueError):
        ptwt_amd.imra([parts[0], parts[1].double()])
    with pytest.raises(ValueError):
        ptwt_amd.imra([parts[0], parts[1].to("meta")])
    with pytest.raises(ValueError):
        ptwt_amd.imra([parts[0], 1.0])
