"""Host tests (no GPU) of the periodized transform: the torch reference tests/_per_ref.py against PyWavelets' goldens, against the
emulation on the padded "periodic" level of the oracle, its adjoint identities and orthogonality; the argument errors of
``mode="periodization"``; the C ABI (header, exported symbols, ``mifwt_per_supported``).

Errors are norm-wise per tensor (``_per_ref.relerr``).  Only a band that is ZERO in exact arithmetic — the details of an axis of one
sample, a cancellation sum of the taps; ``_per_ref.ZERO_BAND`` — is measured relative to the norm of the transform's input, the scale
its rounding has.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ptwt_amd
from oracle import fwt_oracle as O
from ptwt_amd import _engine, _per
from ptwt_amd._wavelets import host_taps
from tests import _per_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mifwt_per_supported", "mifwt_per_kernel_id", "mifwt_per_fwd", "mifwt_per_inv", "mifwt_per_axis_fwd", "mifwt_per_axis_inv")


def scaled_err(got, want, scale):
    return R.relerr(got, want, float(scale))


def test_reference_matches_pywavelets():
    worst = 0.0
    for c in R.goldens():
        bank = host_taps(c["wavelet"])
        coeffs = R.wavedecn(c["x"], bank, c["ndim"], c["level"])
        got = R.flat_ref(coeffs, c["ndim"])
        assert set(got) == set(c["coeffs"])
        scale = c["x"].norm()
        for k, t in got.items():
            assert t.shape == c["coeffs"][k].shape, (c["wavelet"], c["shape"], k)
            worst = max(worst, scaled_err(t, c["coeffs"][k], scale))
        rec = R.waverecn(coeffs, bank, c["ndim"])
        assert rec.shape == c["rec"].shape
        worst = max(worst, scaled_err(rec, c["rec"], scale))
        # (reconstruction is exact: the input, an odd extent extended by its last sample)
        ext = c["x"]
        for a, n in enumerate(c["shape"]):
            if n % 2:
                ext = torch.cat([ext, ext.narrow(a, n - 1, 1)], a)
        worst = max(worst, scaled_err(rec, ext, scale))
    print("reference vs PyWavelets goldens, worst: %.3e" % worst)
    assert worst < 1e-12


def test_goldens_shapes_are_ceil_halves():
    for c in R.goldens():
        n = list(c["shape"])
        for lvl in range(c["level"]):
            n = [(v + 1) // 2 for v in n]
            name = {1: "%d", 2: "%d_d", 3: "%d_ddd"}[c["ndim"]] % (c["level"] - 1 - lvl)
            assert tuple(c["coeffs"][name].shape) == tuple(n)
        assert tuple(c["coeffs"]["a"].shape) == tuple(n)


@pytest.mark.parametrize("flen", list(range(2, 21, 2)))
def test_reference_matches_emulation_on_periodic_level(flen):
    """Even N: per(x)[k] = periodic_level(roll(x, -(L/2 - 1)))[k] for k < N/2 — a second, independent check through the oracle."""
    g = np.random.default_rng(100 + flen)
    lo, hi = g.standard_normal(flen), g.standard_normal(flen)
    for n in (flen + (flen & 1) + 2, 32, 66):
        if flen - 2 > n:  # (the padded level refuses a circular pad beyond one period)
            continue
        x = g.standard_normal((3, n))
        ca, cd = R.dwt_axis(torch.from_numpy(x), lo, hi, -1)
        ea, ed = O.dwt_axis(np.roll(x, -(flen // 2 - 1), axis=-1), lo, hi, "periodic", -1)
        assert R.relerr(ca, torch.from_numpy(ea[..., : n // 2])) < 1e-13
        assert R.relerr(cd, torch.from_numpy(ed[..., : n // 2])) < 1e-13


@pytest.mark.parametrize("n", [1, 2, 3, 7, 16, 33])
@pytest.mark.parametrize("wavelet", ["haar", "db4", "bior3.5", "db10"])
def test_adjoint_identities(n, wavelet):
    """<A x, c> = <x, A^T c> with A^T = synthesis with the reversed dec taps over N~ samples + the virtual sample folded onto N - 1;
    <S c, y> = <c, S^T y> with S^T = analysis with the reversed rec taps."""
    dec_lo, dec_hi, rec_lo, rec_hi = host_taps(wavelet)
    g = torch.Generator().manual_seed(n)
    m = (n + 1) // 2
    x = torch.randn(2, n, generator=g, dtype=torch.float64)
    ca, cd = torch.randn(2, m, generator=g, dtype=torch.float64), torch.randn(2, m, generator=g, dtype=torch.float64)
    a, d = R.dwt_axis(x, dec_lo, dec_hi, -1)
    at = R.idwt_axis(ca, cd, dec_lo[::-1], dec_hi[::-1], -1)
    if n % 2:
        at = torch.cat([at[:, : n - 1], at[:, n - 1 : n] + at[:, n : n + 1]], -1)
    lhs, rhs = float((a * ca).sum() + (d * cd).sum()), float((x * at).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    y = torch.randn(2, 2 * m, generator=g, dtype=torch.float64)
    s = R.idwt_axis(ca, cd, rec_lo, rec_hi, -1)
    sa, sd = R.dwt_axis(y, rec_lo[::-1], rec_hi[::-1], -1)
    lhs, rhs = float((s * y).sum()), float((sa * ca).sum() + (sd * cd).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0)
    # and autograd of the reference agrees with the first identity
    xr = x.clone().requires_grad_(True)
    a, d = R.dwt_axis(xr, dec_lo, dec_hi, -1)
    ((a * ca).sum() + (d * cd).sum()).backward()
    assert R.relerr(xr.grad, at) < 1e-12


def test_orthogonality_db4():
    dec_lo, dec_hi, _, _ = host_taps("db4")
    a = R.matrix(16, dec_lo, dec_hi)
    assert float((a @ a.T - torch.eye(16, dtype=torch.float64)).abs().max()) < 1e-12


# ---- argument errors --------------------------------------------------------------------------------------------------------------------
def test_cpu_tensor_is_refused():
    x = torch.randn(2, 13, 10)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.wavedec2(x, "db2", mode="periodization")
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.wavedec(x, "db2", mode="periodization")
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.waverec([x, x], "db2", mode="periodization")


def test_float16_is_refused():
    x = torch.randn(2, 16, 16).half()
    with pytest.raises(ValueError, match="not supported"):
        ptwt_amd.wavedec2(x, "db2", mode="periodization")
    with ptwt_amd.half_storage():
        with pytest.raises(ValueError, match="Input dtype .* not supported"):
            ptwt_amd.wavedec2(x, "db2", mode="periodization")
        with pytest.raises(ValueError, match="Input dtype .* not supported"):
            ptwt_amd.fswaverec2((x, {"ad": x, "da": x, "dd": x}), "db2", mode="periodization")


def test_learnable_and_device_taps_are_refused():
    x = torch.randn(2, 16, 16)
    bank = tuple(torch.tensor(t, dtype=torch.float32) for t in host_taps("db2"))
    learnable = tuple(t.clone().requires_grad_(True) for t in bank)
    with pytest.raises(NotImplementedError, match="learnable"):
        ptwt_amd.wavedec2(x, learnable, mode="periodization")
    with pytest.raises(NotImplementedError, match="learnable"):
        ptwt_amd.waverec2((x, (x, x, x)), learnable, mode="periodization")
    ptwt_amd.set_device_taps("always")
    try:
        with pytest.raises(NotImplementedError, match="device-resident"):
            ptwt_amd.wavedec2(x, bank, mode="periodization")
    finally:
        ptwt_amd.set_device_taps("auto")
    with pytest.raises(RuntimeError, match="ROCm device"):  # (tensor taps that need no gradient are read on the host: accepted)
        ptwt_amd.wavedec2(x, bank, mode="periodization")


def test_unknown_modes_keep_their_errors():
    x = torch.randn(2, 16, 16)
    with pytest.raises(ValueError, match="Padding mode not supported"):
        ptwt_amd.waverec2((x, (x, x, x)), "db2", mode="periodisation")
    with pytest.raises(ValueError):
        ptwt_amd.MatrixWavedec("db2", level=1, odd_coeff_padding_mode="periodization")(torch.randn(2, 15))
    assert "periodization" not in _engine.MODE_IDS


def test_negative_level_is_refused():
    x = torch.randn(2, 16, 16)
    with pytest.raises(ValueError, match="Level value"):
        ptwt_amd.wavedec2(x, "db2", mode="periodization", level=-1)


@pytest.mark.parametrize("order", ["3d-first", "2d-first"])
def test_level_plans_are_keyed_by_every_stride_set(order, monkeypatch):
    """The fused launch inside a 3-D level (depth folded into the batch, planes of its own temporary) and a 2-D level on a tensor of the
    folded shape have the same signal geometry and different band strides: each must get the descriptor of ITS buffers, whichever runs
    first.  No device: the launches are recorded instead of made."""
    seen = []
    monkeypatch.setattr(_engine, "_require_gpu", lambda t: None)
    monkeypatch.setattr(_engine, "_run", lambda tag, kid, extent, anchor, entry, args, **kw: seen.append((kid, args)) or 0)
    _per._plans.clear()
    lo, hi = host_taps("db2")[:2]
    calls = {"3d": lambda: _per.level_fwd(torch.zeros(2, 9, 8, 12), lo, hi), "2d": lambda: _per.level_fwd(torch.zeros(18, 8, 12), lo, hi)}
    want = {"3d": (24, 6, 1), "2d": (96, 6, 1)}  # band (batch, row, sample) strides: planes [4, 18, 4, 6] against a buffer [18, 4, 4, 6]
    try:
        for which in (("3d", "2d") if order == "3d-first" else ("2d", "3d")):
            del seen[:]
            calls[which]()
            fused = [args for kid, args in seen if kid == _per.KID_FWD]
            assert len(fused) == 1
            d = fused[0][0]._obj
            assert (tuple(d.approx_stride[:3]), tuple(d.detail_stride[:3])) == (want[which], want[which]), (order, which)
            assert (d.batch, tuple(d.sig_extent[:2]), tuple(d.coef_extent[:2])) == (18, (8, 12), (4, 6))
    finally:
        _per._plans.clear()


@pytest.mark.parametrize("n", [1, 2, 3, 5, 8, 16])
def test_summing_the_aliasing_taps_is_the_same_map(n):
    """``_per._taps`` hands a launch over an axis shorter than the filter the taps that meet the same sample summed in double (same
    length, zeros behind the period): in float64 the same level to rounding, analysis and synthesis; longer axes get the bank as it is."""
    g = np.random.default_rng(n)
    flen, m = 18, (n + 1) // 2
    bank = [tuple(g.standard_normal(flen)) for _ in range(4)]
    folded = [list(t) for t in (*_per._taps(bank[0], bank[1], [2 * m]), *_per._taps(bank[2], bank[3], [2 * m]))]
    assert all(len(t) == flen and not any(t[2 * m:]) for t in folded)
    x = torch.from_numpy(g.standard_normal((3, n)))
    for a, b in zip(R.level_fwd(x, folded, 1), R.level_fwd(x, bank, 1)):
        assert R.relerr(a, b) < 1e-13
    c = [torch.from_numpy(g.standard_normal((3, m))) for _ in range(2)]
    assert R.relerr(R.level_inv(c, folded, 1), R.level_inv(c, bank, 1)) < 1e-13
    assert [list(t) for t in _per._taps(bank[0], bank[1], [18])] == [list(bank[0]), list(bank[1])]
    assert [list(t) for t in _per._taps(bank[0], bank[1], [4, 6])] == [list(bank[0]), list(bank[1])]  # (one bank per launch)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_header_and_library_export_the_symbols():
    with open(os.path.join(ROOT, "include", "mifwt.h")) as f:
        header = f.read()
    lib = _engine.load_library()
    for sym in SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert getattr(lib, sym) is not None
    for name, kid in (("MIFWT_KID_PER_FWD", 38), ("MIFWT_KID_PER_INV", 39), ("MIFWT_KID_PER_AXIS_FWD", 40), ("MIFWT_KID_PER_AXIS_INV", 41)):
        assert re.search(r"#define %s %d\b" % (name, kid), header)
    assert lib.mifwt_abi_version() == 3
    assert "#define MIFWT_ABI_VERSION 3" in header


def _desc(dtype, flen, sig, coef=None, last=1):
    nd = len(sig)
    coef = [(n + 1) // 2 for n in sig] if coef is None else coef
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


def test_per_supported_answers_on_the_host():
    lib = _per._lib()  # (the entries with their argument types, _engine.PER_ENTRIES)

    def ask(d, direction):
        return lib.mifwt_per_supported(ctypes.byref(d), direction), lib.mifwt_per_kernel_id(ctypes.byref(d), direction)

    for direction, kid in ((0, 38), (1, 39)):
        assert ask(_desc(torch.float32, 20, [1, 1]), direction) == (1, kid)
        assert ask(_desc(torch.float64, 2, [7]), direction) == (1, kid)
        assert ask(_desc(torch.float32, 22, [1, 1]), direction) == (0, -2)
        assert ask(_desc(torch.float16, 8, [16, 16]), direction) == (0, -2)
        assert ask(_desc(torch.float32, 8, [16, 16], last=2), direction) == (0, -2)
        assert ask(_desc(torch.float32, 8, [4, 5, 6]), direction) == (0, -2)
        assert ask(_desc(torch.float32, 8, [13, 10], coef=[6, 5]), direction) == (-1, -1)
        assert ask(_desc(torch.float32, 8, [13, 10], coef=[7, 6]), direction) == (-1, -1)
        assert ask(_desc(torch.float32, 7, [13, 10]), direction) == (-1, -1)
    assert lib.mifwt_per_supported(ctypes.byref(_desc(torch.float32, 8, [16, 16])), 2) == -1
    # outside the envelope the fused entries launch nothing (null pointers never reach a kernel: the refusal comes first for valid ones)
    d = _desc(torch.float32, 22, [4, 4])
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    det = (ctypes.c_void_p * 3)(p, p, p)
    taps = (ctypes.c_double * 22)()
    before = [_engine.launch_count(k) for k in (38, 39)]
    assert lib.mifwt_per_fwd(ctypes.byref(d), p, p, det, taps, taps, None) == -2
    assert lib.mifwt_per_inv(ctypes.byref(d), p, det, p, taps, taps, None) == -2
    assert [_engine.launch_count(k) for k in (38, 39)] == before
    # a null descriptor, then a null data or tap pointer on a served descriptor: each is refused before any launch
    assert (lib.mifwt_per_supported(None, 0), lib.mifwt_per_kernel_id(None, 1)) == (-1, -1)
    assert lib.mifwt_per_fwd(None, p, p, det, taps, taps, None) == -1
    assert lib.mifwt_per_inv(None, p, det, p, taps, taps, None) == -1
    ok = _desc(torch.float32, 8, [4, 4])
    null_det = (ctypes.c_void_p * 3)(p, None, p)
    for args in ((None, p, det, taps, taps), (p, None, det, taps, taps), (p, p, None, taps, taps), (p, p, null_det, taps, taps),
                 (p, p, det, None, taps), (p, p, det, taps, None)):
        assert lib.mifwt_per_fwd(ctypes.byref(ok), *args, None) == -1, args
    for args in ((None, det, p, taps, taps), (p, None, p, taps, taps), (p, null_det, p, taps, taps), (p, det, None, taps, taps),
                 (p, det, p, None, taps), (p, det, p, taps, None)):
        assert lib.mifwt_per_inv(ctypes.byref(ok), *args, None) == -1, args
    assert [_engine.launch_count(k) for k in (38, 39)] == before
    # the axis entries: a null data, stride or tap pointer (-1); float16 with valid pointers is outside their envelope (-2, nothing launched)
    st = (ctypes.c_int64 * 3)(8, 1, 1)
    before = [_engine.launch_count(k) for k in (40, 41)]
    for entry in (lib.mifwt_per_axis_fwd, lib.mifwt_per_axis_inv):
        good = [p, st, p, st, p, st, taps, taps]
        for hole in range(len(good)):
            assert entry(0, 8, 1, 8, 1, *[None if i == hole else v for i, v in enumerate(good)], None) == -1, hole
        assert entry(2, 8, 1, 8, 1, *good, None) == -2
        assert entry(0, 7, 1, 8, 1, *good, None) == -1
    assert [_engine.launch_count(k) for k in (40, 41)] == before
