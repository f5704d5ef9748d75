"""Host-side tests of the boundary-wavelet transforms (no GPU): the boundary tables against the reference's matrices
(tests/golden/ptwt_ref_boundary.npz, group "blocks"), the public interface and its errors, the host half of the C ABI, and the
float64 level operators as a reference chain (tests/_boundary_ref.py) against the reference's classes at mid sizes
(tests/golden/ptwt_ref_boundary_mid.npz)."""
import ctypes
import inspect
import io
import contextlib

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _boundary, _bwt, _engine
from ptwt_amd._wavelets import host_taps
from tests import _golden as G

WAVELETS = ("haar", "db2", "db3", "db4", "sym5", "db8", "db10", "coif2", "bior2.2")


def test_tables_match_the_reference_blocks():
    """gramschmidt: exact in sign; qr: up to one sign per row.  1e-12 on entries (the reference's two methods differ from one another
    by at most 4e-14 for L <= 20)."""
    z, idx = G.load("ptwt_ref_boundary.npz")
    blocks = [c for c in idx if c["group"] == "blocks"]
    assert {c["wavelet"] for c in blocks} == set(WAVELETS) and {c["method"] for c in blocks} == {"qr", "gramschmidt"}
    flipped = 0
    for case in blocks:
        taps = host_taps(case["wavelet"])
        nt, nb = _boundary.boundary_rows(case["filt_len"])
        for which in ("analysis", "synthesis"):
            got = _boundary.boundary_blocks(taps, case["method"], which)
            for band in ("lo", "hi"):
                for end, rows in (("top", nt), ("bot", nb)):
                    want = z["%s_%s_%s_%s" % (case["key"], which, band, end)]
                    mine = got["%s_%s" % (band, end)]
                    assert mine.shape == want.shape == (rows, case["filt_len"] - 1)
                    if case["method"] == "qr":
                        s = np.sign((mine * want).sum(axis=1))
                        flipped += int((s < 0).sum())
                        mine = mine * s[:, None]
                    assert np.abs(mine - want).max(initial=0.0) < 1e-12, (case, which, band, end)
    assert flipped > 0  # (the reference's qr signs do differ from the Gram-Schmidt signs somewhere: the rule above is exercised)


@pytest.mark.parametrize("wavelet", ["db12", "db16", "db20"])
def test_long_filters_are_orthogonal_to_1e_9(wavelet):
    """No golden for L > 20: the reference's classical Gram-Schmidt has lost orthogonality there (1e-12 at L = 24, 6e-5 at L = 40, which
    would fail this bound); its QR reaches 1.5e-11 at L = 40."""
    taps = host_taps(wavelet)
    L = len(taps[0])
    for n in (2 * (L - 1), 4 * L + 2):
        a = _boundary.level_matrix(taps, n, "qr", "analysis")
        assert np.abs(a @ a.T - np.eye(n)).max() < 1e-9
        s = _boundary.level_matrix(taps, n, "gramschmidt", "synthesis")
        assert np.abs(s @ a - np.eye(n)).max() < 1e-9


def test_blocks_do_not_depend_on_the_length_and_short_levels_are_orthogonal():
    for wavelet in WAVELETS:
        taps = host_taps(wavelet)
        L = len(taps[0])
        nt, nb = _boundary.boundary_rows(L)
        blocks = _boundary.boundary_blocks(taps, "qr", "analysis")
        assert blocks is _boundary.boundary_blocks(taps, "gramschmidt", "analysis")  # cached per bank, both methods
        for n in (2 * (L - 1), 2 * (L - 1) + 2, 6 * L, 6 * L + 2):
            if n < 2:
                continue
            a = _boundary.level_matrix(taps, n, "qr", "analysis")
            h = n // 2
            for off, band in ((0, "lo"), (h, "hi")):
                assert np.array_equal(a[off:off + nt, : L - 1], blocks[band + "_top"])
                assert np.array_equal(a[off + h - nb:off + h, n - L + 1:], blocks[band + "_bot"])
                assert not a[off:off + nt, L - 1:].any() and not a[off + h - nb:off + h, : n - L + 1].any()
        if not wavelet.startswith("bior"):
            for n in range(L + (L % 2), 2 * (L - 1), 2):  # L <= N < 2 (L - 1): the two ends overlap
                a = _boundary.level_matrix(taps, n, "qr", "analysis")
                assert np.abs(a @ a.T - np.eye(n)).max() < 1e-12, (wavelet, n)
        tab = _boundary.kernel_tables(taps, "qr", "analysis")
        assert tab.shape == (2, max(nt + nb, 1), L) and not tab[:, :nt, L - 1].any() and not tab[:, nt:nt + nb, 0].any()


def test_exports_signatures_and_defaults():
    for name in ("MatrixWavedec", "MatrixWaverec", "MatrixWavedec2", "MatrixWaverec2"):
        assert name in ptwt_amd.__all__ and hasattr(ptwt_amd, name)
    from ptwt_amd import matmul_transform, matmul_transform_2

    assert matmul_transform.MatrixWavedec is ptwt_amd.MatrixWavedec and matmul_transform_2.MatrixWaverec2 is ptwt_amd.MatrixWaverec2

    def params(cls):
        return {k: (v.kind, v.default) for k, v in inspect.signature(cls.__init__).parameters.items() if k != "self"}

    P, K = inspect.Parameter.POSITIONAL_OR_KEYWORD, inspect.Parameter.KEYWORD_ONLY
    assert params(ptwt_amd.MatrixWavedec) == {"wavelet": (P, inspect.Parameter.empty), "level": (P, None), "axis": (K, None),
                                              "orthogonalization": (K, "qr"), "odd_coeff_padding_mode": (K, "zero")}
    assert params(ptwt_amd.MatrixWaverec) == {"wavelet": (P, inspect.Parameter.empty), "axis": (K, None), "orthogonalization": (K, "qr")}
    assert params(ptwt_amd.MatrixWavedec2) == {"wavelet": (P, inspect.Parameter.empty), "level": (P, None), "axes": (K, None),
                                               "orthogonalization": (K, "qr"), "separable": (K, True),
                                               "odd_coeff_padding_mode": (K, "zero")}
    assert params(ptwt_amd.MatrixWaverec2) == {"wavelet": (P, inspect.Parameter.empty), "axes": (K, None), "orthogonalization": (K, "qr"),
                                               "separable": (K, True)}
    dec = ptwt_amd.MatrixWavedec("db2", 3)
    assert (dec.level, dec.input_length, dec.padded, dec.size_list, dec.pad_list, dec.axis) == (3, None, False, [], [], -1)
    dec2 = ptwt_amd.MatrixWavedec2("db2")
    assert (dec2.level, dec2.padded, dec2.size_list, dec2.pad_list, dec2.axes, dec2.separable) == (None, False, [], [], (-2, -1), True)
    rec = ptwt_amd.MatrixWaverec("db2")
    assert (rec.level, rec.input_length, rec.padded) == (None, None, False)


def test_errors_come_before_any_gpu_work():
    for cls in (ptwt_amd.MatrixWavedec, ptwt_amd.MatrixWaverec, ptwt_amd.MatrixWavedec2, ptwt_amd.MatrixWaverec2):
        with pytest.raises(NotImplementedError):
            cls("db2", orthogonalization="householder")
        with pytest.raises(ValueError, match="same length"):
            cls((torch.ones(4), torch.ones(4), torch.ones(6), torch.ones(6)))
        with pytest.warns(DeprecationWarning):
            obj = cls("db2", boundary="gramschmidt")
        assert obj.orthogonalization == "gramschmidt"
        with pytest.raises(TypeError):
            cls("db2", boundary="qr", orthogonalization="qr")
    for cls in (ptwt_amd.MatrixWavedec2, ptwt_amd.MatrixWaverec2):
        with pytest.raises(NotImplementedError, match="Kronecker"):
            cls("db2", separable=False)
    with pytest.raises(NotImplementedError):
        ptwt_amd.MatrixWavedec2("db2").sparse_fwt_operator
    with pytest.raises(NotImplementedError):
        ptwt_amd.MatrixWaverec2("db2").sparse_ifwt_operator
    with pytest.raises(ValueError, match="Call this object first"):
        ptwt_amd.MatrixWavedec("db2").sparse_fwt_operator
    with pytest.raises(ValueError, match="Call this object first"):
        ptwt_amd.MatrixWaverec("db2").sparse_ifwt_operator
    x1, x2 = torch.randn(3, 64), torch.randn(3, 32, 32)
    for level in (0, -2):
        with pytest.raises(ValueError, match="positive integer"):
            ptwt_amd.MatrixWavedec("db2", level)(x1)
        with pytest.raises(ValueError, match="positive integer"):
            ptwt_amd.MatrixWavedec2("db2", level)(x2)
    with pytest.raises(ValueError, match="same shape"):
        ptwt_amd.MatrixWaverec("db2")([torch.randn(3, 8), torch.randn(3, 9)])
    with pytest.raises(ValueError, match="same shape"):
        ptwt_amd.MatrixWaverec2("db2")((torch.randn(3, 8, 8), ptwt_amd.WaveletDetailTuple2d(*(torch.randn(3, 8, 9) for _ in range(3)))))
    with pytest.raises(ValueError, match="3-tuple"):
        ptwt_amd.MatrixWaverec2("db2")((torch.randn(3, 8, 8), torch.randn(3, 8, 8)))
    with pytest.raises(ValueError, match="Padding mode not supported"):
        ptwt_amd.MatrixWavedec("db2", 1, odd_coeff_padding_mode="antireflect")(torch.randn(3, 33))
    # a CPU tensor: the package's usual refusal, after the argument checks
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.MatrixWavedec("db2", 2)(x1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.MatrixWavedec2("db2", 2)(x2)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.MatrixWaverec("db2")([torch.randn(3, 8), torch.randn(3, 8)])
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.MatrixWaverec2("db2")((torch.randn(3, 8, 8), ptwt_amd.WaveletDetailTuple2d(*(torch.randn(3, 8, 8) for _ in range(3)))))
    with pytest.raises(ValueError):
        ptwt_amd.MatrixWavedec("db2", 1)(torch.randn(2, 64).half())
    # the packet trees still refuse the boundary mode
    with pytest.raises(NotImplementedError):
        ptwt_amd.WaveletPacket(torch.randn(2, 64), "db2", mode="boundary")


def test_level_bookkeeping_and_the_too_deep_warning():
    """level=None is int(log2(N / (L - 1))); a level whose input is shorter than L is not computed (stderr warning)."""
    dec = ptwt_amd.MatrixWavedec("db4", 5)
    err = io.StringIO()
    with contextlib.redirect_stderr(err), pytest.raises(RuntimeError, match="ROCm device"):
        dec(torch.randn(2, 40))
    assert "too large" in err.getvalue() and "level 3" in err.getvalue()
    assert dec.size_list == [40, 20, 10, 5] and dec.pad_list == [False, False, False] and not dec.padded and dec.input_length == 40
    dec = ptwt_amd.MatrixWavedec("db3", None)
    with pytest.raises(RuntimeError):
        dec(torch.randn(97))
    assert dec.level == int(np.log2(98 / 5)) == 4 and dec.input_length == 98
    assert dec.size_list == [98, 50, 26, 14, 7] and dec.pad_list == [False, True, True, True] and dec.padded
    dec2 = ptwt_amd.MatrixWavedec2("db2", None)
    with pytest.raises(RuntimeError):
        dec2(torch.randn(33, 47))
    assert dec2.level == 3 and dec2.size_list == [(34, 48), (18, 24), (10, 12), (5, 6)]
    assert dec2.pad_list == [(True, True), (False, True), (False, True)] and dec2.padded


def _desc(ndim, dtype, flen, batch, sig, mode=0, coef=None, inner=1):
    d = _engine.LevelDesc()
    d.ndim, d.dtype, d.mode, d.filt_len, d.batch = ndim, dtype, mode, flen, batch
    coef = coef or [(n + 1) // 2 for n in sig]
    s, c = inner, inner
    for a in reversed(range(ndim)):
        d.sig_extent[a], d.coef_extent[a] = sig[a], coef[a]
        d.sig_stride[1 + a], d.approx_stride[1 + a], d.detail_stride[1 + a] = s, c, c
        s, c = s * sig[a], c * coef[a]
    d.sig_stride[0], d.approx_stride[0], d.detail_stride[0] = s, c * (1 << ndim), c * (1 << ndim)
    return d


def test_c_abi_host_side():
    lib = _bwt._lib()
    for sym in ("mifwt_bwt_fwd", "mifwt_bwt_inv", "mifwt_bwt_supported", "mifwt_bwt_kernel_id", "mifwt_bwt_axis_fwd", "mifwt_bwt_axis_inv"):
        assert hasattr(lib, sym)
    assert lib.mifwt_abi_version() == 3 == _engine.ABI_VERSION
    F32, F64, F16 = 0, 1, 2
    OK, BADARG, UNSUPPORTED = 0, -1, -2

    def kid(d, direction):
        return lib.mifwt_bwt_kernel_id(ctypes.byref(d), direction), lib.mifwt_bwt_supported(ctypes.byref(d), direction)

    for dtype in (F32, F64):
        for L in range(2, 22, 2):
            assert kid(_desc(1, dtype, L, 7, [4096]), 0) == (26, 1)
            assert kid(_desc(1, dtype, L, 7, [4095]), 1) == (27, 1)
            assert kid(_desc(2, dtype, L, 3, [101, 64], mode=4), 0) == (26, 1)
            assert kid(_desc(2, dtype, L, 3, [64, 77]), 1) == (27, 1)
    assert kid(_desc(1, F32, 8, 2, [14]), 0) == (26, 1)                     # N = 2 (L - 1): the shortest axis with disjoint ends
    assert kid(_desc(1, F32, 8, 2, [12]), 0) == (UNSUPPORTED, 0)            # L <= N < 2 (L - 1): the dense route of the host layer
    assert kid(_desc(2, F64, 8, 2, [12, 64]), 1) == (UNSUPPORTED, 0)
    assert kid(_desc(1, F32, 22, 2, [4096]), 0) == (UNSUPPORTED, 0)         # long filters: the per-axis passes
    assert kid(_desc(1, F32, 32, 2, [4096]), 1) == (UNSUPPORTED, 0)
    assert kid(_desc(1, F16, 8, 2, [4096]), 0) == (UNSUPPORTED, 0)
    assert kid(_desc(3, F32, 4, 2, [32, 32, 32]), 0) == (UNSUPPORTED, 0)
    assert kid(_desc(1, F32, 8, 2, [4096], inner=2), 0) == (UNSUPPORTED, 0)  # non-unit innermost stride
    # inconsistent requests
    assert kid(_desc(1, F32, 8, 2, [4096], coef=[2051]), 0) == (BADARG, BADARG)  # the padded transform's extent, not ceil(N / 2)
    assert kid(_desc(1, F32, 8, 2, [4096], coef=[2047]), 1) == (BADARG, BADARG)
    assert kid(_desc(2, F32, 8, 2, [64, 63], coef=[32, 31]), 0) == (BADARG, BADARG)
    assert kid(_desc(1, F32, 7, 2, [4096]), 0) == (BADARG, BADARG)
    assert kid(_desc(1, F32, 8, 2, [6]), 0) == (BADARG, BADARG)              # shorter than the filter
    assert kid(_desc(1, 5, 8, 2, [4096]), 0) == (BADARG, BADARG)
    assert kid(_desc(1, F32, 8, 2, [4096], mode=9), 0) == (BADARG, BADARG)
    assert lib.mifwt_bwt_kernel_id(ctypes.byref(_desc(1, F32, 8, 2, [4096])), 2) == BADARG
    assert lib.mifwt_bwt_kernel_id(None, 0) == BADARG
    # the calls refuse before they launch: null pointers, inconsistent extents, a table of the wrong bank
    d = _desc(1, F32, 8, 2, [4096])
    taps = (ctypes.c_double * 8)(*host_taps("db4")[0])
    tab = _bwt.BwtTables(0, 2, 2)
    null_details = (ctypes.c_void_p * 1)(None)
    assert lib.mifwt_bwt_fwd(ctypes.byref(d), None, None, null_details, taps, taps, ctypes.byref(tab), None) == BADARG
    bad = _desc(1, F32, 8, 2, [4096], coef=[2051])
    assert lib.mifwt_bwt_fwd(ctypes.byref(bad), None, None, null_details, taps, taps, ctypes.byref(tab), None) == BADARG
    assert lib.mifwt_bwt_inv(ctypes.byref(bad), None, null_details, None, taps, taps, ctypes.byref(tab), None) == BADARG
    strides = (ctypes.c_int64 * 3)(4096, 1, 1)
    assert lib.mifwt_bwt_axis_fwd(F32, 8, 0, 2, 4096, 1, None, strides, None, strides, None, strides, taps, taps, ctypes.byref(tab), None) == BADARG
    # a null descriptor, then one null pointer at a time on a served descriptor (the table's rows are never read on the host)
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    det, null_det = (ctypes.c_void_p * 3)(p, p, p), (ctypes.c_void_p * 3)(p, None, p)
    tab, no_rows = ctypes.byref(_bwt.BwtTables(p.value, 2, 2)), ctypes.byref(_bwt.BwtTables(0, 2, 2))
    assert lib.mifwt_bwt_supported(None, 0) == BADARG
    assert lib.mifwt_bwt_fwd(None, p, p, det, taps, taps, tab, None) == BADARG
    assert lib.mifwt_bwt_inv(None, p, det, p, taps, taps, tab, None) == BADARG
    d2 = _desc(2, F32, 8, 1, [16, 16])
    for args in ((None, p, det, taps, taps, tab), (p, None, det, taps, taps, tab), (p, p, None, taps, taps, tab), (p, p, null_det, taps, taps, tab),
                 (p, p, det, None, taps, tab), (p, p, det, taps, None, tab), (p, p, det, taps, taps, None), (p, p, det, taps, taps, no_rows)):
        assert lib.mifwt_bwt_fwd(ctypes.byref(d2), *args, None) == BADARG, args
    for args in ((None, det, p, taps, taps, tab), (p, None, p, taps, taps, tab), (p, null_det, p, taps, taps, tab), (p, det, None, taps, taps, tab),
                 (p, det, p, None, taps, tab), (p, det, p, taps, None, tab), (p, det, p, taps, taps, None), (p, det, p, taps, taps, no_rows)):
        assert lib.mifwt_bwt_inv(ctypes.byref(d2), *args, None) == BADARG, args
    # outside the fused envelope with valid pointers: refused, nothing launched (a launch without a device could not answer UNSUPPORTED)
    long_taps = (ctypes.c_double * 22)()
    long_tab = ctypes.byref(_bwt.BwtTables(p.value, 5, 5))
    far = _desc(2, F32, 22, 1, [64, 64])
    assert lib.mifwt_bwt_fwd(ctypes.byref(far), p, p, det, long_taps, long_taps, long_tab, None) == UNSUPPORTED
    assert lib.mifwt_bwt_inv(ctypes.byref(far), p, det, p, long_taps, long_taps, long_tab, None) == UNSUPPORTED
    near = _desc(1, F32, 8, 2, [12])  # L <= N < 2 (L - 1)
    assert lib.mifwt_bwt_fwd(ctypes.byref(near), p, p, det, taps, taps, tab, None) == UNSUPPORTED
    # the axis entries: one null at a time (-1), float16 and overlapping ends with valid pointers (-2)
    st = (ctypes.c_int64 * 3)(16, 1, 1)
    good = [p, st, p, st, p, st, taps, taps, tab]
    for entry, head in ((lib.mifwt_bwt_axis_fwd, (8, 0)), (lib.mifwt_bwt_axis_inv, (8,))):
        for hole in range(len(good)):
            assert entry(F32, *head, 1, 16, 1, *[None if i == hole else v for i, v in enumerate(good)], None) == BADARG, hole
        assert entry(F32, *head, 1, 16, 1, *good[:-1], no_rows, None) == BADARG
        assert entry(F16, *head, 1, 16, 1, *good, None) == UNSUPPORTED
        assert entry(F32, *head, 1, 12, 1, *good, None) == UNSUPPORTED
        assert entry(F32, *head, 1, 6, 1, *good, None) == BADARG
    assert OK == 0


def test_bank_and_virtual_sample_rules():
    taps = host_taps("bior2.2")
    a, s = _bwt.bank(taps, "qr", "analysis"), _bwt.bank(taps, "gramschmidt", "synthesis")
    assert a is _bwt.bank(taps, "gramschmidt", "analysis") and a is not s
    assert a.f_lo == tuple(taps[0]) and s.f_lo == tuple(taps[2])[::-1] and (a.n_top, a.n_bot) == (1, 1)
    assert not np.array_equal(a._host_tab, s._host_tab)  # biorthogonal: S != A^T, an adjoint must not borrow the other tables
    o = host_taps("db3")
    assert np.array_equal(_bwt.bank(o, "qr", "analysis")._host_tab, _bwt.bank(o, "qr", "synthesis")._host_tab)
    n = 9
    x = np.arange(n)
    for mode, want in (("zero", None), ("constant", 8), ("reflect", 7), ("periodic", 0), ("symmetric", 8)):
        src = _bwt.virtual_source(n, _engine.MODE_IDS[mode])
        assert (None if src < 0 else x[src]) == want
        pt = {"zero": "constant", "constant": "replicate", "reflect": "reflect", "periodic": "circular"}.get(mode)
        if pt is not None:
            ref = torch.nn.functional.pad(torch.arange(n, dtype=torch.float64).reshape(1, 1, n), (0, 1), mode=pt)[0, 0, -1]
            assert float(ref) == (0.0 if src < 0 else float(x[src]))
    assert _bwt.is_short([12], 8) and not _bwt.is_short([13], 8) and not _bwt.is_short([14], 8) and _bwt.is_short([64, 11], 8)


# ---- the float64 operators as the reference of the GPU kernel tests: pinned to the reference library at L = 10 .. 18 and mid sizes --------
MID = "ptwt_ref_boundary_mid.npz"
MID_WAVELETS = ("db5", "db6", "db7", "db9", "sym7", "coif3", "bior4.4")


def test_tables_match_the_reference_blocks_at_the_lengths_the_first_fixture_misses():
    """L = 10, 12, 14 and 18 (db5, db6, db7 / sym7, db9 / coif3) and the biorthogonal bior4.4, gramschmidt: exact in sign, 1e-12 on
    entries."""
    z, idx = G.load(MID)
    blocks = [c for c in idx if c["group"] == "blocks"]
    assert tuple(c["wavelet"] for c in blocks) == MID_WAVELETS and {c["filt_len"] for c in blocks} == {10, 12, 14, 18}
    for case in blocks:
        taps = host_taps(case["wavelet"])
        assert len(taps[0]) == case["filt_len"]
        nt, nb = _boundary.boundary_rows(case["filt_len"])
        for which in ("analysis", "synthesis"):
            got = _boundary.boundary_blocks(taps, "gramschmidt", which)
            for band in ("lo", "hi"):
                for end, rows in (("top", nt), ("bot", nb)):
                    want = z["%s_%s_%s_%s" % (case["key"], which, band, end)]
                    mine = got["%s_%s" % (band, end)]
                    assert mine.shape == want.shape == (rows, case["filt_len"] - 1)
                    assert np.abs(mine - want).max(initial=0.0) < 1e-12, (case, which, band, end)


def _flat_golden(z, case, stem):
    return [torch.from_numpy(z["%s_%s%d" % (case["key"], stem, i)]) for i in range(case["ncoef"])]


def test_level_operators_reproduce_the_reference_at_mid_sizes():
    """``level_coo`` / ``level_matrix`` applied in float64 on the CPU (tests/_boundary_ref.py: sparse for rows, dense for planes, the
    virtual sample of an odd extent by mode) against the reference's classes at 2110 and 4101 samples and planes of 70 x 150 and
    67 x 133, L = 8, 14 and 18, every non-zero ``odd_coeff_padding_mode``: coefficients and reconstruction to 1e-12 (a comparison with
    the live reference at (2, 2110) and (1, 70, 150) showed 2e-14 at worst), the recorded gradients to 1e-11."""
    from tests import _boundary_ref as BR

    z, idx = G.load(MID)
    cases = [c for c in idx if c["group"] == "gs"]
    assert {(c["ndim"], c["filt_len"]) for c in cases} >= {(1, 8), (1, 14), (1, 18), (2, 8), (2, 18)}
    assert {c["kw"].get("odd_coeff_padding_mode", "zero") for c in cases if c["padded"]} == set(BR.MODES)
    assert {c["ndim"] for c in cases if c["grads"]} == {1, 2}
    weight = lambda t, i: torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64) + i).reshape(t.shape)  # noqa: E731
    for case in cases:
        taps = host_taps(case["wavelet"])
        mode = case["kw"].get("odd_coeff_padding_mode", "zero")
        x = torch.from_numpy(z[case["key"] + "_x"]).double().requires_grad_(True)
        assert list(x.shape) == case["shape"]
        c = BR.wavedec(x, taps, case["level"], mode)
        want = _flat_golden(z, case, "c")
        assert len(c) == len(want) == case["ncoef"]
        for i, (a, b) in enumerate(zip(c, want)):
            assert G.relerr(a.detach().numpy(), b.numpy()) < 1e-12, (case, "coefficient", i)
        leaves = [t.clone().requires_grad_(True) for t in want]
        y = BR.waverec(leaves, taps, case["ndim"])
        assert G.relerr(y.detach().numpy(), z[case["key"] + "_rec"]) < 1e-12, (case, "reconstruction")
        if case["grads"]:
            (gx,) = torch.autograd.grad(sum((weight(t, i) * t).sum() for i, t in enumerate(c)), x)
            assert G.relerr(gx.numpy(), z[case["key"] + "_gx"]) < 1e-11, (case, "analysis backward")
            gl = torch.autograd.grad((weight(y, 7) * y).sum(), leaves)
            for i, g in enumerate(gl):
                assert G.relerr(g.numpy(), z["%s_gc%d" % (case["key"], i)]) < 1e-11, (case, "synthesis backward", i)


@pytest.mark.parametrize("flen", list(range(2, 22, 2)) + [22, 34, 76, 128])
def test_level_coo_and_level_matrix_agree_entry_for_entry(flen):
    """One even length per L, four independent random filters (``_boundary`` accepts any taps), both directions: the sparse triplets
    are the dense matrix, entry for entry and without duplicates."""
    g = np.random.default_rng(flen)
    taps = tuple(tuple(float(v) for v in g.standard_normal(flen) / np.sqrt(flen)) for _ in range(4))
    n = 2 * (flen - 1) + 2 * (flen % 7) + 6
    for which in ("analysis", "synthesis"):
        dense = _boundary.level_matrix(taps, n, "qr", which)
        r, c, v = _boundary.level_coo(taps, n, "qr", which)
        assert len(set(zip(r.tolist(), c.tolist()))) == len(r)
        sparse = np.zeros((n, n))
        sparse[r, c] = v
        assert np.array_equal(sparse, dense), (flen, which)
        assert np.count_nonzero(dense) <= len(v)
    # the rows of the synthesis bank are built from the reversed rec_* filters, not from the dec_* ones
    assert not np.array_equal(_boundary.level_matrix(taps, n, "qr", "synthesis").T, _boundary.level_matrix(taps, n, "qr", "analysis"))


def test_tile_table_of_the_gpu_kernel_tests_is_the_geometry_of_the_source():
    """tests/test_gpu_boundary_kernels.py places its extents around the tile widths; the table it states is read against
    ``FwdTile`` / ``InvTile`` of csrc/mifwt_bwt.hip here, so that a change of the geometry cannot leave the cells behind."""
    import os
    import re

    from tests import test_gpu_boundary_kernels as K

    with open(os.path.join(os.path.dirname(_bwt.__file__), "csrc", "mifwt_bwt.hip")) as f:
        src = f.read()

    def const(name):
        (expr,) = re.findall(r"static constexpr int %s = ([^;]+);" % name, src)
        return expr.strip()

    with open(os.path.join(os.path.dirname(_bwt.__file__), "csrc", "mifwt_level_tile.h")) as f:
        shared = f.read()  # (the vector type is shared by every fused-level unit; the row bank takes it from there)
    assert re.search(r"struct Vec16<float> \{\s*static constexpr int E = 4;", shared) and re.search(r"struct Vec16<double> \{\s*static constexpr int E = 2;", shared)
    with open(os.path.join(os.path.dirname(_bwt.__file__), "csrc", "mifwt_bwt_rows.h")) as f:
        assert '#include "mifwt_level_tile.h"' in f.read()
    assert K.E == {torch.float32: 4, torch.float64: 2}
    assert (const("TC1"), const("TC"), const("TR")) == ("256 * E", "16 * E", "8")
    assert (const("TQ1"), const("TQ"), const("TQC")) == ("128 * E", "16", "(L <= 12 ? 16 : 8) * E")
    for dtype, e in K.E.items():
        assert K.TILE1[("fwd", dtype)] == 256 * e and K.TILE1[("inv", dtype)] == 128 * e
        for flen in K.FUSED:
            assert K.tile2("fwd", dtype, flen) == (8, 16 * e) and K.tile2("inv", dtype, flen) == (16, (16 if flen <= 12 else 8) * e)
    # (the axis launcher is shared and takes the family's grid cap: at most `grid_cap` workgroups of 256)
    assert "g((unsigned)(blocks < grid_cap ? blocks : grid_cap)), blk(256)" in shared
    assert "launch_axis(dtype, inverse, total, 8192, stream, a, bwt_axis_generic<" in src and K.GENERIC_GRID == 8192 * 256
    # (one length dispatch for every fused-level unit: the even lengths 2 .. 20 and no other)
    assert K.FUSED == list(range(2, 21, 2)) and re.findall(r"MIFWT_LEN_CASE\((\d+)\)\n", shared) == [str(flen) for flen in K.FUSED]
    assert "for_even_len(d->filt_len," in src and "launch_fused<T, decltype(len)::value>" in src
