"""bfloat16 storage, host side (no GPU): the scope, the dtype id, the routes, the refusals and the element-wise bound helpers.

bfloat16 is the second 16-bit storage type (f32 arithmetic) and follows float16 route by route: the same kernel id for every
descriptor, the same refusal (exception type and message) wherever float16 is refused.  The bf16 bound helpers of
``tests/_bf16_ref.py`` are checked like those of ``tests/_probe_ref.py``: they hold for an honest emulation at every element and are
violated by a truncating store and by tap pairs without their low halves.
"""
import ctypes
import itertools
import threading

import numpy as np
import pytest
import torch

import ptwt_amd
from oracle import fwt_oracle as O
from ptwt_amd import _engine, _ext, _per, _bwt, constants as C, packets
from tests import _bf16_ref as B
from tests import _boundary_ref as BR
from tests import _probe_ref as R

BF16, F16 = torch.bfloat16, torch.float16


# ---- the scope ---------------------------------------------------------------------------------------------------------------
def test_bfloat16_is_supported_inside_the_half_storage_scope_only():
    assert BF16 not in C.supported_dtypes() and F16 not in C.supported_dtypes()
    seen = {}
    with C.half_storage():
        assert BF16 in C.supported_dtypes() and F16 in C.supported_dtypes()
        t = threading.Thread(target=lambda: seen.setdefault("other", BF16 in C.supported_dtypes()))
        t.start()
        t.join()
        with C.half_storage(False):
            assert BF16 not in C.supported_dtypes()
        assert BF16 in C.supported_dtypes()
    assert seen["other"] is False  # the scope is local to the thread
    assert BF16 not in C.supported_dtypes()
    C.set_half_storage(True)
    try:
        assert BF16 in C.supported_dtypes() and F16 in C.supported_dtypes()
        with C.half_storage(False):
            assert BF16 not in C.supported_dtypes()
    finally:
        C.set_half_storage(False)
    assert C.supported_dtypes() == {torch.float32, torch.float64}


def test_outside_the_scope_bfloat16_is_refused_like_float16():
    x = torch.zeros(2, 16, 16)
    for dt in (F16, BF16):
        with pytest.raises(ValueError, match="Input dtype %s not supported" % str(dt).replace(".", r"\.")):
            ptwt_amd.wavedec2(x.to(dt), "haar")


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_dtype_id_and_header():
    assert _engine._DTYPE_IDS[BF16] == 3 and _engine._DTYPE_IDS[F16] == 2
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mifwt.h")).read()
    assert "MIFWT_BF16 = 3" in header and "#define MIFWT_ABI_VERSION 3" in header
    assert _engine.load_library().mifwt_abi_version() == 3


_LENGTHS = (2, 8, 16, 18, 20, 24, 28, 32, 40)
_MODES = ("zero", "constant", "reflect", "periodic", "symmetric")
# extents per ndim: below and above the matrix-core synthesis threshold (four 32 x 128 tiles per image), odd and even
_EXTENTS = {1: ((81,), (1001,)), 2: ((81, 90), (300, 402), (512, 512)), 3: ((81, 82, 83), (90, 100, 128))}


def test_kernel_id_answers_for_bfloat16_what_it_answers_for_float16():
    """Every descriptor of the grid, both directions: the same kernel id, never BADARG.  Ids 0, 3, 4, 7, 8, 11 and 23 all occur; 5 and 6
    (planes + depth pass) serve float32 / float64 volumes only and occur for neither 16-bit type."""
    seen = set()
    for ndim, flen, mode, direction in itertools.product((1, 2, 3), _LENGTHS, _MODES, (0, 1)):
        for ext in _EXTENTS[ndim]:
            if min(ext) < flen:
                continue
            for batch in (1, 4):
                want = _engine.kernel_id(ndim, F16, mode, flen, batch, ext, direction)
                got = _engine.kernel_id(ndim, BF16, mode, flen, batch, ext, direction)
                assert got == want and got >= 0, (ndim, flen, mode, direction, ext, batch, got, want)
                seen.add(got)
    assert seen == {0, 3, 4, 7, 8, 11, 23}, seen
    for opt7 in (2, 4):  # the vector tile kernel forced / the matrix cores forced
        _engine.set_option(7, opt7)
        try:
            for flen, direction, ext in itertools.product((18, 32), (0, 1), _EXTENTS[2]):
                assert _engine.kernel_id(2, BF16, "reflect", flen, 2, ext, direction) == _engine.kernel_id(2, F16, "reflect", flen, 2, ext, direction)
        finally:
            _engine.set_option(7, 0)


def test_adjoint_routes_and_workspace_follow_float16():
    lib = _engine.load_library()
    lib.mifwt_workspace_bytes.restype = ctypes.c_size_t
    for ndim, flen, direction in itertools.product((1, 2, 3), (8, 20, 28), (0, 1, 2, 3)):
        ext = _EXTENTS[ndim][-1]
        coef = [(n + flen - 1) // 2 for n in ext]
        planes = _engine._plane_strides((2, 1 << ndim, *coef))[0]
        ds = [_engine._desc(ndim, dt, _engine.MODE_IDS["symmetric"], flen, 2, ext, _engine._dense_strides(ext), coef, planes, planes) for dt in (F16, BF16)]
        kids = [lib.mifwt_kernel_id(ctypes.byref(d), direction) for d in ds]
        assert kids[0] == kids[1] and kids[1] >= 0, (ndim, flen, direction, kids)
        ws = [lib.mifwt_workspace_bytes(ctypes.byref(d), direction) for d in ds]
        assert ws[0] == ws[1], (ndim, flen, direction, ws)


def _desc(dtype_id, flen, sig, coef):
    nd = len(sig)
    ss, cs = [1], [1]
    for n, m in zip(reversed(sig), reversed(coef)):
        ss.insert(0, ss[0] * n)
        cs.insert(0, cs[0] * m)
    d = _engine.LevelDesc()
    d.ndim, d.dtype, d.mode, d.filt_len, d.batch = nd, dtype_id, 0, flen, 1
    for a in range(nd):
        d.sig_extent[a], d.coef_extent[a] = sig[a], coef[a]
    for a in range(nd + 1):
        d.sig_stride[a], d.approx_stride[a], d.detail_stride[a] = ss[a], cs[a], cs[a]
    return d


def test_unsupported_not_badarg_where_float16_is_unsupported():
    """The periodized, value-map and boundary-wavelet entry points answer dtype 3 as they answer dtype 2 (a valid request without a
    kernel: 0 from the queries, MIFWT_ERR_UNSUPPORTED = -2 from the calls); dtype 7 stays MIFWT_ERR_BADARG = -1."""
    per, ext = _per._lib(), _ext._lib()
    for direction in (0, 1):
        for dt in (2, 3):
            d = _desc(dt, 8, [16, 16], [8, 8])
            assert (per.mifwt_per_supported(ctypes.byref(d), direction), per.mifwt_per_kernel_id(ctypes.byref(d), direction)) == (0, -2)
            d = _desc(dt, 8, [16, 16], [11, 11])
            assert (ext.mifwt_ext_supported(ctypes.byref(d), 0, direction), ext.mifwt_ext_kernel_id(ctypes.byref(d), 0, direction)) == (0, -2)
        assert per.mifwt_per_supported(ctypes.byref(_desc(7, 8, [16, 16], [8, 8])), direction) == -1
        assert ext.mifwt_ext_supported(ctypes.byref(_desc(7, 8, [16, 16], [11, 11])), 0, direction) == -1
    lib = _engine.load_library()
    d7 = _desc(7, 8, [16, 16], [11, 11])
    assert lib.mifwt_kernel_id(ctypes.byref(d7), 0) == -1
    # the single-axis and subtree entries take the dtype as an argument: null pointers are never dereferenced, the dtype check comes first
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    taps = (ctypes.c_double * 8)()
    st = (ctypes.c_int64 * 3)(16, 1, 1)
    for dt, want in ((2, -2), (3, -2), (7, -1)):
        assert per.mifwt_per_axis_fwd(dt, 8, 1, 16, 1, p, st, p, st, p, st, taps, taps, None) == want
        assert ext.mifwt_ext_axis_fwd(0, dt, 8, 1, 16, 1, p, st, p, st, p, st, taps, taps, None) == want
    blib = _bwt._lib()
    assert blib.mifwt_bwt_tree_levels(3, 4, 64, 3) == blib.mifwt_bwt_tree_levels(2, 4, 64, 3) == 0
    for fn in (blib.mifwt_bwt_supported, blib.mifwt_bwt3_supported):
        nd = 2 if fn is blib.mifwt_bwt_supported else 3
        answers = [fn(ctypes.byref(_desc(dt, 4, [16] * nd, [8] * nd)), 0) for dt in (2, 3, 7)]
        assert answers[0] == answers[1] == 0 and answers[2] == -1, answers


# ---- refusals: wherever float16 is refused, bfloat16 is refused the same way ----------------------------------------------------
def _refusal(call):
    with pytest.raises(Exception) as e:
        call()
    return type(e.value), str(e.value)


def _same_refusal(make):
    """make(dtype) -> a call; inside the scope both 16-bit types must raise the same exception type with the same message (up to the
    dtype's own name)."""
    with ptwt_amd.half_storage():
        t16, m16 = _refusal(make(F16))
        tb, mb = _refusal(make(BF16))
    assert t16 is tb and t16 in (ValueError, NotImplementedError), (t16, tb)
    assert mb.replace("torch.bfloat16", "torch.float16") == m16 and "not supported" in mb, (m16, mb)


@pytest.mark.parametrize("mode", ["periodization", "smooth", "antisymmetric", "antireflect"])
def test_periodized_and_value_map_modes_refuse_bfloat16(mode):
    x = torch.randn(2, 16, 16)
    _same_refusal(lambda dt: (lambda: ptwt_amd.wavedec2(x.to(dt), "db2", mode=mode)))
    _same_refusal(lambda dt: (lambda: ptwt_amd.wavedec(x.to(dt), "db2", mode=mode)))
    if mode == "periodization":
        _same_refusal(lambda dt: (lambda: ptwt_amd.fswaverec2((x.to(dt), {k: x.to(dt) for k in ("ad", "da", "dd")}), "db2", mode=mode)))


def test_stationary_2d_3d_refuse_bfloat16():
    x = torch.zeros(2, 8, 8)
    v = torch.zeros(2, 8, 8, 8)
    _same_refusal(lambda dt: (lambda: ptwt_amd.swt2(x.to(dt), "haar", level=1)))
    _same_refusal(lambda dt: (lambda: ptwt_amd.iswt2([x.to(dt), (x.to(dt),) * 3], "haar")))
    _same_refusal(lambda dt: (lambda: ptwt_amd.swt3(v.to(dt), "haar", level=1)))


def test_boundary_wavelet_transforms_refuse_bfloat16(monkeypatch):
    """The Matrix* transforms check the device before the dtype, so their public refusal is a GPU test (tests/test_gpu_bf16.py); the
    refusal itself — the one place every boundary-wavelet level passes before its first launch — and the packets' are checked here."""
    _same_refusal(lambda dt: (lambda: _bwt._composed_setup(torch.zeros(2, 64).to(dt), 1)))
    monkeypatch.setattr(packets, "_boundary_on_device", lambda t: True)  # (the device check of the packets comes first as well)
    monkeypatch.setattr(packets, "_boundary_rows", lambda x, bk, mode_id: BR.rows_level(x, bk.taps, bk.which, "zero"))
    _same_refusal(lambda dt: (lambda: ptwt_amd.WaveletPacket(torch.randn(2, 64).to(dt), "db2", mode="boundary")))


# ---- the bf16 bound helpers ----------------------------------------------------------------------------------------------------
def test_half_spacing_bf16_bounds_every_rounding():
    rng = np.random.default_rng(1)
    v = np.concatenate([np.exp(rng.uniform(np.log(1e-30), np.log(1e30), 4000)), [0.0, 1.0, 1.0 - 2.0 ** -9, 131072.0, 255.0, 255.5, 2.0 ** -20]])
    x = torch.from_numpy(v)
    up = B.bf16_up(x)
    assert torch.all(up >= x) and torch.all(up.float().to(BF16).double() == up)       # a bf16 value, not below
    assert torch.all((up - x) <= 2 * B.half_spacing_bf16(x))                           # ... and the nearest such
    hs = B.half_spacing_bf16(x)
    assert hs[4000] == 0 and B.half_spacing_bf16(torch.tensor([1.0, 1.5, 131072.0], dtype=torch.float64)).tolist() == [2.0 ** -8, 2.0 ** -8, 2.0 ** 9]
    assert torch.all((x.float().to(BF16).double() - x.float().double()).abs() <= hs)  # round to nearest stays inside
    assert torch.all(hs <= B.UBF16 * up)                                               # unit roundoff 2^-8
    both = torch.cat([x, -x]).float().double()
    t = B.trunc_bf16(both)
    assert torch.all(t.abs() <= both.abs()) and torch.all((t - both).abs() < 2 * B.half_spacing_bf16(both.abs()) + 1e-300)
    assert torch.any((t - both).abs() > B.half_spacing_bf16(both.abs()))              # truncation is what rounding is not


@pytest.mark.parametrize("wavelet", ["db9", "db10", "db12", "db14", "sym16"])
def test_bf16_tap_pair_residual_is_relative_2_pow_minus_16(wavelet):
    """|t - t_hi - t_lo| <= 2^-16 |t| (+ the float cast) for every tap of the long banks — 1/256 of the output's unit roundoff, which is
    why two parts suffice — and a single part is off by up to 2^-8 |t|."""
    for t in O.filter_bank(wavelet):
        th, tl = B.pair_bf16(t)
        err = np.abs(t - (th + tl))
        assert np.all(err <= B.pair_bf16_err(t)) and np.all(B.pair_bf16_err(t) <= (2.0 ** -16 + 2.0 ** -23) * np.abs(t))
        assert np.all(np.abs(t - th) <= 2.0 ** -8 * np.abs(t) * (1 + 2.0 ** -20))
        assert np.max(np.abs(t - th) / np.abs(t)) > 2.0 ** -11  # one part alone is no better than bf16 itself


CASES = B.cases()


def _judge(job, got, st):
    ratio, idx, nbad = R.worst(got, st)
    return ratio, nbad, job.where(idx, st.want.shape)


@pytest.mark.parametrize("case", CASES, ids=R.case_ids(CASES))
def test_bound_holds_for_impulses_and_sees_the_mutations(case):
    """Isolated impulses (the thinned one-impulse-per-image plane and the diagonal lattice shifts of the seam planes, as in
    tests/test_probe_host.py): the honest torch emulation — intermediate and output rounded with ``.to(torch.bfloat16)`` — is inside the
    bound at every element; a store that truncates is not, nor is a matrix-core pass without the low halves of its tap pairs."""
    for mode in case.modes[:3]:
        batch = R.jobs(case, mode, thin=True)
        for job in (batch[0], batch[-1]):
            st = B.bound(job, job.x)
            ratio, nbad, where = _judge(job, B.emulate(job, job.x), st)
            assert nbad == 0 and ratio <= 1.0, (where, ratio, nbad)
            ratio, nbad, _ = _judge(job, B.emulate(job, job.x, trunc=True), st)
            assert nbad > 0 and ratio > 1.0, (case.id, mode, job.label, "truncating store", ratio)
            ratio, nbad, _ = _judge(job, B.emulate(job, job.x, drop=R.smallest_taps(job.op_c)), st)
            assert nbad > 0 and ratio > 1.0, (case.id, mode, job.label, "dropped end tap", ratio)
            if case.arith.taps == "pairbf16":
                ratio, nbad, _ = _judge(job, B.emulate(job, job.x, flush_lo=True), st)
                assert nbad > 0 and ratio > 1.0, (case.id, mode, job.label, "t_lo dropped", ratio)


@pytest.mark.parametrize("family", ["mfma_fwd", "mfma_inv", "tile_fwd", "axis_fwd"])
def test_bound_holds_for_random_data_and_sees_the_mutations(family):
    """Random bf16 data on a ragged plane / an odd length: the bound holds for the honest emulation; the truncating store and (matrix
    cores) the dropped low halves violate it there too."""
    case = next(c for c in CASES if c.family == family and c.wavelet == "sym16")
    L = case.flen
    g = torch.Generator().manual_seed(5)
    if case.ndim == 1:
        x = torch.randn(64, 301, generator=g).to(BF16).double()
        job = R.Job(case, "symmetric", "random", x, R.fwd_op(case.wavelet, 301, "symmetric"))
    elif case.direction == 0:
        h, w = 2 * L + 3, 3 * L + 6
        x = torch.randn(8, h, w, generator=g).to(BF16).double()
        job = R.Job(case, "reflect", "random", x, R.fwd_op(case.wavelet, w, "reflect"), R.fwd_op(case.wavelet, h, "reflect"))
    else:
        mh, mw = L + 5, L + 12
        x = torch.randn(8, 2 * mh, 2 * mw, generator=g).to(BF16).double()
        job = R.Job(case, "reflect", "random", x, R.inv_op(case.wavelet, mw, 1), R.inv_op(case.wavelet, mh, 0))
    st = B.bound(job, job.x)
    ratio, nbad, where = _judge(job, B.emulate(job, job.x), st)
    assert nbad == 0 and ratio <= 1.0, (where, ratio, nbad)
    ratio, nbad, _ = _judge(job, B.emulate(job, job.x, trunc=True), st)
    assert nbad > 0 and ratio > 1.0, (family, "truncating store", ratio)
    if case.arith.taps == "pairbf16":
        ratio_lo, nbad, _ = _judge(job, B.emulate(job, job.x, flush_lo=True), st)
        assert nbad > 0 and ratio_lo > 1.0, (family, "t_lo dropped", ratio_lo)
