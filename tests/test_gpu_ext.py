"""GPU tests (``-m gpu``) of the value-map extension levels (csrc/mifwt_ext.hip, kernel ids 42 .. 45) and of ``mode="smooth"``,
``"antisymmetric"`` and ``"antireflect"`` of the public transforms, against the float64 torch reference tests/_ext_ref.py (which
tests/test_ext_host.py pins to the oracle in the five old modes and to ``numpy.pad`` in the three new ones).

1. Single levels and their adjoints through ``_ext.level_fwd`` / ``level_adj``, every mode and both dtypes, on the fused route and again
   under ``FORCE_AXIS``: rows of 1, 2, 3, 5, 8, 13, 33, 127, 128, 129, 131 and 1031 samples (batch 3: the N = 1 and N = 2 rules, several
   wraps under db10, the 128-sample edge of the float32 tile, unaligned rows), planes 1x7, 2x2, 5x7, 13x10, 33x65, 34x130 and 67x131 as
   a slice of a wider tensor with an odd row pitch, volumes 5x6x7 and 9x8x12; haar, db2, db4, bior3.5, db10 and one random 24-tap bank
   (axis route only).  ``mifwt_launch_count`` must show the intended ids per cell.
2. Whole calls: ``wavedec`` / ``wavedec2`` / ``wavedec3`` at levels 1 to 3, ``fswavedec2``, a permuted-axes call, packet trees of depth
   2 in 1-D and 2-D; ``waverec*`` of the result against the reference's round trip.
3. A linear ramp along each axis, float64: every detail band of "smooth" and "antireflect" under db2 and db4 is zero to 1e-12 of the
   input's norm, boundary coefficients included, where "symmetric" has details above 1e-3 of it.
4. Data gradients against float64 autograd through the reference with Gaussian cotangents; second order under ``create_graph=True``.
5. Entry by entry: unit impulses through the level and through its adjoint at N = 13 and 16 under db4: the two matrices are transposes
   of each other and equal the reference operator.
6. ``ptwt_amd.capture`` replays to the same bits; guard regions around every output of ids 42 .. 45 stay intact.

Bounds, norm-wise per tensor (``_ext_ref.relerr``): float64 1e-12 (values) / 1e-10 (gradients).  float32 values: max(1e-6, 10 x
e_ref32(cell)), e_ref32 = the error of the REFERENCE's float32 run against its own float64 run on the same inputs, per cell (the
extension weights grow with the pad, so the bound comes from the cell).  Only a band that is zero in exact arithmetic (below
``ZERO_BAND`` of the input's norm) is measured relative to the norm of the transform's input.  float32 gradients: ``python -m
tests.test_gpu_ext`` runs the reference in float32 on the host over GRAD_CASES x modes x GRAD_WAVELETS and prints its worst norm-wise
gradient error against its float64 run: 1.32e-6 (d wavedec3 / d x of 1x9x8x12 under db4, "smooth": the extrapolated samples of short
axes are large; 1.8e-7 and below in the other two modes); the bound is ten times that, F32_GRAD_TOL = 1.3e-5.

On the MI355X (52 cases, 7 s): float64 values at 2.5e-13 and below, float64 gradients at 2.3e-14 and below, float32 data gradients at
1.0e-6; the float32 check closest to its bound is at 0.68 of it (the "smooth" diagonal band of the 5x7 plane under db4, zero in exact
arithmetic: 4.4e-6 of the input's norm against 6.4e-6), the fused adjoint at 0.45 of its bound and below.
"""
import ctypes

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, _ext
from ptwt_amd._wavelets import host_taps
from tests import _ext_ref as R

pytestmark = pytest.mark.gpu

F64_TOL, F64_GRAD_TOL = 1e-12, 1e-10
F32_GRAD_TOL = 1.3e-5  # 10 x the float32 reference's own worst gradient error over the gradient cases (module docstring)
MODES = R.NEW_MODES
DTYPES = (torch.float32, torch.float64)
ROWS = [1, 2, 3, 5, 8, 13, 33, 127, 128, 129, 131, 1031]
PLANES = [(1, 7), (2, 2), (5, 7), (13, 10), (33, 65), (34, 130), (67, 131)]
VOLUMES = [(5, 6, 7), (9, 8, 12)]
WAVELETS = ("haar", "db2", "db4", "bior3.5", "db10")
KIDS = (42, 43, 44, 45)
WORST = {}
_REFS = {}


def dev():
    return torch.device("cuda:0")


def _name(dtype):
    return str(dtype).split(".")[-1]


def _bank24():
    g = np.random.default_rng(24)
    return tuple(tuple(float(np.float32(v)) for v in g.standard_normal(24) / np.sqrt(24)) for _ in range(4))


def _bank(wavelet):
    return _bank24() if wavelet == "rand24" else host_taps(wavelet)


def _counts():
    return [_engine.launch_count(k) for k in KIDS]


def _delta(before):
    return [a - b for a, b in zip(_counts(), before)]


def _check(got, want, tol, what, key=None, scale=0.0):
    err = R.relerr(got, want, scale)
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    if key is not None:
        WORST[key] = max(WORST.get(key, 0.0), err)
    print("%s: %.3e (bound %.1e)" % (what, err, tol))
    assert err < tol, (what, err, tol)
    return err


def _tol(dtype, e32):
    return F64_TOL if dtype == torch.float64 else max(1e-6, 10 * e32)


def _gauss(shape, seed):
    """Gaussian float64 values that float32 holds exactly: one draw serves both dtypes."""
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64).float().double()


def _cell(mode, wavelet, shape):
    """The float64 reference of one cell, computed once and shared: inputs, the level, its adjoint, the reference's float32 errors."""
    key = (mode, wavelet, shape)
    if key not in _REFS:
        bank, ndim = _bank(wavelet), len(shape) - 1
        flen = len(bank[0])
        x = _gauss(shape, 11 * sum(shape) + flen)
        coef = tuple((n + flen - 1) // 2 for n in shape[1:])
        g = _gauss((shape[0], 1 << ndim, *coef), 13 * sum(shape) + flen)
        fwd = lambda t: R.level_fwd(t, bank, mode, ndim)  # noqa: E731
        adj = lambda t: R.level_adj(list(t.unbind(1)), bank, mode, ndim, shape[1:])  # noqa: E731
        _REFS[key] = {"x": x, "g": g, "fwd": fwd(x), "adj": adj(g), "e_fwd": R.e_ref32(fwd, x, scale=float(x.norm())),
                      "e_adj": R.e_ref32(adj, g, scale=float(g.norm()))}
    return _REFS[key]


def _on_device(t, dtype, pitched=False):
    t = t.to(dtype)
    if pitched:  # a slice of a wider tensor with an odd row pitch
        wide = torch.zeros(*t.shape[:-1], t.shape[-1] + 5 - t.shape[-1] % 2, dtype=dtype)
        wide[..., :t.shape[-1]] = t
        assert wide.stride(-2) % 2 == 1
        return wide.to(dev())[..., :t.shape[-1]]
    return t.to(dev())


# ---- 1. single levels ------------------------------------------------------------------------------------------------------------------
def _run_cell(mode, dtype, wavelet, shape, route):
    ref = _cell(mode, wavelet, shape)
    bank, ndim = _bank(wavelet), len(shape) - 1
    pitched = shape[1:] == (67, 131)
    x = _on_device(ref["x"], dtype, pitched)
    g = _on_device(ref["g"], dtype, pitched)
    fused = route == "fused"
    what = (mode, _name(dtype), wavelet, shape, route)
    _ext.FORCE_AXIS = not fused
    try:
        before = _counts()
        buf = _ext.level_fwd(x, bank[0], bank[1], mode)
        d_fwd = _delta(before)
        before = _counts()
        gx = _ext.level_adj(g, bank[0], bank[1], mode, shape[1:])
        d_adj = _delta(before)
    finally:
        _ext.FORCE_AXIS = False
    passes = (1 << ndim) - 1
    if fused and len(bank[0]) <= 20:
        assert (d_fwd, d_adj) == ([1, 0, ndim == 3, 0], [0, 1, 0, ndim == 3]), (what, d_fwd, d_adj)
    else:
        assert (d_fwd, d_adj) == ([0, 0, passes, 0], [0, 0, 0, passes]), (what, d_fwd, d_adj)
    assert buf.dtype == dtype and gx.dtype == dtype
    scale = float(ref["x"].norm())
    for s, want in enumerate(ref["fwd"]):
        _check(buf[:, s], want, _tol(dtype, ref["e_fwd"]), what + ("band", s), "level %s %s" % (route, _name(dtype)), scale)
    _check(gx, ref["adj"], _tol(dtype, ref["e_adj"]), what + ("adjoint",), "adjoint %s %s" % (route, _name(dtype)), float(ref["g"].norm()))


@pytest.mark.parametrize("route", ["fused", "axis"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("mode", MODES)
def test_single_levels(mode, dtype, route):
    for wavelet in WAVELETS + (("rand24",) if route == "fused" else ()):
        for shape in [(3, n) for n in ROWS] + [(2, *p) for p in PLANES] + [(2, *v) for v in VOLUMES]:
            _run_cell(mode, dtype, wavelet, shape, route)


# ---- 2. whole calls ----------------------------------------------------------------------------------------------------------------------
_DEC = {1: (ptwt_amd.wavedec, ptwt_amd.waverec), 2: (ptwt_amd.wavedec2, ptwt_amd.waverec2), 3: (ptwt_amd.wavedec3, ptwt_amd.waverec3)}
API_CASES = [((3, 131), 1, "db4"), ((2, 33, 65), 2, "db4"), ((2, 13, 10), 2, "bior3.5"), ((1, 9, 8, 12), 3, "db2")]


def _api_to_ref(coeffs, ndim):
    out = [coeffs[0]]
    for c in coeffs[1:]:
        if ndim == 1:
            out.append([c])
        elif ndim == 2:
            out.append([c[1], c[0], c[2]])  # (H, V, D) = bands 2, 1, 3
        else:
            out.append([c[format(s, "03b").replace("0", "a").replace("1", "d")] for s in range(1, 8)])
    return out


def _flat(ref_coeffs):
    return [ref_coeffs[0]] + [t for det in ref_coeffs[1:] for t in det]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("mode", MODES)
def test_whole_calls_and_round_trip(mode, dtype):
    for shape, ndim, wavelet in API_CASES:
        bank = host_taps(wavelet)
        x64 = _gauss(shape, sum(shape))
        scale = float(x64.norm())
        dec, rec = _DEC[ndim]
        for level in (1, 2, 3):
            want = R.wavedecn(x64, bank, mode, ndim, level)
            e32 = R.e_ref32(lambda t: _flat(R.wavedecn(t, bank, mode, ndim, level)), x64, scale=scale)
            before = _counts()
            coeffs = dec(x64.to(dtype).to(dev()), wavelet, mode=mode, level=level)
            assert _delta(before) == [level, 0, level * (ndim == 3), 0]
            what = (mode, _name(dtype), shape, wavelet, level)
            for i, (a, b) in enumerate(zip(_flat(_api_to_ref(coeffs, ndim)), _flat(want))):
                _check(a, b, _tol(dtype, e32), what + ("coefficient", i), "api values %s" % _name(dtype), scale)
            want_rec = R.waverecn(want, bank, ndim)
            e32r = R.e_ref32(lambda t: R.waverecn(R.wavedecn(t, bank, mode, ndim, level), bank, ndim), x64)
            y = rec(coeffs, wavelet, mode=mode)
            _check(y, want_rec, _tol(dtype, e32r), what + ("round trip",), "api round trip %s" % _name(dtype))


@pytest.mark.parametrize("mode", MODES)
def test_separable_permuted_and_packets(mode):
    dtype = torch.float64
    bank = host_taps("db2")
    x64 = _gauss((2, 13, 10), 5)
    x = x64.to(dev())
    want = R.wavedecn(x64, bank, mode, 2, 2)
    # fswavedec2: the same bands by key
    fs = ptwt_amd.fswavedec2(x, "db2", mode=mode, level=2)
    _check(fs[0], want[0], F64_TOL, (mode, "fswavedec2 approximation"))
    for lvl, det in zip(fs[1:], want[1:]):
        for key, band in (("ad", 0), ("da", 1), ("dd", 2)):
            _check(lvl[key], det[band], F64_TOL, (mode, "fswavedec2", key))
    _check(ptwt_amd.fswaverec2(fs, "db2", mode=mode), R.waverecn(want, bank, 2), F64_TOL, (mode, "fswaverec2"))
    # permuted axes: the axis route
    xp = x64.permute(1, 2, 0).contiguous().to(dev())  # [13, 10, 2], transformed axes (0, 1)
    before = _counts()
    cp = ptwt_amd.wavedec2(xp, "db2", mode=mode, level=1, axes=(0, 1))
    assert _delta(before) == [0, 0, 3, 0]
    one = R.wavedecn(x64, bank, mode, 2, 1)
    for a, b in zip(_flat(_api_to_ref(cp, 2)), _flat(one)):
        _check(a.permute(2, 0, 1), b, F64_TOL, (mode, "permuted axes"))
    # packets of depth 2: every node is the reference applied recursively; both key maps in 2-D
    x1 = _gauss((2, 37), 6)
    wp = ptwt_amd.WaveletPacket(x1.to(dev()), "db2", mode=mode, maxlevel=2)
    for key in ("aa", "ad", "da", "dd"):
        node = x1
        for c in key:
            node = R.dwt_axis(node, bank[0], bank[1], mode, -1)[c == "d"]
        _check(wp[key], node, F64_TOL, (mode, "packet", key))
    for separable in (False, True):
        wp2 = ptwt_amd.WaveletPacket2D(x, "db2", mode=mode, maxlevel=2, separable=separable)
        band = {"a": 0, "h": 1, "v": 2, "d": 3} if separable else {"a": 0, "v": 1, "h": 2, "d": 3}  # (fswavedec2's "ad" is h there)
        for key in ("aa", "hv", "dd", "va"):
            node = x64
            for c in key:
                node = R.level_fwd(node, bank, mode, 2)[band[c]]
            _check(wp2[key], node, F64_TOL, (mode, "packet2d", separable, key))


# ---- 3. analytic checks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wavelet", ["db2", "db4"])
def test_linear_ramp_has_no_details(wavelet):
    """A polynomial of degree 1 is annihilated by a high-pass filter with two vanishing moments wherever the EXTENDED signal is that
    polynomial: "smooth" and "antireflect" continue a ramp as the ramp, so every detail coefficient vanishes, those at the boundary
    included; "symmetric" folds it back and leaves boundary details."""
    ramps = {1: torch.arange(131, dtype=torch.float64)[None].repeat(3, 1) * 0.25 - 3.0,
             2: (torch.arange(33, dtype=torch.float64)[:, None] * 0.5 - torch.arange(65, dtype=torch.float64)[None, :] * 0.125 + 2.0)[None],
             3: (torch.arange(9, dtype=torch.float64)[:, None, None] + 2.0 * torch.arange(8, dtype=torch.float64)[None, :, None]
                 - 0.5 * torch.arange(12, dtype=torch.float64)[None, None, :])[None]}
    for ndim, x64 in ramps.items():
        scale = float(x64.norm())
        for mode in ("smooth", "antireflect", "symmetric"):
            coeffs = _api_to_ref(_DEC[ndim][0](x64.to(dev()), wavelet, mode=mode, level=2), ndim)
            worst = max(float(t.norm()) for det in coeffs[1:] for t in det) / scale
            print(wavelet, ndim, mode, "largest detail band / input norm: %.3e" % worst)
            if mode == "symmetric":
                assert worst > 1e-3
            else:
                assert worst < 1e-12, (wavelet, ndim, mode, worst)


# ---- 4. data gradients -------------------------------------------------------------------------------------------------------------------
GRAD_CASES = [((3, 13), 1), ((2, 5, 7), 2), ((2, 33, 65), 2), ((1, 9, 8, 12), 3)]
GRAD_WAVELETS = ("db2", "db4")
GRAD_LEVEL = 2


def _cotangents(tensors, seed):
    return [_gauss(t.shape, 2000 + 17 * seed + i) for i, t in enumerate(tensors)]


def _ref_grad(x64, bank, mode, ndim, dtype):
    x = x64.to(dtype).requires_grad_(True)
    flat = _flat(R.wavedecn(x, bank, mode, ndim, GRAD_LEVEL))
    ws = _cotangents(flat, sum(x64.shape))
    (g_x,) = torch.autograd.grad(sum((c * w.to(dtype)).sum() for c, w in zip(flat, ws)), x)
    return g_x, ws


@pytest.mark.parametrize("wavelet", GRAD_WAVELETS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("mode", MODES)
def test_data_gradients(mode, dtype, wavelet):
    bank = host_taps(wavelet)
    for shape, ndim in GRAD_CASES:
        x64 = _gauss(shape, sum(shape))
        want, ws = _ref_grad(x64, bank, mode, ndim, torch.float64)
        x = x64.to(dtype).to(dev()).requires_grad_(True)
        before = _counts()
        flat = _flat(_api_to_ref(_DEC[ndim][0](x, wavelet, mode=mode, level=GRAD_LEVEL), ndim))
        (g_x,) = torch.autograd.grad(sum((c * w.to(dtype).to(dev())).sum() for c, w in zip(flat, ws)), x)
        assert _delta(before) == [GRAD_LEVEL, GRAD_LEVEL, GRAD_LEVEL * (ndim == 3), GRAD_LEVEL * (ndim == 3)]
        _check(g_x, want, F64_GRAD_TOL if dtype == torch.float64 else F32_GRAD_TOL, (mode, _name(dtype), shape, wavelet, "d/dx"),
               "data gradients %s" % _name(dtype))


@pytest.mark.parametrize("mode", MODES)
def test_second_order_float64(mode):
    """The level is linear: the derivative of <A^T v, w2> w.r.t. the cotangent v is A w2 — through the backward of the backward."""
    bank = host_taps("db4")
    for shape, ndim in (((2, 13), 1), ((2, 5, 7), 2), ((2, 33, 65), 2)):
        x64 = _gauss(shape, 3 + sum(shape))

        def second(x, dec):
            x = x.requires_grad_(True)
            flat = _flat(dec(x))
            vs = [w.to(x.device).requires_grad_(True) for w in _cotangents(flat, 5)]
            (g_x,) = torch.autograd.grad(flat, x, vs, create_graph=True)
            w2 = _gauss(g_x.shape, 77).to(x.device)
            return g_x, torch.autograd.grad((g_x * w2).sum(), vs)

        want_g, want = second(x64.clone(), lambda t: R.wavedecn(t, bank, mode, ndim, 2))
        got_g, got = second(x64.clone().to(dev()), lambda t: _api_to_ref(_DEC[ndim][0](t, "db4", mode=mode, level=2), ndim))
        _check(got_g, want_g, F64_GRAD_TOL, (mode, shape, "first order under create_graph"))
        for i, (a, b) in enumerate(zip(got, want)):
            _check(a, b, F64_GRAD_TOL, (mode, shape, "second order, cotangent %d" % i), "second order float64")


# ---- 5. entry by entry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "axis"])
@pytest.mark.parametrize("mode", MODES)
def test_operator_entry_by_entry(mode, route):
    """Unit impulses through the level give the columns of its matrix, unit impulses through the adjoint its rows: entry by entry the
    reference operator, which sees a wrong edge weight that a norm-wise bound on random data could pass."""
    lo, hi = host_taps("db4")[:2]
    _ext.FORCE_AXIS = route == "axis"
    try:
        for n in (13, 16):
            m = (n + 7) // 2
            want = R.matrix(n, lo, hi, mode)  # [2 M, n]
            buf = _ext.level_fwd(torch.eye(n, dtype=torch.float64, device=dev()), lo, hi, mode)  # [n, 2, M]: row i = A e_i
            a = buf.reshape(n, 2 * m).T.cpu()
            g = torch.eye(2 * m, dtype=torch.float64, device=dev()).reshape(2 * m, 2, m)
            at = _ext.level_adj(g, lo, hi, mode, (n,)).cpu()  # [2 M, n]: row r = A^T e_r
            assert float((a - want).abs().max()) < 1e-12 * float(want.abs().max()), (mode, route, n, "level")
            assert float((at - want).abs().max()) < 1e-12 * float(want.abs().max()), (mode, route, n, "adjoint")
            assert float((a - at).abs().max()) < 1e-12 * float(want.abs().max()), (mode, route, n, "transposes")
    finally:
        _ext.FORCE_AXIS = False


# ---- 6. capture and canaries -----------------------------------------------------------------------------------------------------------
def test_capture_replays_to_the_same_bits():
    g = torch.Generator().manual_seed(8)
    x = torch.randn(3, 45, 80, generator=g).to(dev())
    x2 = torch.randn(3, 45, 80, generator=g).to(dev())

    def flat(c):
        return [c[0]] + [t for lv in c[1:] for t in lv]

    fwd = ptwt_amd.capture(lambda t: ptwt_amd.wavedec2(t, "db4", mode="smooth", level=2), x)
    eager = flat(ptwt_amd.wavedec2(x2, "db4", mode="smooth", level=2))
    before = _counts()
    replay = flat(fwd(x2))
    torch.cuda.synchronize()
    assert _delta(before) == [0, 0, 0, 0]  # a replay enqueues nothing through the C ABI
    assert len(replay) == len(eager) == 7 and all(torch.equal(a, b) for a, b in zip(replay, eager))


@pytest.mark.parametrize("shape", [(5, 7), (33, 65), (67, 131)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_guard_regions_stay_intact(dtype, shape):
    """The outputs of ids 42 .. 45 embedded in a poisoned allocation (two guard rows above and below, five / six guard columns left and
    right of every plane, guard images at both ends): every element outside keeps the pattern, every one inside is the reference's."""
    b, (h, w), poison = 3, shape, -12345.5
    mode, bank = "antireflect", host_taps("db4")
    flen = len(bank[0])
    mh, mw = (h + flen - 1) // 2, (w + flen - 1) // 2
    lib, dt, mid = _ext._lib(), _engine._DTYPE_IDS[dtype], _ext.MODES[mode]
    ref = _cell(mode, "db4", (b, h, w))
    x, g = ref["x"].to(dtype).to(dev()), ref["g"].to(dtype).to(dev())
    lo, hi = _engine._taps_array(bank[0]), _engine._taps_array(bank[1])
    stream = _engine._stream_of(x)

    def embedded(nout, eh, ew):
        block = torch.full((nout * b + 2, eh + 4, ew + 11), poison, dtype=dtype, device=dev())
        planes = [block[1 + q * b:1 + (q + 1) * b, 2:2 + eh, 5:5 + ew] for q in range(nout)]
        inside = torch.zeros_like(block, dtype=torch.bool)
        for q in range(nout):
            inside[1 + q * b:1 + (q + 1) * b, 2:2 + eh, 5:5 + ew] = True
        return block, planes, inside

    def strides3(t):
        return (ctypes.c_int64 * 3)(*t.stride())

    # id 42
    block, planes, inside = embedded(4, mh, mw)
    d = _engine._desc(2, dtype, 0, flen, b, (h, w), x.stride(), (mh, mw), planes[0].stride(), planes[1].stride())
    _engine._check(lib.mifwt_ext_fwd(ctypes.byref(d), mid, x.data_ptr(), planes[0].data_ptr(), _engine._ptr_array(planes[1:]), lo, hi, stream))
    torch.cuda.synchronize()
    assert bool((block[~inside] == poison).all()), "id 42: a guard element was overwritten"
    for q in range(4):
        _check(planes[q], ref["fwd"][q], _tol(dtype, ref["e_fwd"]), ("guarded level", _name(dtype), shape, q))
    # id 43
    block, planes, inside = embedded(1, h, w)
    gs = (g.stride(0), g.stride(2), g.stride(3))
    d = _engine._desc(2, dtype, 0, flen, b, (h, w), planes[0].stride(), (mh, mw), gs, gs)
    _engine._check(lib.mifwt_ext_adj(ctypes.byref(d), mid, g[:, 0].data_ptr(), _engine._ptr_array([g[:, s] for s in (1, 2, 3)]),
                                     planes[0].data_ptr(), lo, hi, stream))
    torch.cuda.synchronize()
    assert bool((block[~inside] == poison).all()), "id 43: a guard element was overwritten"
    _check(planes[0], ref["adj"], _tol(dtype, ref["e_adj"]), ("guarded adjoint", _name(dtype), shape))
    # id 44: along the rows axis of [b, h, w] into embedded [b, mh, w] planes; id 45: back into an embedded [b, h, w] plane
    x64 = ref["x"]
    want_lo, want_hi = R.dwt_axis(x64, bank[0], bank[1], mode, 1)
    block, planes, inside = embedded(2, mh, w)
    _engine._check(lib.mifwt_ext_axis_fwd(mid, dt, flen, b, h, w, x.data_ptr(), strides3(x), planes[0].data_ptr(), strides3(planes[0]),
                                          planes[1].data_ptr(), strides3(planes[1]), lo, hi, stream))
    torch.cuda.synchronize()
    assert bool((block[~inside] == poison).all()), "id 44: a guard element was overwritten"
    e32 = R.e_ref32(lambda t: list(R.dwt_axis(t, bank[0], bank[1], mode, 1)), x64)
    _check(planes[0], want_lo, _tol(dtype, e32), ("guarded axis level lo", _name(dtype), shape))
    _check(planes[1], want_hi, _tol(dtype, e32), ("guarded axis level hi", _name(dtype), shape))
    ga, gd = want_lo.to(dtype).to(dev()), want_hi.to(dtype).to(dev())
    want_adj = R.adj_axis(ga.cpu().double(), gd.cpu().double(), bank[0], bank[1], mode, h, 1)
    e32 = R.e_ref32(lambda p, q: R.adj_axis(p, q, bank[0], bank[1], mode, h, 1), ga.cpu().double(), gd.cpu().double())
    block, planes, inside = embedded(1, h, w)
    _engine._check(lib.mifwt_ext_axis_adj(mid, dt, flen, b, h, w, ga.data_ptr(), strides3(ga), gd.data_ptr(), strides3(gd),
                                          planes[0].data_ptr(), strides3(planes[0]), lo, hi, stream))
    torch.cuda.synchronize()
    assert bool((block[~inside] == poison).all()), "id 45: a guard element was overwritten"
    _check(planes[0], want_adj, _tol(dtype, e32), ("guarded axis adjoint", _name(dtype), shape))


def test_print_worst():
    """Runs last (file order)."""
    print("\nworst norm-wise errors vs the float64 reference:", {k: "%.2e" % v for k, v in sorted(WORST.items())})


def measure_reference_f32():
    """The float32 reference's own gradient error over the gradient cases (host, no GPU): the yardstick of F32_GRAD_TOL."""
    worst = (0.0, None)
    for shape, ndim in GRAD_CASES:
        for wavelet in GRAD_WAVELETS:
            for mode in MODES:
                bank = host_taps(wavelet)
                x64 = _gauss(shape, sum(shape))
                e = R.relerr(_ref_grad(x64, bank, mode, ndim, torch.float32)[0], _ref_grad(x64, bank, mode, ndim, torch.float64)[0])
                print(shape, wavelet, mode, "%.3e" % e)
                if e > worst[0]:
                    worst = (e, (shape, wavelet, mode))
    print("float32 reference, worst gradient error: %.3e at %s" % worst)


if __name__ == "__main__":
    measure_reference_f32()
