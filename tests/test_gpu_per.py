"""GPU tests (``-m gpu``) of the periodized levels (csrc/mifwt_per.hip, kernel ids 38 .. 41) and of ``mode="periodization"`` of the
public transforms, against the float64 torch reference tests/_per_ref.py (which tests/test_per_host.py pins to PyWavelets' goldens).

1. Single levels through ``_per.level_fwd`` / ``level_inv``: banks of two INDEPENDENT random filters scaled by 1 / sqrt(L); the unrolled
   lengths 2, 4, 6, 8, 10, 20 on the fused route (L/2 odd for 6 and 10, even for 4, 8, 20: the phase that slicing a periodic level gets
   wrong) and 22, 34 on the axis route; float32 and float64; 1 and 3 images; planes 1x1, 2x3, 5x7, 3x40 (every window wraps several
   times), 33x65, 64x256, 130x258, 257x64 (odd against even, across tile seams), 1x300, 300x1; rows of 1, 2, 3, 7, 64, 257, 4099 samples;
   dense operands and slices of a wider and taller tensor at an odd element offset (no 16-byte alignment: the scalar tails run);
   synthesis to both 2 M and 2 M - 1 samples.  ``mifwt_launch_count`` must show ids 38 / 39 or 40 / 41 as intended per cell; every fused
   cell is also run with ``FORCE_AXIS``.
2. The API: every golden of tests/golden/pywt_per.npz through ``wavedec*`` / ``waverec*`` / ``fswavedec*`` / ``fswaverec*`` (separable
   containers compared by key), the round trip, non-default ``axes`` (axis route), the launches of a 3-D level, a 3-D level and the
   2-D level of the folded shape one after the other in both orders (their inner launches differ in the band strides only);
   ``WaveletPacket`` (db2,
   depth 3, 2x37) and ``WaveletPacket2D`` (haar and db2, depth 2, 2x13x10, both values of ``separable``): every node against the
   reference applied recursively, one launch per tree level, ``reconstruct()`` against the input extended to its even extents.
3. Data gradients of ``wavedec*`` w.r.t. the input and of ``waverec*`` w.r.t. every coefficient leaf against float64 autograd of the
   reference, cosine weights; one float64 double backward.
4. Guard bands around output planes embedded in a poisoned allocation; ``ptwt_amd.capture`` replays.

Bounds, norm-wise per tensor (``tests._golden.relerr``) with a max-abs companion of 10 x bound x the largest value: float64 1e-12
(values) / 1e-10 (gradients).  float32 values: max(1e-6, 10 x e_ref32(cell)), e_ref32 = the error of the reference's float32 tap-by-tap
run against its own float64 run on the same inputs, computed on the host per cell — on an axis shorter than the filter the taps alias
onto the same samples and random taps cancel; the factor 10 is the project's margin for another summation order.  Only a band that is
zero in exact arithmetic (the details of an axis of one sample: below ``_per_ref.ZERO_BAND`` of the input's norm) is measured relative
to the norm of the transform's input, in the comparison and in e_ref32 alike; every other tensor against its own norm.
float32 gradients: ``python -m tests.test_gpu_per`` runs the reference in float32 on the host over GRAD_CASES and prints its worst
norm-wise gradient error against its float64 run: 8.76e-6 (waverec2 of 2x33x65 db4 w.r.t. its finest diagonal leaf; 4.6e-6 for 3x101 db4,
1.2e-6 and below elsewhere); the bound is ten times that, F32_GRAD_TOL = 8.8e-5.
WORST_ON_MI355X holds the worst errors the module showed on the MI355X (printed by its last test).
"""
import ctypes

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, _per
from ptwt_amd._wavelets import host_taps
from tests import _golden as G
from tests import _per_ref as R

pytestmark = pytest.mark.gpu

F64_TOL, F64_GRAD_TOL = 1e-12, 1e-10
F32_GRAD_TOL = 8.8e-5  # 10 x the float32 reference's own worst gradient error over GRAD_CASES (module docstring)
# worst norm-wise errors the module showed on the MI355X (printed by its last test).  "level fwd": the 2-tap bank on the 1x1 plane, whose
# two random taps nearly cancel — the float32 reference itself is at 5.4e-4 there (its bound 5.4e-3), the float64 one at the 1e-13
# level on both routes; every other single-level cell is at or below 4e-7 / 5e-15.  "api values float32": one-sample bands at level 3
# of 8 samples, small against the input (bior2.2 detail 3.5e-6 against its bound of 3.0e-5; bior3.5 approximation 2.2e-6 against
# 8.1e-6, the check closest to its bound at 0.27 of it); 2.5e-7 and below elsewhere.
WORST_ON_MI355X = {
    "api round trip float32": 2.53e-07, "api round trip float64": 7.32e-16, "api values float32": 3.51e-06,
    "api values float64": 4.96e-14, "coefficient gradients float32": 6.18e-06, "coefficient gradients float64": 1.60e-14,
    "data gradients float32": 1.00e-07, "data gradients float64": 2.47e-16, "level fwd axis float32": 1.31e-07,
    "level fwd axis float64": 7.66e-13, "level fwd fused float32": 5.75e-04, "level fwd fused float64": 9.25e-13,
    "level inv axis float32": 1.13e-07, "level inv axis float64": 4.49e-15, "level inv fused float32": 2.34e-07,
    "level inv fused float64": 4.49e-15, "mixed 3-D / 2-D float32": 9.57e-08, "mixed 3-D / 2-D float64": 2.86e-16,
    "packet nodes float32": 1.58e-07, "packet nodes float64": 4.03e-16, "packet reconstruct float32": 1.63e-07,
    "packet reconstruct float64": 5.97e-16, "second order float64": 6.40e-16,
}

WORST = {}
DTYPES = (torch.float32, torch.float64)
FUSED_LENGTHS = (2, 4, 6, 8, 10, 20)
AXIS_LENGTHS = (22, 34)
PLANES = [(1, 1), (2, 3), (5, 7), (3, 40), (33, 65), (64, 256), (130, 258), (257, 64), (1, 300), (300, 1)]
ROWS = [1, 2, 3, 7, 64, 257, 4099]
KIDS = (38, 39, 40, 41)


def dev():
    return torch.device("cuda:0")


def weight(t, i):
    return torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64, device=t.device) + i).reshape(t.shape).to(t.dtype)


def _name(dtype):
    return str(dtype).split(".")[-1]


def random_bank(flen, seed, dtype):
    """(dec_lo, dec_hi, rec_lo, rec_hi): four independent filters scaled by 1 / sqrt(L), already representable in ``dtype``."""
    g = np.random.default_rng(7000 + seed)
    q = (lambda v: float(v)) if dtype == torch.float64 else (lambda v: float(np.float32(v)))
    return tuple(tuple(q(v) for v in g.standard_normal(flen) / np.sqrt(flen)) for _ in range(4))


def _check(got, want, tol, what, key=None, scale=0.0):
    got = got.detach().double().cpu()
    want = torch.as_tensor(want).detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    zero_band = bool(scale) and float(want.norm()) < R.ZERO_BAND * scale  # (zero in exact arithmetic: relative to the input's norm)
    err = float((got - want).norm()) / scale if zero_band else G.relerr(got.numpy(), want.numpy())
    if key is not None:
        WORST[key] = max(WORST.get(key, 0.0), float(err))
    print("%s: %.3e (bound %.1e)" % (what, err, tol))
    assert err < tol, (what, err)
    if want.numel():
        assert float((got - want).abs().max()) <= 10 * tol * max(float(want.abs().max()), scale if zero_band else 0.0, 1e-30), (what, "max-abs")
    return err


def _value_tol(dtype, e32):
    return F64_TOL if dtype == torch.float64 else max(1e-6, 10 * e32)


def _counts():
    return [_engine.launch_count(k) for k in KIDS]


def _delta(before):
    return [a - b for a, b in zip(_counts(), before)]


def _operand(shape, layout, dtype, gen):
    """A tensor of ``shape`` [b, (h,) w] with contiguous samples: dense, or a slice of a taller and wider allocation that starts at an
    odd element offset (row stride w + 7, image stride (h + 3)(w + 7) + 1)."""
    if layout == "dense":
        return torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype).to(dev())
    b, w = shape[0], shape[-1]
    h = shape[1] if len(shape) == 3 else 1
    rs, bs = w + 7, (h + 3) * (w + 7) + 1
    off = rs + 2 + ((rs + 2) % 2 == 0)
    store = torch.randn(off + b * bs + 8, generator=gen, dtype=torch.float64).to(dtype).to(dev())
    if len(shape) == 3:
        return torch.as_strided(store, (b, h, w), (bs, rs, 1), off)
    return torch.as_strided(store, (b, w), (bs, 1), off)


# ---- 1. single levels ------------------------------------------------------------------------------------------------------------------
def _level_cell(dtype, flen, shape, layout, seed):
    """Analysis and synthesis (to 2 M and to 2 M - 1) of one geometry on the default route and, for a fused cell, on the axis route."""
    ndim = len(shape) - 1
    bank = random_bank(flen, seed, dtype)
    gen = torch.Generator().manual_seed(seed)
    fused = flen <= 20
    x = _operand(shape, layout, dtype, gen)
    coef = (shape[0], *[(n + 1) // 2 for n in shape[1:]])
    bands = [_operand(coef, layout, dtype, gen) for _ in range(1 << ndim)]
    xh, bh = x.cpu().double(), [t.cpu().double() for t in bands]
    want_f = R.level_fwd(xh, bank, ndim)
    e32_f = R.e_ref32(lambda t: R.level_fwd(t, bank, ndim), xh) if dtype == torch.float32 else 0.0
    full = [2 * m for m in coef[1:]]
    outs = [full, [n - 1 for n in full]]
    want_i = [R.level_inv(bh, bank, ndim, ext) for ext in outs]
    e32_i = [R.e_ref32(lambda *t: R.level_inv(list(t), bank, ndim, ext), *bh) if dtype == torch.float32 else 0.0 for ext in outs]
    tag = "%s L%d %s %s" % (_name(dtype), flen, "x".join(map(str, shape)), layout)
    for route in (("fused", "axis") if fused else ("axis",)):
        _per.FORCE_AXIS = route == "axis" and fused
        try:
            before = _counts()
            buf = _per.level_fwd(x, bank[0], bank[1])
            ys = [_per.level_inv(bands, bank[2], bank[3], ext) for ext in outs]
            torch.cuda.synchronize()
            d = _delta(before)
        finally:
            _per.FORCE_AXIS = False
        if route == "fused":
            assert d == [1, 2, 0, 0], (tag, d)
        else:
            n_axis = (1 << ndim) - 1
            assert d == [0, 0, n_axis, 2 * n_axis], (tag, d)
        assert buf.shape == (shape[0], 1 << ndim, *coef[1:])
        for s in range(1 << ndim):
            _check(buf[:, s], want_f[s], _value_tol(dtype, e32_f), "fwd %s %s band %d" % (route, tag, s), "level fwd %s %s" % (route, _name(dtype)))
        for y, w_, ext, e32 in zip(ys, want_i, outs, e32_i):  # (each output extent against the reference's float32 error on that output)
            _check(y, w_, _value_tol(dtype, e32), "inv %s %s -> %s" % (route, tag, ext), "level inv %s %s" % (route, _name(dtype)))


@pytest.mark.parametrize("flen", FUSED_LENGTHS + AXIS_LENGTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_single_levels_2d(dtype, flen):
    for pi, (h, w) in enumerate(PLANES):
        for li, layout in enumerate(("dense", "slice")):
            _level_cell(dtype, flen, (1 if (pi + li + flen // 2) % 2 else 3, h, w), layout, 100 * flen + 2 * pi + li)


@pytest.mark.parametrize("flen", FUSED_LENGTHS + AXIS_LENGTHS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_single_levels_1d(dtype, flen):
    for ri, n in enumerate(ROWS):
        for layout in ("dense", "slice"):
            _level_cell(dtype, flen, (1 if (ri + flen // 2) % 2 else 3, n), layout, 100 * flen + 70 + ri)


# ---- 2. the API ------------------------------------------------------------------------------------------------------------------------
def _flat_api(coeffs, ndim, fs=False):
    out = {"a": coeffs[0]}
    for i, c in enumerate(coeffs[1:]):
        if ndim == 1:
            out["%d" % i] = c
        elif ndim == 2 and not fs:
            out["%d_h" % i], out["%d_v" % i], out["%d_d" % i] = c
        elif ndim == 2:
            out["%d_h" % i], out["%d_v" % i], out["%d_d" % i] = c["da"], c["ad"], c["dd"]
        else:
            out.update({"%d_%s" % (i, k): v for k, v in c.items()})
    return out


_DEC = {1: (ptwt_amd.wavedec, ptwt_amd.waverec), 2: (ptwt_amd.wavedec2, ptwt_amd.waverec2), 3: (ptwt_amd.wavedec3, ptwt_amd.waverec3)}
_FS = {2: (ptwt_amd.fswavedec2, ptwt_amd.fswaverec2), 3: (ptwt_amd.fswavedec3, ptwt_amd.fswaverec3)}


@pytest.mark.parametrize("ndim", [1, 2, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_api_matches_pywavelets_goldens(dtype, ndim):
    cases = [c for c in R.goldens() if c["ndim"] == ndim]
    assert len(cases) == {1: 270, 2: 36, 3: 18}[ndim]
    for c in cases:
        bank = host_taps(c["wavelet"])
        x = c["x"].to(dtype)
        scale = float(x.double().norm())
        e32 = e32_rec = 0.0
        if dtype == torch.float32:
            e32 = R.e_ref32(lambda t: list(R.flat_ref(R.wavedecn(t, bank, ndim, c["level"]), ndim).values()), x.double(), scale=scale)
            e32_rec = R.e_ref32(lambda t: R.waverecn(R.wavedecn(t, bank, ndim, c["level"]), bank, ndim), x.double())
        tol = _value_tol(dtype, e32)
        what = "%s %s %s L%d" % (_name(dtype), c["wavelet"], c["shape"], c["level"])
        for fs in ((False, True) if ndim > 1 else (False,)):
            dec, rec = (_FS if fs else _DEC)[ndim]
            coeffs = dec(x.to(dev()), c["wavelet"], mode="periodization", level=c["level"])
            got = _flat_api(coeffs, ndim, fs)
            assert set(got) == set(c["coeffs"])
            for k, t in got.items():
                _check(t, c["coeffs"][k].to(dtype), tol, "%s %s %s" % ("fs" if fs else "", what, k), "api values %s" % _name(dtype), scale)
            y = rec(coeffs, c["wavelet"], mode="periodization")
            _check(y, c["rec"].to(dtype), _value_tol(dtype, e32_rec), "rec %s" % what, "api round trip %s" % _name(dtype), scale)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_level_none_axes_and_launches(dtype):
    g = torch.Generator().manual_seed(5)
    bank = host_taps("db2")
    # level=None is dwtn_max_level, as for every mode
    x = torch.randn(2, 37, 50, generator=g, dtype=torch.float64).to(dtype)
    coeffs = ptwt_amd.wavedec2(x.to(dev()), "db2", mode="periodization")
    nlev = ptwt_amd._wavelets.dwtn_max_level((37, 50), 4)
    assert len(coeffs) == nlev + 1 and coeffs[0].shape[-2:] == (5, 7)
    want = R.wavedecn(x.double(), bank, 2, nlev)
    f32 = dtype == torch.float32  # (float32 bounds: the reference's own float32 error on the same inputs, per computation)
    e32 = R.e_ref32(lambda t: R.wavedecn(t, bank, 2, nlev)[0], x.double()) if f32 else 0.0
    _check(coeffs[0], want[0], _value_tol(dtype, e32), "level=None approx")
    # non-default axes: the transposed problem on the axis route (non-unit innermost stride), without a fused launch
    before = _counts()
    got = ptwt_amd.wavedec2(x.to(dev()), "db2", mode="periodization", level=2, axes=(-1, -2))
    y = ptwt_amd.waverec2(got, "db2", mode="periodization", axes=(-1, -2))
    torch.cuda.synchronize()
    d = _delta(before)
    # (level 1 sees the permuted input; level 2 decomposes the dense approximation of level 1, and the coefficients, permuted back by
    # the synthesis, are the dense planes the analysis wrote: fused)
    assert d == [1, 2, 3, 0], d
    xt = x.double().transpose(-1, -2)
    want = R.wavedecn(xt, bank, 2, 2)
    e32 = R.e_ref32(lambda t: [c_ for lv in R.wavedecn(t, bank, 2, 2) for c_ in (lv if isinstance(lv, list) else [lv])], xt) if f32 else 0.0
    e32_rt = R.e_ref32(lambda t: R.waverecn(R.wavedecn(t, bank, 2, 2), bank, 2), xt) if f32 else 0.0
    _check(got[0], want[0].transpose(-1, -2), _value_tol(dtype, e32), "axes approx")
    for lvl in (1, 2):
        for t, s in zip(got[lvl], (1, 0, 2)):  # (H, V, D) = bands 2, 1, 3
            _check(t, want[lvl][s].transpose(-1, -2), _value_tol(dtype, e32), "axes level %d band %d" % (lvl, s + 1))
    ext = torch.cat([x, x[:, -1:, :]], 1)
    _check(y, ext, _value_tol(dtype, e32_rt), "axes round trip")
    # 1-D along a leading axis: strided rows, no copy, axis route
    before = _counts()
    c1 = ptwt_amd.wavedec(x[0].to(dev()), "db2", mode="periodization", level=1, axis=-2)
    torch.cuda.synchronize()
    assert _delta(before) == [0, 0, 1, 0]
    w1 = R.level_fwd(x[0].double().transpose(-1, -2), bank, 1)
    e32 = R.e_ref32(lambda t: R.level_fwd(t, bank, 1)[1], x[0].double().transpose(-1, -2)) if f32 else 0.0
    _check(c1[1], w1[1].transpose(-1, -2), _value_tol(dtype, e32), "wavedec axis=-2 detail")
    # a 3-D level: the fused launch over the planes and one axis launch along depth; its synthesis: four axis launches and the fused one
    v = torch.randn(2, 9, 8, 12, generator=g, dtype=torch.float64).to(dtype).to(dev())
    before = _counts()
    c3 = ptwt_amd.wavedec3(v, "db2", mode="periodization", level=1)
    assert _delta(before) == [1, 0, 1, 0]
    before = _counts()
    y3 = ptwt_amd.waverec3(c3, "db2", mode="periodization")
    assert _delta(before) == [0, 1, 0, 4]
    assert c3[0].shape == (2, 5, 4, 6) and y3.shape == (2, 10, 8, 12)
    # the headline shapes halve exactly
    big = torch.randn(2, 256, 256, generator=g).to(dev())
    cb = ptwt_amd.wavedec2(big, "db4", mode="periodization", level=3)
    assert [tuple(cb[0].shape[-2:])] + [tuple(c[0].shape[-2:]) for c in cb[1:]] == [(32, 32), (32, 32), (64, 64), (128, 128)]
    _check(ptwt_amd.waverec2(cb, "db4", mode="periodization"), big, 1e-6, "256x256 db4 round trip")


@pytest.mark.parametrize("order", ["3d-first", "2d-first"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_3d_level_and_folded_2d_level_do_not_share_a_plan(dtype, order):
    """``wavedec3`` on (2, 9, 8, 12) runs its fused launch on the folded (18, 8, 12) planes with the band strides of its own temporary;
    ``wavedec2`` on an (18, 8, 12) tensor has the same signal geometry and the band strides of a level buffer.  Whichever comes first
    must not decide the descriptor of the other (the plans are cleared first, so the order is what the test says)."""
    g = torch.Generator().manual_seed(31)
    bank = host_taps("db2")
    v = torch.randn(2, 9, 8, 12, generator=g, dtype=torch.float64).to(dtype)
    f32 = dtype == torch.float32

    def flat3(c):
        return [c[0]] + [t for lv in c[1:] for t in lv]

    def run3():
        c = ptwt_amd.wavedec3(v.to(dev()), "db2", mode="periodization", level=1)
        y = ptwt_amd.waverec3(c, "db2", mode="periodization")
        return [c[0]] + [c[1][format(s, "03b").replace("0", "a").replace("1", "d")] for s in range(1, 8)], y

    def run2():
        c = ptwt_amd.wavedec2(v.reshape(18, 8, 12).to(dev()), "db2", mode="periodization", level=1)
        y = ptwt_amd.waverec2(c, "db2", mode="periodization")
        return [c[0], c[1][1], c[1][0], c[1][2]], y

    _per._plans.clear()
    got = {}
    for which in (("3d", "2d") if order == "3d-first" else ("2d", "3d")):
        got[which] = run3() if which == "3d" else run2()
        torch.cuda.synchronize()
    for which, ndim, x64 in (("3d", 3, v.double()), ("2d", 2, v.double().reshape(18, 8, 12))):
        want = flat3(R.wavedecn(x64, bank, ndim, 1))
        e32 = R.e_ref32(lambda t: flat3(R.wavedecn(t, bank, ndim, 1)), x64) if f32 else 0.0
        e32_rt = R.e_ref32(lambda t: R.waverecn(R.wavedecn(t, bank, ndim, 1), bank, ndim), x64) if f32 else 0.0
        bands, y = got[which]
        for s, (a, b) in enumerate(zip(bands, want)):
            _check(a, b, _value_tol(dtype, e32), "%s %s %s band %d" % (order, which, _name(dtype), s), "mixed 3-D / 2-D %s" % _name(dtype))
        ext = torch.cat([x64, x64.narrow(1, 8, 1)], 1) if ndim == 3 else x64
        _check(y, ext, _value_tol(dtype, e32_rt), "%s %s %s round trip" % (order, which, _name(dtype)), "mixed 3-D / 2-D %s" % _name(dtype))


def _packet_nodes(x, bank, ndim, bands, depth):
    """{key: float64 tensor} of every node down to ``depth``: the reference level applied recursively, key char -> band."""
    nodes, level = {"": x}, [""]
    for _ in range(depth):
        nxt = []
        for key in level:
            out = R.level_fwd(nodes[key], bank, ndim)
            for ch, s in bands.items():
                nodes[key + ch] = out[s]
                nxt.append(key + ch)
        level = nxt
    return nodes


def _packet_round_trip(x, bank, ndim, bands, depth):
    """The root rebuilt from the leaves of ``depth`` by the reference: an inner node is cropped to the extents it had, the root is not."""
    nodes = _packet_nodes(x, bank, ndim, bands, depth)
    order = sorted(bands, key=bands.get)
    for level in range(depth - 1, -1, -1):
        for key in [k for k in list(nodes) if len(k) == level]:
            kids = [nodes[key + ch] for ch in order]
            ext = [2 * m for m in kids[0].shape[-ndim:]] if level == 0 else list(nodes[key].shape[-ndim:])
            nodes[key] = R.level_inv(kids, bank, ndim, ext)
    return nodes[""]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_packets(dtype):
    g = torch.Generator().manual_seed(21)
    f32 = dtype == torch.float32
    cases = [(1, (2, 37), "db2", 3, None)] + [(2, (2, 13, 10), w, 2, sep) for w in ("haar", "db2") for sep in (False, True)]
    for ndim, shape, wavelet, depth, sep in cases:
        bank = host_taps(wavelet)
        x = torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)
        before = _counts()
        if ndim == 1:
            tree = ptwt_amd.WaveletPacket(x.to(dev()), wavelet, mode="periodization", maxlevel=depth)
        else:
            tree = ptwt_amd.WaveletPacket2D(x.to(dev()), wavelet, mode="periodization", maxlevel=depth, separable=sep)
        want = _packet_nodes(x.double(), bank, ndim, tree._bands, depth)
        keys = [k for k in want if k]
        # (float32 bounds: the reference's own float32 error over the nodes / over the tree and its reconstruction)
        e32 = R.e_ref32(lambda t: [_packet_nodes(t, bank, ndim, tree._bands, depth)[k] for k in keys], x.double()) if f32 else 0.0
        tol = _value_tol(dtype, e32)
        leaves = [k for k in want if len(k) == depth]
        tree.initialize(leaves)
        torch.cuda.synchronize()
        assert _delta(before) == [depth, 0, 0, 0], "a tree level is one launch over all its nodes"
        for key, w_ in want.items():
            if key:
                _check(tree[key], w_, tol, "packet %s %s sep=%s node %s" % (_name(dtype), wavelet, sep, key), "packet nodes %s" % _name(dtype))
        before = _counts()
        tree.reconstruct()
        torch.cuda.synchronize()
        assert _delta(before) == [0, depth, 0, 0], "reconstruct is one synthesis launch per level"
        ext = x
        for a in range(1, len(shape)):
            if shape[a] % 2:
                ext = torch.cat([ext, ext.narrow(a, shape[a] - 1, 1)], a)
        e32 = R.e_ref32(lambda t: _packet_round_trip(t, bank, ndim, tree._bands, depth), x.double()) if f32 else 0.0
        _check(tree[""], ext, _value_tol(dtype, e32), "packet %s %s sep=%s reconstruct" % (_name(dtype), wavelet, sep),
               "packet reconstruct %s" % _name(dtype))


# ---- 3. gradients ----------------------------------------------------------------------------------------------------------------------
GRAD_CASES = [((2, 13, 10), 2), ((2, 33, 65), 2), ((3, 101), 1), ((1, 9, 8, 12), 3)]
GRAD_WAVELETS = ("db2", "db4")
GRAD_LEVEL = 2


def _loss(tensors):
    return sum((t * weight(t, i)).sum() for i, t in enumerate(tensors))


def _ref_to_api(coeffs, ndim):
    """A `_per_ref.wavedecn` result as the container the API takes."""
    out = [coeffs[0]]
    for det in coeffs[1:]:
        if ndim == 1:
            out.append(det[0])
        elif ndim == 2:
            out.append((det[1], det[0], det[2]))
        else:
            out.append({format(s, "03b").replace("0", "a").replace("1", "d"): t for s, t in enumerate(det, start=1)})
    return out


def _api_to_ref(coeffs, ndim):
    out = [coeffs[0]]
    for c in coeffs[1:]:
        if ndim == 1:
            out.append([c])
        elif ndim == 2:
            out.append([c[1], c[0], c[2]])
        else:
            out.append([c[format(s, "03b").replace("0", "a").replace("1", "d")] for s in range(1, 8)])
    return out


def _ref_grads(x64, bank, ndim, dtype):
    """(d loss / d x of wavedec, d loss / d leaves of waverec, the coefficient values the latter was taken at), reference, in ``dtype``."""
    x = x64.to(dtype).requires_grad_(True)
    coeffs = R.wavedecn(x, bank, ndim, GRAD_LEVEL)
    (g_x,) = torch.autograd.grad(_loss([coeffs[0]] + [t for det in coeffs[1:] for t in det]), x)
    leaves = [[t.detach().clone().requires_grad_(True) for t in ([c] if torch.is_tensor(c) else c)] for c in coeffs]
    rec = R.waverecn([leaves[0][0]] + leaves[1:], bank, ndim)
    flat = [t for lv in leaves for t in lv]
    return g_x, list(torch.autograd.grad(_loss([rec]), flat)), [t.detach() for t in flat]


@pytest.mark.parametrize("wavelet", GRAD_WAVELETS)
@pytest.mark.parametrize("case", GRAD_CASES, ids=lambda c: "x".join(map(str, c[0])))
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_data_gradients(dtype, case, wavelet):
    shape, ndim = case
    bank = host_taps(wavelet)
    x64 = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape)), dtype=torch.float64).float().double()
    want_x, want_c, values = _ref_grads(x64, bank, ndim, torch.float64)
    tol = F64_GRAD_TOL if dtype == torch.float64 else F32_GRAD_TOL
    dec, rec = _DEC[ndim]
    x = x64.to(dtype).to(dev()).requires_grad_(True)
    coeffs = dec(x, wavelet, mode="periodization", level=GRAD_LEVEL)
    ref_order = _api_to_ref(coeffs, ndim)
    (g_x,) = torch.autograd.grad(_loss([ref_order[0]] + [t for det in ref_order[1:] for t in det]), x)
    _check(g_x, want_x, tol, "d wavedec%d / d x %s %s %s" % (ndim, _name(dtype), shape, wavelet), "data gradients %s" % _name(dtype))
    # waverec at the reference's coefficient values, every leaf
    it = iter([t.to(dtype).to(dev()).requires_grad_(True) for t in values])
    ref_shape = R.wavedecn(x64, bank, ndim, GRAD_LEVEL)
    leaves = [[next(it) for _ in ([c] if torch.is_tensor(c) else c)] for c in ref_shape]
    flat = [t for lv in leaves for t in lv]
    y = rec(_ref_to_api([leaves[0][0]] + leaves[1:], ndim), wavelet, mode="periodization")
    grads = torch.autograd.grad(_loss([y]), flat)
    for i, (g, w_) in enumerate(zip(grads, want_c)):
        _check(g, w_, tol, "d waverec%d / d leaf %d %s %s %s" % (ndim, i, _name(dtype), shape, wavelet), "coefficient gradients %s" % _name(dtype))


def test_double_backward_float64():
    """The analysis is linear: the derivative of <A^T v, w2> w.r.t. the cotangent v is A w2 — through the backward of the backward."""
    bank = host_taps("db4")
    g = torch.Generator().manual_seed(3)
    x64 = torch.randn(2, 13, 10, generator=g, dtype=torch.float64)

    def second(x, dec, to_ref):
        x = x.requires_grad_(True)
        coeffs = dec(x)
        flat = [coeffs[0]] + [t for det in to_ref(coeffs)[1:] for t in det]
        vs = [weight(t, 3 + i).requires_grad_(True) for i, t in enumerate(flat)]
        (g_x,) = torch.autograd.grad(flat, x, vs, create_graph=True)
        return g_x, torch.autograd.grad((g_x * weight(g_x, 11)).sum(), vs)

    want_g, want = second(x64.clone(), lambda t: R.wavedecn(t, bank, 2, 2), lambda c: c)
    got_g, got = second(x64.clone().to(dev()), lambda t: ptwt_amd.wavedec2(t, "db4", mode="periodization", level=2), lambda c: _api_to_ref(c, 2))
    _check(got_g, want_g, F64_GRAD_TOL, "first order under create_graph")
    for i, (a, b) in enumerate(zip(got, want)):
        _check(a, b, F64_GRAD_TOL, "second order, cotangent %d" % i, "second order float64")


# ---- 4. guard bands and graph capture ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flen", (8, 22))
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_guard_bands_stay_untouched(dtype, flen):
    """One analysis and one synthesis level at 33 x 65 (8 taps: the fused launches through the C ABI; 22 taps: the axis launches), three
    images, the output planes embedded in a poisoned allocation (two guard rows above and below, five / six guard columns left and
    right of every plane, guard images at both ends): every element outside the planes keeps the pattern, every one inside is the
    reference's."""
    b, h, w, poison = 3, 33, 65, -12345.5
    mh, mw = 17, 33
    bank = random_bank(flen, 9, dtype)
    gen = torch.Generator().manual_seed(77)
    lib, dt = _per._lib(), _engine._DTYPE_IDS[dtype]  # (the entries with their argument types)
    x = torch.randn(b, h, w, generator=gen, dtype=torch.float64).to(dtype).to(dev())
    bands = [torch.randn(b, mh, mw, generator=gen, dtype=torch.float64).to(dtype).to(dev()) for _ in range(4)]
    want_f = R.level_fwd(x.cpu().double(), bank, 2)
    want_i = R.level_inv([t.cpu().double() for t in bands], bank, 2, (h, w))
    e32_f = e32_i = 0.0
    if dtype == torch.float32:  # (the reference's own float32 error on these inputs)
        e32_f = R.e_ref32(lambda t: R.level_fwd(t, bank, 2), x.cpu().double())
        e32_i = R.e_ref32(lambda *t: R.level_inv(list(t), bank, 2, (h, w)), *[t.cpu().double() for t in bands])
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

    lo_f, hi_f, lo_i, hi_i = (_engine._taps_array(t) for t in bank)
    # analysis
    block, planes, inside = embedded(4, mh, mw)
    if flen <= 20:
        d = _engine._desc(2, dtype, 0, flen, b, (h, w), x.stride(), (mh, mw), planes[0].stride(), planes[1].stride())
        _engine._check(lib.mifwt_per_fwd(ctypes.byref(d), x.data_ptr(), planes[0].data_ptr(), _engine._ptr_array(planes[1:]), lo_f, hi_f, stream))
    else:  # rows, then columns into the embedded planes
        tmp = torch.empty(2, b, h, mw, dtype=dtype, device=dev())
        _engine._check(lib.mifwt_per_axis_fwd(dt, flen, b * h, w, 1, x.data_ptr(), (ctypes.c_int64 * 3)(w, 1, 1), tmp[0].data_ptr(),
                                               (ctypes.c_int64 * 3)(mw, 1, 1), tmp[1].data_ptr(), (ctypes.c_int64 * 3)(mw, 1, 1), lo_f, hi_f, stream))
        for cb in range(2):
            _engine._check(lib.mifwt_per_axis_fwd(dt, flen, b, h, mw, tmp[cb].data_ptr(), strides3(tmp[cb]), planes[cb].data_ptr(),
                                                   strides3(planes[cb]), planes[2 + cb].data_ptr(), strides3(planes[2 + cb]), lo_f, hi_f, stream))
    torch.cuda.synchronize()
    assert bool((block[~inside] == poison).all()), "analysis: a guard element was overwritten"
    for q in range(4):
        _check(planes[q], want_f[q], _value_tol(dtype, e32_f), ("guarded fwd", _name(dtype), flen, q))
    # synthesis to the odd extents
    block, planes, inside = embedded(1, h, w)
    y = planes[0]
    if flen <= 20:
        d = _engine._desc(2, dtype, 0, flen, b, (h, w), y.stride(), (mh, mw), bands[0].stride(), bands[1].stride())
        _engine._check(lib.mifwt_per_inv(ctypes.byref(d), bands[0].data_ptr(), _engine._ptr_array(bands[1:]), y.data_ptr(), lo_i, hi_i, stream))
    else:  # columns, then rows into the embedded plane
        tmp = torch.empty(2, b, h, mw, dtype=dtype, device=dev())
        for cb in range(2):
            _engine._check(lib.mifwt_per_axis_inv(dt, flen, b, h, mw, bands[cb].data_ptr(), strides3(bands[cb]), bands[2 + cb].data_ptr(),
                                                   strides3(bands[2 + cb]), tmp[cb].data_ptr(), strides3(tmp[cb]), lo_i, hi_i, stream))
        for bi in range(b):  # (an embedded image is no [outer, n, 1] array with one outer stride for rows AND images: one launch per image)
            _engine._check(lib.mifwt_per_axis_inv(dt, flen, h, w, 1, tmp[0][bi].data_ptr(), (ctypes.c_int64 * 3)(mw, 1, 1), tmp[1][bi].data_ptr(),
                                                   (ctypes.c_int64 * 3)(mw, 1, 1), y[bi].data_ptr(), (ctypes.c_int64 * 3)(y.stride(1), 1, 1), lo_i, hi_i, stream))
    torch.cuda.synchronize()
    assert bool((block[~inside] == poison).all()), "synthesis: a guard element was overwritten"
    _check(y, want_i, _value_tol(dtype, e32_i), ("guarded inv", _name(dtype), flen))


def test_capture_replays_on_new_data():
    g = torch.Generator().manual_seed(8)
    x = torch.randn(3, 45, 80, generator=g).to(dev())
    x2 = torch.randn(3, 45, 80, generator=g).to(dev())

    def flat(c):
        return [c[0]] + [t for lv in c[1:] for t in lv]

    fwd = ptwt_amd.capture(lambda t: ptwt_amd.wavedec2(t, "db4", mode="periodization", level=2), x)
    eager = flat(ptwt_amd.wavedec2(x2, "db4", mode="periodization", level=2))
    before = _counts()
    replay = flat(fwd(x2))
    torch.cuda.synchronize()
    assert _delta(before) == [0, 0, 0, 0]  # a replay enqueues nothing through the C ABI
    assert len(replay) == len(eager) == 7 and all(torch.equal(a, b) for a, b in zip(replay, eager))
    shapes = [tuple(t.shape) for t in eager]

    def pack(tensors):  # (a captured call takes ONE tensor: the coefficients end to end)
        return torch.cat([t.reshape(-1) for t in tensors])

    def rec(buf):
        parts, off = [], 0
        for shp in shapes:
            n = int(np.prod(shp))
            parts.append(buf[off:off + n].view(shp))
            off += n
        return ptwt_amd.waverec2((parts[0], tuple(parts[1:4]), tuple(parts[4:7])), "db4", mode="periodization")

    inv = ptwt_amd.capture(rec, pack(eager))
    other = pack(flat(ptwt_amd.wavedec2(x, "db4", mode="periodization", level=2)))
    y = inv(other)
    assert torch.equal(y, rec(other))
    _check(y[:, :45], x, 1e-6, "captured round trip")


def test_print_worst():
    """Runs last (file order)."""
    print("\nworst norm-wise errors vs the float64 references:", {k: "%.2e" % v for k, v in sorted(WORST.items())})


def measure_reference_f32():
    """The float32 reference's own gradient error over GRAD_CASES (host, no GPU): the yardstick of F32_GRAD_TOL."""
    worst = (0.0, None)
    for shape, ndim in GRAD_CASES:
        for wavelet in GRAD_WAVELETS:
            bank = host_taps(wavelet)
            x64 = torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape)), dtype=torch.float64).float().double()
            gx64, gc64, _ = _ref_grads(x64, bank, ndim, torch.float64)
            gx32, gc32, _ = _ref_grads(x64, bank, ndim, torch.float32)
            errs = [("wavedec", R.relerr(gx32, gx64))] + [("waverec leaf %d" % i, R.relerr(a, b)) for i, (a, b) in enumerate(zip(gc32, gc64))]
            for what, e in errs:
                if e > worst[0]:
                    worst = (e, (shape, wavelet, what))
            print(shape, wavelet, "worst %.3e" % max(e for _, e in errs))
    print("float32 reference, worst gradient error: %.3e at %s" % worst)


if __name__ == "__main__":
    measure_reference_f32()
