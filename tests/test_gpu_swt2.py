"""GPU tests (``-m gpu``) of the fused 2-D stationary levels (csrc/mifwt_swt2.hip, kernel ids 34 / 35) and of ``ptwt_amd.swt2`` /
``iswt2`` against the float64 references of tests/_swt2_ref.py (composed from the 1-D stand-ins of tests/_oracle_engine.py, which
tests/test_torch_autograd_ref.py pins to the reference library's goldens).

1. Single level calls, ``stationary_transform._level2_fwd`` / ``_level2_inv``, on the same, already quantised, inputs.  A lane owns
   E = 4 / 2 columns (float32 / float64; half of that above 10 taps) and a wave 64 E, a wave walks one row residue modulo the dilation:
   planes 1x1, 2x3, 5x7 (below a lane's run), 33x65, 64x256, 130x258, 257x64 (tails after a full wave, several strips), 1x300 and
   300x1 (single rows and columns); dilations 1, 2, 4, 8, 3 and 512 (larger than both extents; on the small planes, where every
   window wraps many times); the unrolled lengths 2, 4, 8, 10, 20 (``mifwt_launch_count`` must show the fused launch) and 22, 34 (no
   fused kernel: the composed route must have run, with the same bounds); banks of four INDEPENDENT random filters; 1 and 3 images;
   dense operands, slices of a wider and taller tensor at an odd element offset, the cA plane of a level buffer and, for synthesis,
   four operands with four different stride sets; scales 1, 1/4 and pi/7.  Synthesis inputs are random coefficient sets.  Every
   supported cell is also run on the composed route.
2. ``swt2`` / ``iswt2``: every returned tensor, the round trip, fused against composed, the data gradients (of ``swt2`` w.r.t. the
   input, of ``iswt2`` w.r.t. every coefficient leaf) against float64 autograd of the torch reference, one float64 double backward,
   one case with the four taps as leaf tensors (composed route, four tap gradients).
3. Guard bands around output planes embedded in a poisoned allocation; ``ptwt_amd.capture`` replays.

Bounds, norm-wise per plane (``tests._golden.relerr``) with a max-abs companion of 10 x bound x the largest value, as
tests/test_gpu_swt_kernels.py: float64 1e-12 (values) / 1e-10 (gradients, second order included); float32 values 1e-6.
The float32 GRADIENT bound comes from the reference alone: ``python -m tests.test_gpu_swt2`` runs the torch reference in float32 on
the host over API_CASES and prints its worst norm-wise error against its own float64 run on the same inputs — 6.53e-6 (the
2x40x48 db11 case; 5.31e-6 for 40x56 sym5, 1.3e-6 and below elsewhere: the gradients w.r.t. the approximation leaves are low-passed
oscillating weights, sums that cancel) — and the bound is ten times that, because the GPU sums in another order: F32_GRAD_TOL = 6.5e-5.
WORST_ON_MI355X holds the worst errors the module showed on the MI355X (printed by its last test).

No cell is skipped: a cell whose reference raises must raise in the library too and is counted; the last test fails on a non-zero
count.
"""
import ctypes

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine
from ptwt_amd import stationary_transform as st
from ptwt_amd._wavelets import host_taps
from tests import _golden as G
from tests import _swt2_ref as R2

pytestmark = pytest.mark.gpu

VALUE_TOL = {torch.float64: 1e-12, torch.float32: 1e-6}
F64_GRAD_TOL = 1e-10
F32_GRAD_TOL = 6.5e-5  # 10 x the float32 reference's own worst data / coefficient gradient error (module docstring)
# worst norm-wise errors the module showed on the MI355X (printed by its last test).  Before the host summed the taps that read the
# same sample in double (stationary_transform._merge_aliased) two float32 analysis cells missed 1e-6 on BOTH routes, with identical
# numbers: 1x1, 22 taps, D = 512 (cH 1.09e-6) and 300x1, 20 taps, D = 1 (cV 1.33e-6) — the axis of extent 1 turns the filter into
# the sum of its random taps, which float32 rounded tap by tap.
WORST_ON_MI355X = {
    "level fwd fused float32": 1.28e-7, "level fwd fused float64": 2.77e-15, "level fwd composed float32": 1.57e-7, "level fwd composed float64": 2.77e-15,
    "level inv fused float32": 1.70e-7, "level inv fused float64": 8.72e-16, "level inv composed float32": 2.16e-7, "level inv composed float64": 8.72e-16,
    "swt2 values float32": 1.64e-7, "swt2 values float64": 3.38e-16, "swt2 composed float32": 1.64e-7, "swt2 composed float64": 3.38e-16,
    "swt2 round trip float32": 1.81e-7, "swt2 round trip float64": 5.47e-13,
    "swt2 data gradients float32": 7.31e-6, "swt2 data gradients float64": 1.64e-14,
    "swt2 second order float64": 3.26e-16, "swt2 tap gradients float64": 7.01e-16, "swt2 learnable values float64": 3.05e-16,
}

WORST = {}
COUNTS = {"cells": 0, "skipped": 0}


def dev():
    return torch.device("cuda:0")


def weight(t, i):
    return torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64, device=t.device) + i).reshape(t.shape).to(t.dtype)


def random_bank(flen, seed):
    """Four independent filters scaled by 1 / sqrt(L), as tests/test_gpu_swt_kernels.py."""
    g = np.random.default_rng(4000 + seed)
    return [g.standard_normal(flen) / np.sqrt(flen) for _ in range(4)]


def _name(dtype):
    return str(dtype).split(".")[-1]


def _check(got, want, tol, what, key=None):
    got = got.detach().double().cpu()
    want = torch.as_tensor(want).detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = G.relerr(got.numpy(), want.numpy())
    if key is not None:
        WORST[key] = max(WORST.get(key, 0.0), float(err))
    print("%s: %.3e (bound %.1e)" % (what, err, tol))
    assert err < tol, (what, err)
    if want.numel():
        assert float((got - want).abs().max()) <= 10 * tol * max(float(want.abs().max()), 1e-30), (what, "max-abs")
    return err


def _quantised(values, dtype):
    if dtype == torch.float64:
        return tuple(float(v) for v in values)
    return tuple(float(np.float32(v)) for v in values)


# ---- 1. single level calls ------------------------------------------------------------------------------------------------------------
PLANES = [(1, 1), (2, 3), (5, 7), (33, 65), (64, 256), (130, 258), (257, 64), (1, 300), (300, 1)]
SMALL_DILATIONS = (1, 2, 4, 8, 3)
BIG_DILATION = 512  # larger than every extent above
FUSED_LENGTHS = (2, 4, 8, 10, 20)
COMPOSED_LENGTHS = (22, 34)
LENGTHS = FUSED_LENGTHS + COMPOSED_LENGTHS
SCALES = (1.0, 0.25, float(np.pi / 7))
LAYOUTS = ("contiguous", "slice", "plane", "mixed")
DTYPES = (torch.float32, torch.float64)


def _cells():
    """Not the full product: every plane meets every length, the other factors rotate through the cells; the dilation larger than the
    extents goes to the small planes (at most 65 columns), the big planes take the dilations of a three- or four-level transform."""
    cells = []
    for dtype in DTYPES:
        for pi, (h, w) in enumerate(PLANES):
            for li, flen in enumerate(LENGTHS):
                i = len(cells)
                dils = SMALL_DILATIONS + (BIG_DILATION,) if h * w <= 33 * 65 else SMALL_DILATIONS
                cells.append((dtype, h, w, flen, dils[(pi + li) % len(dils)], 1 if (pi + li) % 2 else 3, LAYOUTS[i % 4], SCALES[i % 3]))
    return cells


CELLS = _cells()


def _cell_id(c):
    return "%s-%dx%d-L%d-D%d-B%d-%s-s%.3g" % (_name(c[0]), c[1], c[2], c[3], c[4], c[5], c[6], c[7])


def _operand(b, h, w, layout, dtype, gen):
    """A [b, h, w] operand with contiguous samples: dense; a slice of a taller and wider tensor (odd element offset, row stride w + 7,
    image stride (h + 3)(w + 7)); plane 0 / 2 of a [b, 4, h, w] level buffer; plane 1 of a [b, 2, h, w] buffer."""
    def rnd(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype).to(dev())

    if layout == "contiguous":
        return rnd(b, h, w)
    if layout == "slice":
        t = rnd(b, h + 3, w + 7)[:, 2:2 + h, 3:3 + w]
        assert t.storage_offset() % 2 == 1
        return t
    if layout == "plane":
        return rnd(b, 4, h, w)[:, 0]
    if layout == "plane2":
        return rnd(b, 4, h, w)[:, 2]
    assert layout == "pair1"
    return rnd(b, 2, h, w)[:, 1]


def _run_cell(direction, cell):
    dtype, h, w, flen, dilation, b, layout, scale = cell
    bank = random_bank(flen, 7 * flen + h + w)
    taps = tuple(_quantised(t, dtype) for t in bank)
    (scale,) = _quantised([scale], dtype)
    gen = torch.Generator().manual_seed(flen * 100003 + 1009 * h + w + dilation)
    if direction == "fwd":
        ops = [_operand(b, h, w, "slice" if layout == "mixed" else layout, dtype, gen)]
        kid = st.KID_SWT2
    else:
        lay = ("slice", "plane2", "contiguous", "pair1") if layout == "mixed" else (layout,) * 4
        ops = [_operand(b, h, w, l, dtype, gen) for l in lay]
        if layout == "mixed":
            assert len({t.stride() for t in ops}) == 4 or h == 1
        kid = st.KID_ISWT2

    def call(composed):
        if direction == "fwd":
            return st._level2_fwd(ops[0], taps, dilation, scale, composed=composed)
        return st._level2_inv(ops, taps, dilation, scale, composed=composed)

    keep = [t.clone() for t in ops]
    COUNTS["cells"] += 1
    host = [t.double().cpu().numpy() for t in ops]
    try:
        if direction == "fwd":
            want = np.stack(R2.level_fwd(host[0], taps, dilation, scale), axis=1)
        else:
            want = R2.level_inv(host, taps, dilation, scale)
    except Exception:
        COUNTS["skipped"] += 1
        with pytest.raises(Exception):
            call(False)
        return
    n0 = _engine.launch_count(kid)
    got = call(False)
    torch.cuda.synchronize()
    ran = _engine.launch_count(kid) - n0
    assert ran == (1 if flen in FUSED_LENGTHS else 0), (_cell_id(cell), "fused launches", ran)
    assert got.dtype == dtype and got.is_contiguous()
    for a, k in zip(ops, keep):
        assert torch.equal(a, k), "an input was modified"
    tol = VALUE_TOL[dtype]
    routes = [("fused" if ran else "composed", got)]
    if ran:
        n1 = _engine.launch_count(kid)
        routes.append(("composed", call(True)))
        assert _engine.launch_count(kid) == n1, "the composed route launched the fused kernel"
    for route, res in routes:
        key = "level %s %s %s" % (direction, route, _name(dtype))
        if direction == "fwd":
            assert res.shape == (b, 4, h, w)
            for q, band in enumerate(("cA", "cH", "cV", "cD")):
                _check(res[:, q], want[:, q], tol, (direction, route, _cell_id(cell), band), key)
        else:
            assert res.shape == (b, h, w)
            _check(res, want, tol, (direction, route, _cell_id(cell)), key)


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_analysis_level_vs_float64_reference(cell):
    _run_cell("fwd", cell)


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_synthesis_level_vs_float64_reference(cell):
    _run_cell("inv", cell)


def test_the_matrix_covers_what_it_claims():
    """(no GPU work) every value of every factor occurs in every dtype; the dilation beyond the extents meets small planes only."""
    for dtype in DTYPES:
        mine = [c for c in CELLS if c[0] == dtype]
        assert {(c[1], c[2]) for c in mine} == set(PLANES)
        assert {c[3] for c in mine} == set(LENGTHS)
        assert {c[4] for c in mine} == set(SMALL_DILATIONS) | {BIG_DILATION}
        assert {c[5] for c in mine} == {1, 3}
        assert {c[6] for c in mine} == set(LAYOUTS) and {c[7] for c in mine} == set(SCALES)
        assert all(c[1] * c[2] <= 33 * 65 and c[4] > max(c[1], c[2]) for c in mine if c[4] == BIG_DILATION)
        for flen in LENGTHS:  # every length on a plane of several strips and on one with a ragged tail
            assert {(130, 258), (33, 65)} <= {(c[1], c[2]) for c in mine if c[3] == flen}
        # windows that wrap several times, rows that wrap (H not a multiple of D, D >= H), fused
        assert any(c[4] * c[3] > 2 * c[2] and c[3] in FUSED_LENGTHS for c in mine)
        assert any(c[1] % c[4] and c[4] < c[1] and c[3] in FUSED_LENGTHS for c in mine)
        assert any(c[4] >= c[1] > 1 and c[3] in FUSED_LENGTHS for c in mine)


def test_level_calls_refuse_bad_lengths_and_take_empty_batches():
    x = torch.randn(2, 8, 16, device=dev())
    for flen in (3, 130):
        taps = ([0.1] * flen,) * 4
        with pytest.raises(RuntimeError, match="libmifwt"):
            st._level2_fwd(x, taps, 1, 1.0)
        with pytest.raises(RuntimeError, match="libmifwt"):
            st._level2_inv((x, x, x, x), taps, 1, 0.25)
    lib = st._swt2_entries()
    four = st._vp4(*[x.data_ptr()] * 4)
    i4 = st._i64x4(128, 128, 128, 128)
    r4 = st._i64x4(16, 16, 16, 16)
    t22 = _engine._taps_array([0.1] * 22)
    # the C entries answer UNSUPPORTED (-2) where the query says no, and BADARG (-1) to odd lengths; nothing is launched
    assert lib.mifwt_swt2_supported(0, 22, 2, 8, 16, 1) == 0
    assert lib.mifwt_swt2_fwd(0, 22, 2, 8, 16, 1, x.data_ptr(), 128, 16, four, i4, r4, t22, t22, t22, t22, 1.0, None) == -2
    assert lib.mifwt_swt2_inv(0, 22, 2, 8, 16, 1, four, i4, r4, x.data_ptr(), 128, 16, t22, t22, t22, t22, 1.0, None) == -2
    assert lib.mifwt_swt2_fwd(0, 3, 2, 8, 16, 1, x.data_ptr(), 128, 16, four, i4, r4, t22, t22, t22, t22, 1.0, None) == -1
    assert lib.mifwt_swt2_fwd(2, 8, 2, 8, 16, 1, x.data_ptr(), 128, 16, four, i4, r4, t22, t22, t22, t22, 1.0, None) == -2
    torch.cuda.synchronize()
    half = (0.5, 0.5), (0.5, -0.5), (0.5, 0.5), (0.5, -0.5)
    for dtype in DTYPES:
        e = torch.empty(0, 8, 16, device=dev(), dtype=dtype)
        assert st._level2_fwd(e, half, 1, 1.0).shape == (0, 4, 8, 16)
        assert st._level2_inv((e, e, e, e), half, 1, 0.25).shape == (0, 8, 16)


# ---- 2. the public functions ----------------------------------------------------------------------------------------------------------
# (name, shape, wavelet, level, axes)
API_CASES = [
    ("2x3x64x96-db4-L3", (2, 3, 64, 96), "db4", 3, (-2, -1)),
    ("40x56-sym5-auto", (40, 56), "sym5", None, (-2, -1)),
    ("axes(-1,-2)-3x48x40-db2-L2", (3, 48, 40), "db2", 2, (-1, -2)),
    ("axes(1,3)-2x24x3x40-db3-L2", (2, 24, 3, 40), "db3", 2, (1, 3)),
    ("3x33x65-db4-L2", (3, 33, 65), "db4", 2, (-2, -1)),         # odd extents: rows and columns wrap off the lattice
    ("2x40x48-db11-L2", (2, 40, 48), "db11", 2, (-2, -1)),       # 22 taps: no fused kernel, the composed route
]


def _flat(coeffs):
    return [coeffs[0]] + [t for c in coeffs[1:] for t in c]


def _nest(flat):
    return [flat[0]] + [tuple(flat[1 + 3 * k:4 + 3 * k]) for k in range((len(flat) - 1) // 3)]


def _api_run(lib, x, wavelet, leaves, level, axes, dtype):
    """Coefficients, the reconstruction of given coefficient leaves, and the gradients of the ``weight`` loss w.r.t. the input and every
    leaf.  ``lib``: the library on the device, or the torch reference on the host in ``x``'s dtype."""
    x = x.detach().requires_grad_(True)
    if lib:
        c = _flat(ptwt_amd.swt2(x, wavelet, level, axes=axes))
    else:
        taps = [_quantised(t, dtype) for t in host_taps(wavelet)]
        c = _flat(R2.t_swt2(x, taps[0], taps[1], level, axes))
    if leaves is None:
        leaves = [t.detach().clone() for t in c]
    leaves = [t.detach().clone().requires_grad_(True) for t in leaves]
    y = ptwt_amd.iswt2(_nest(leaves), wavelet, axes=axes) if lib else R2.t_iswt2(_nest(leaves), taps[2], taps[3], axes)
    loss = sum((weight(t, i) * t).sum() for i, t in enumerate(c)) + (weight(y, 7) * y).sum()
    grads = torch.autograd.grad(loss, [x] + leaves)
    return [t.detach() for t in c], y.detach(), grads[0], list(grads[1:])


def _api_input(case, dtype):
    gen = torch.Generator().manual_seed(sum(case[1]) + len(case[0]))
    return torch.randn(*case[1], generator=gen, dtype=torch.float64).to(dtype)


def measure_reference_f32():
    """The torch reference in float32 on the host against its own float64 run, over API_CASES on the same float32 inputs and
    coefficient leaves: the worst norm-wise error of the data / coefficient gradients.  F32_GRAD_TOL is ten times what this prints."""
    worst = {"values": 0.0, "gradients": 0.0}
    for case in API_CASES:
        name, shape, wavelet, level, axes = case
        x = _api_input(case, torch.float32)
        first = _api_run(False, x.double(), wavelet, None, level, axes, torch.float32)
        leaves = [t.float() for t in first[0]]
        c64, y64, gx64, gl64 = _api_run(False, x.double(), wavelet, [t.double() for t in leaves], level, axes, torch.float32)
        c32, y32, gx32, gl32 = _api_run(False, x, wavelet, leaves, level, axes, torch.float32)
        e_v = max(G.relerr(a.numpy(), b.numpy()) for a, b in zip(c32 + [y32], c64 + [y64]))
        e_g = max(G.relerr(a.numpy(), b.numpy()) for a, b in zip([gx32] + gl32, [gx64] + gl64))
        print("%-30s values %.2e  gradients %.2e" % (name, e_v, e_g))
        worst["values"], worst["gradients"] = max(worst["values"], e_v), max(worst["gradients"], e_g)
    print("worst:", {k: "%.2e" % v for k, v in worst.items()})
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", API_CASES, ids=lambda c: c[0])
def test_swt2_iswt2_vs_reference(case, dtype):
    name, shape, wavelet, level, axes = case
    x = _api_input(case, dtype)
    tag = _name(dtype)
    COUNTS["cells"] += 1
    try:
        first = _api_run(False, x.double(), wavelet, None, level, axes, dtype)
        leaves = [t.to(dtype) for t in first[0]]  # the library reconstructs the reference's coefficients, rounded to its dtype
        want = _api_run(False, x.double(), wavelet, [t.double() for t in leaves], level, axes, dtype)
    except Exception:
        COUNTS["skipped"] += 1
        with pytest.raises(Exception):
            _api_run(True, x.to(dev()), wavelet, None, level, axes, dtype)
        return
    flen = len(host_taps(wavelet)[0])
    n_f, n_i = _engine.launch_count(st.KID_SWT2), _engine.launch_count(st.KID_ISWT2)
    got = _api_run(True, x.to(dev()), wavelet, [t.to(dev()) for t in leaves], level, axes, dtype)
    torch.cuda.synchronize()
    levels = (len(want[0]) - 1) // 3
    assert levels == (level if level is not None else 3)
    # forward of each + backward of the other, per level: fused where the length has a kernel, none otherwise
    per = 2 * levels if flen <= 20 else 0
    assert _engine.launch_count(st.KID_SWT2) - n_f == per and _engine.launch_count(st.KID_ISWT2) - n_i == per
    v_tol, g_tol = VALUE_TOL[dtype], (F64_GRAD_TOL if dtype == torch.float64 else F32_GRAD_TOL)
    assert len(got[0]) == len(want[0])
    for i, (a, b) in enumerate(zip(got[0], want[0])):
        assert a.dtype == dtype and a.shape == x.shape
        _check(a, b, v_tol, (name, tag, "coefficient", i), "swt2 values " + tag)
    _check(got[1], want[1], v_tol, (name, tag, "reconstruction"), "swt2 values " + tag)
    _check(got[2], want[2], g_tol, (name, tag, "d/dx"), "swt2 data gradients " + tag)
    for i, (a, b) in enumerate(zip(got[3], want[3])):
        _check(a, b, g_tol, (name, tag, "d/dcoefficient", i), "swt2 data gradients " + tag)
    # round trip, and the composed route on the same call
    with torch.no_grad():
        xd = x.to(dev())
        coeffs = ptwt_amd.swt2(xd, wavelet, level, axes=axes)
        assert isinstance(coeffs, list) and all(isinstance(c, ptwt_amd.WaveletDetailTuple2d) for c in coeffs[1:])
        _check(ptwt_amd.iswt2(coeffs, wavelet, axes=axes), x, v_tol, (name, tag, "round trip"), "swt2 round trip " + tag)
        n_f, n_i = _engine.launch_count(st.KID_SWT2), _engine.launch_count(st.KID_ISWT2)
        st.FORCE_COMPOSED = True
        try:
            composed = ptwt_amd.swt2(xd, wavelet, level, axes=axes)
            rec = ptwt_amd.iswt2(_nest([t.to(dev()) for t in leaves]), wavelet, axes=axes)
        finally:
            st.FORCE_COMPOSED = False
        assert _engine.launch_count(st.KID_SWT2) == n_f and _engine.launch_count(st.KID_ISWT2) == n_i
        for i, (a, b) in enumerate(zip(_flat(composed), want[0])):
            _check(a, b, v_tol, (name, tag, "composed coefficient", i), "swt2 composed " + tag)
        _check(rec, want[1], v_tol, (name, tag, "composed reconstruction"), "swt2 composed " + tag)


def test_swt2_double_backward_vs_reference():
    """create_graph=True through both transforms (each level op's backward is the other op), float64, odd extents."""
    wavelet, level = "db3", 2
    x = torch.randn(2, 17, 36, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    taps = host_taps(wavelet)

    def second(lib, xx):
        coeffs = _flat(ptwt_amd.swt2(xx, wavelet, level) if lib else R2.t_swt2(xx, taps[0], taps[1], level))
        f = sum((weight(t, i) * t.square()).sum() for i, t in enumerate(coeffs)) / 2
        y = ptwt_amd.iswt2(_nest(coeffs), wavelet) if lib else R2.t_iswt2(_nest(coeffs), taps[2], taps[3])
        f = f + (weight(y, 7) * y.square()).sum() / 2
        (first,) = torch.autograd.grad(f, [xx], create_graph=True)
        s = (first * weight(first, 11)).sum()
        return [first.detach(), torch.autograd.grad(s, [xx])[0]]

    want = second(False, x.clone().requires_grad_(True))
    got = second(True, x.to(dev()).requires_grad_(True))
    for i, (a, b) in enumerate(zip(got, want)):
        _check(a, b, F64_GRAD_TOL, ("double backward", i), "swt2 second order float64")


def test_learnable_taps_take_the_composed_route():
    """The four taps as leaf tensors: no fused launch, and the four tap gradients (and the data gradient) match the reference."""
    flen, level = 6, 2
    bank = random_bank(flen, 99)
    x = torch.randn(2, 20, 28, generator=torch.Generator().manual_seed(6), dtype=torch.float64)

    def run(lib, xx, taps):
        coeffs = ptwt_amd.swt2(xx, tuple(taps), level) if lib else R2.t_swt2(xx, taps[0], taps[1], level)
        y = ptwt_amd.iswt2(coeffs, tuple(taps)) if lib else R2.t_iswt2(coeffs, taps[2], taps[3])
        loss = sum((weight(t, i) * t).sum() for i, t in enumerate(_flat(coeffs))) + (weight(y, 7) * y.square()).sum()
        return [t.detach() for t in _flat(coeffs)] + [y.detach()], torch.autograd.grad(loss, [xx] + list(taps))

    want_v, want_g = run(False, x.clone().requires_grad_(True), [torch.tensor(b).requires_grad_(True) for b in bank])
    n_f, n_i = _engine.launch_count(st.KID_SWT2), _engine.launch_count(st.KID_ISWT2)
    got_v, got_g = run(True, x.to(dev()).requires_grad_(True), [torch.tensor(b, device=dev()).requires_grad_(True) for b in bank])
    torch.cuda.synchronize()
    assert _engine.launch_count(st.KID_SWT2) == n_f and _engine.launch_count(st.KID_ISWT2) == n_i
    for i, (a, b) in enumerate(zip(got_v, want_v)):
        _check(a, b, VALUE_TOL[torch.float64], ("learnable", "value", i), "swt2 learnable values float64")
    for a, b, what in zip(got_g, want_g, ("x", "dec_lo", "dec_hi", "rec_lo", "rec_hi")):
        assert a.shape == b.shape
        _check(a, b, F64_GRAD_TOL, ("learnable", "d/d" + what), "swt2 tap gradients float64")


# ---- 3. guard bands and graph capture ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_guard_bands_stay_untouched(dtype):
    """One analysis and one synthesis launch through the C ABI at 33 x 65, D = 4, 8 taps, three images, the output planes embedded in a
    poisoned allocation (two guard rows above and below, five / six guard columns left and right of every plane, guard images at both
    ends): every element outside the planes still holds the pattern, every element inside is the reference's."""
    b, h, w, flen, dilation, poison = 3, 33, 65, 8, 4, -12345.5
    taps = tuple(_quantised(t, dtype) for t in random_bank(flen, 5))
    arrs = [_engine._taps_array(t) for t in taps]
    gen = torch.Generator().manual_seed(77)
    lib, did = st._swt2_entries(), _engine._DTYPE_IDS[dtype]
    hh, ww = h + 4, w + 11
    for direction, nout in (("fwd", 4), ("inv", 1)):
        block = torch.full((nout * b + 2, hh, ww), poison, dtype=dtype, device=dev())
        inside = torch.zeros_like(block, dtype=torch.bool)
        planes = [block[1 + q * b:1 + (q + 1) * b, 2:2 + h, 5:5 + w] for q in range(nout)]
        for q in range(nout):
            inside[1 + q * b:1 + (q + 1) * b, 2:2 + h, 5:5 + w] = True
        ins = [torch.randn(b, h, w, generator=gen, dtype=torch.float64).to(dtype).to(dev()) for _ in range(5 - nout)]
        host = [t.double().cpu().numpy() for t in ins]
        ptrs = st._vp4(*([p.data_ptr() for p in planes] if nout == 4 else [t.data_ptr() for t in ins]))
        i_s, r_s = (hh * ww, ww) if nout == 4 else (h * w, w)
        if direction == "fwd":
            rc = lib.mifwt_swt2_fwd(did, flen, b, h, w, dilation, ins[0].data_ptr(), h * w, w, ptrs, st._i64x4(*[i_s] * 4),
                                    st._i64x4(*[r_s] * 4), *arrs, 1.0, ctypes.c_void_p(_engine._stream_of(block)))
            want = list(R2.level_fwd(host[0], taps, dilation, 1.0))
        else:
            rc = lib.mifwt_swt2_inv(did, flen, b, h, w, dilation, ptrs, st._i64x4(*[i_s] * 4), st._i64x4(*[r_s] * 4),
                                    planes[0].data_ptr(), hh * ww, ww, *arrs, 0.25, ctypes.c_void_p(_engine._stream_of(block)))
            want = [R2.level_inv(host, taps, dilation, 0.25)]
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((block[~inside] == poison).all()), (direction, "a guard element was overwritten")
        for q in range(nout):
            _check(planes[q], want[q], VALUE_TOL[dtype], ("guarded", direction, _name(dtype), q))


def test_capture_replays_bit_identically():
    x = torch.randn(3, 48, 80, generator=torch.Generator().manual_seed(8)).to(dev())
    fwd = ptwt_amd.capture(lambda t: ptwt_amd.swt2(t, "db4", level=2), x)
    x2 = torch.randn(3, 48, 80, generator=torch.Generator().manual_seed(9)).to(dev())
    eager = _flat(ptwt_amd.swt2(x2, "db4", level=2))
    n_f = _engine.launch_count(st.KID_SWT2)
    replay = _flat(fwd(x2))
    torch.cuda.synchronize()
    assert _engine.launch_count(st.KID_SWT2) == n_f  # a replay enqueues nothing through the C ABI
    assert all(torch.equal(a, b) for a, b in zip(replay, eager)) and len(replay) == len(eager) == 7
    stacked = torch.stack(eager)
    inv = ptwt_amd.capture(lambda t: ptwt_amd.iswt2(_nest(list(t.unbind(0))), "db4"), stacked)
    other = torch.stack(_flat(ptwt_amd.swt2(x, "db4", level=2)))
    eager_y = ptwt_amd.iswt2(_nest(list(other.unbind(0))), "db4")
    assert torch.equal(inv(other), eager_y)
    _check(eager_y, x, VALUE_TOL[torch.float32], "captured round trip")


def test_no_cell_was_skipped():
    """Runs last (file order): the share of skipped cells is zero."""
    assert COUNTS["cells"] >= 2 * len(CELLS) + 2 * len(API_CASES), "run the whole module"
    assert COUNTS["skipped"] == 0, COUNTS
    print("\nworst norm-wise errors vs the float64 references:", {k: "%.2e" % v for k, v in sorted(WORST.items())})


if __name__ == "__main__":
    measure_reference_f32()
