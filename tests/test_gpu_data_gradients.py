"""GPU tests (``-m gpu``) of the DATA gradients of every backward route — fixed taps (a wavelet name), gradients w.r.t. the signal and
w.r.t. the coefficients — element by element against the differentiable float64 CPU reference (oracle/torch_autograd_ref.py, pinned to
the reference library's gradient goldens by tests/test_torch_autograd_ref.py), at the shapes where the routed kernels run.

One case = one differentiable call through the harness of tests/_grad_ref.py (``Harness.run``, shared with
tests/test_gpu_independent_banks.py).  Compared tensor by tensor with ``R`` on the same inputs (quantised to the case's dtype, then
widened): the coefficients of ``fn(x)``; d/dx of ``sum_i <w_i, c_i>``; the reconstruction ``rec(leaves)``; the gradients of
``<v, rec(leaves)>`` w.r.t. every leaf.  ``w_i`` and ``v`` are seeded GAUSSIAN tensors (tests/_grad_ref.py says why).  Per tensor: shape
and dtype, the norm-wise error, the max-abs error over the largest reference value and — d/dx only — the norm-wise error of the BORDER
STRIP, the samples within ``L - 1 + N % 2`` of an edge of a transformed axis (the border kernels touch a few percent of the samples; the
whole-tensor norm dilutes them).

Bounds.  float64: 1e-11 norm-wise (the bound of test_gpu_autograd.test_gradients_vs_reference_autograd); the two other measures keep
the ratio to the norm-wise bound that the float32 bounds have.  float32: ten times what the float32 run of the REFERENCE ITSELF
(float32 inputs, float32 taps) deviates from its float64 run on the same quantised inputs, the worst over every float32 case of this
module — the factor of test_gpu_boundary_packets.py / test_gpu_swt_kernels.py: it allows for the kernels' other summation order and
nothing more.  ``python -m tests.test_gpu_data_gradients`` measures them on the CPU; it printed

    worst float32 reference deviation: norm 5.82e-07  maxabs 1.56e-06  border 4.09e-07

(F32_REF below; the bounds are 10 x that: 5.82e-6 / 1.56e-5 / 4.09e-6.  The first two come from 1 x 140 x 90 coif5, a dense 900-tap
correlation per output, the third from 2 x 40 x 44 x 100 db4 in 3-D; the 1-D and short-filter cases deviate 1.2e-7 .. 3.3e-7 norm-wise).  No bound was chosen by looking at a kernel's output; the worst
errors of the MI355X run are in EXPERIMENTS.md.

Routes.  ``_engine.level_events`` is recorded around the forward, the reconstruction and each backward separately; a case states the
kernel ids it expects on each of the four legs (``fwd``, ``inv``, ``fwd_adj`` = backward of the analysis, ``inv_adj`` = backward of the
synthesis) where the route is its point, no case may reach the generic passes (id 0) unless it says so, and the last test asserts what
the module as a whole reached.  The two 2-D border kernels (csrc/mifwt_adjoint_border.hip) have no id of their own: an analysis adjoint
with a boundary extension whose event carries a non-generic id — or the generic SYNTHESIS under it, 30 taps — has run one of them, which
one follows from the taps and MIFWT_OPT_DEBUG 4096 (border2_fits); the module records that per event.

Shapes moved from the issue's list: 1 x 40 x 33 x 36 db3 runs in float64 (float32 takes the bricks there; the composed route 5 / 6
serves float64 volumes below the walking kernels' threshold); the slab form of kernel 24 runs on 2 x 40 x 44 x 100 db4 under
MIFWT_OPT_TILE_MODE 4 (the default route takes it from 4 x 100^3 on).
"""
import numpy as np
import pytest
import torch

import ptwt_amd
from oracle import torch_autograd_ref as R
from ptwt_amd import _engine
from tests import _grad_ref as D

pytestmark = pytest.mark.gpu

f32, f64 = torch.float32, torch.float64
# worst deviation of the float32 reference from the float64 reference over the float32 cases of this module (see the docstring)
F32_REF = {"norm": 5.82e-07, "maxabs": 1.56e-06, "border": 4.09e-07}
F32_BOUNDS = {m: 10 * v for m, v in F32_REF.items()}
F64_BOUNDS = {m: 1e-11 * F32_REF[m] / F32_REF["norm"] for m in F32_REF}
BOUNDS = {f32: F32_BOUNDS, f64: F64_BOUNDS}
LEGS = D.LEGS
STRIPS = 2097152  # MIFWT_OPT_DEBUG routing bit: kernel 24 keeps its strip form for eight / ten taps
FN2 = ("wavedec2", "fswavedec2")
MODES5 = ("zero", "constant", "reflect", "periodic", "symmetric")
MODES4 = ("reflect", "symmetric", "periodic", "constant")
MODES_1D = ("zero", "reflect", "periodic", "symmetric")
SMALL_ODD = [("wavedec2", "zero"), ("wavedec2", "symmetric"), ("fswavedec2", "constant")]
WIDE = [(2, 256, 1030), (2, 257, 1031)]
TILE_SHAPES = [((3, 61, 128), "db2"), ((2, 64, 70), "db4"), ((1, 131, 67), "db3"), ((2, 45, 42), "db10"), ((1, 140, 90), "coif5"),
               ((70, 18, 19), "db4")]
ROWS = [((3, 5001), "db4", 5), ((2, 40000), "db5", 8), ((40, 1000), "db2", 4), ((2, 4097), "haar", 10)]
BRICK_SHAPES = [((2, 24, 26, 31), "db2"), ((2, 18, 20, 19), "haar")]

Case = D.Case

# the harness of tests/_grad_ref.py with this module's bounds; its state under the names the tests below (and the CPU companion) use
H = D.Harness(BOUNDS)
REACHED = H.reached  # (leg, kernel id) and ("border", "line" | "sample" | "1d" | "3d") of the whole module
WORST = H.worst  # worst error per dtype and measure
_REFS = H.refs  # case -> (inputs, float64 results): computed once per case, shared by its route variants
F32_CASES = H.f32_cases  # every float32 case that ran with Gaussian cotangents: f32_cases() must list them all
run, check, reference, recording = H.run, H.check, H.reference, H.recording
options, border_kernel, ids = D.options, D.border_kernel, D.ids


def dev():
    return torch.device("cuda:0")


# ---- 2-D float32: the streaming multi-level kernels 16 / 22 -----------------------------------------------------------------------------
@pytest.mark.parametrize("fn", FN2)
@pytest.mark.parametrize("mode", MODES5)
def test_streaming_three_levels(mode, fn):
    """4 x 600 x 520 db4 level 3: forward and reconstruction one launch each (16 / 22; periodic: the analysis goes per level); a plain
    backward — zero mode: ONE multi-level synthesis launch with the taps reversed, else the per-level adjoints with their border
    kernels; the synthesis backward ONE zero-mode analysis launch — and a backward under create_graph, which takes the per-level
    adjoints throughout."""
    case = Case(fn, (4, 600, 520), "db4", mode, 3, f32)
    fwd = {7} if mode == "periodic" else {16}
    ev, kids = run(case, expect={"fwd": fwd, "inv": {22}, "fwd_adj": {22} if mode == "zero" else {8}, "inv_adj": {16}})
    assert len(ev["fwd"]) == (3 if mode == "periodic" else 1) and len(ev["inv"]) == 1, ev
    assert kids["fwd"] == fwd, ev["fwd"]
    assert ids(ev, "inv_adj") == [("fwd", 16)], ev["inv_adj"]  # one zero-mode analysis launch
    if mode == "zero":
        assert ids(ev, "fwd_adj") == [("inv", 22)], ev["fwd_adj"]  # one multi-level synthesis launch
    else:
        assert ids(ev, "fwd_adj") == [("fwd_adj", 8)] * 3, ev["fwd_adj"]
    ev, _ = run(case, create_graph=True)
    assert ids(ev, "fwd_adj") == [("fwd_adj", 8)] * 3 and ids(ev, "inv_adj") == [("inv_adj", 7)] * 3, ev


@pytest.mark.parametrize("fn", FN2)
@pytest.mark.parametrize("mode", ["zero", "symmetric"])
def test_streaming_odd_extents_at_every_level(mode, fn):
    """3 x 403 x 611 db2 level 3 (403 -> 203 -> 103 -> 53, 611 -> 307 -> 155 -> 79: every crop of the reconstruction is exercised) on the
    streaming kernels wherever they can run (MIFWT_OPT_PYRAMID_MODE 1)."""
    case = Case(fn, (3, 403, 611), "db2", mode, 3, f32, seed=1)
    opts = ((_engine.OPT_PYRAMID_MODE, 1),)
    ev, _ = run(case, opts, expect={"fwd": {16}, "inv": {22}, "inv_adj": {16}, "fwd_adj": {22} if mode == "zero" else {8}})
    assert len(ev["fwd"]) == 1 and len(ev["inv"]) == 1 and ids(ev, "inv_adj") == [("fwd", 16)], ev
    if mode == "zero":
        assert ids(ev, "fwd_adj") == [("inv", 22)], ev["fwd_adj"]
    run(case, opts, create_graph=True)


def test_separable_synthesis_backward_falls_back_at_a_crop_of_more_than_one_sample():
    """fswaverec2 crops the running approximation to the next level's details by ANY amount; a crop of more than one sample is not a
    zero-mode analysis extent, so the one-launch synthesis backward must stop there: the two finest levels in one zero-mode analysis launch
    (kernel 16), the coarsest through its own adjoint level.  Hand-made leaves (no analysis yields them): db4, a level-3 approximation of
    80 x 70 whose 154 x 134 output is cropped to details of 150 x 131."""
    shapes = [(2, 80, 70)] * 4 + [(2, 150, 131)] * 3 + [(2, 294, 256)] * 3
    vals = [D.gaussian(s, 40 + i, f32) for i, s in enumerate(shapes)]
    keys = ("ad", "da", "dd")

    def build(ts):
        return (ts[0], dict(zip(keys, ts[1:4])), dict(zip(keys, ts[4:7])), dict(zip(keys, ts[7:10])))

    ref_leaves = [t.double().requires_grad_(True) for t in vals]
    want_y = R.fswaverec2(build(ref_leaves), "db4")
    v = D.gaussian(want_y.shape, 77, f32)
    want_g = torch.autograd.grad((v.double() * want_y).sum(), ref_leaves)
    leaves = [t.to(dev()).requires_grad_(True) for t in vals]
    ev = {}
    with recording(ev, "inv"):
        y = ptwt_amd.fswaverec2(build(leaves), "db4")
    with recording(ev, "inv_adj"):
        gl = torch.autograd.grad((v.to(dev()) * y).sum(), leaves)
    check(y, want_y.detach(), f32, "crop: reconstruction")
    for i, (a, b) in enumerate(zip(gl, want_g)):
        check(a, b, f32, ("crop: d/dleaf", i))
    assert ids(ev, "inv_adj") == [("fwd", 16), ("inv_adj", 7)], ev["inv_adj"]
    REACHED.update(("inv_adj", k) for _, k, _ in ev["inv_adj"])


# ---- 2-D float32: the small-plane kernels 20 / 21 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["zero", "reflect", "periodic"])
def test_small_planes_auto_route(mode):
    case = Case("wavedec2", (16, 64, 64), "db2", mode, 3, f32, seed=2)
    ev, _ = run(case, expect={"fwd": {20}, "inv": {21}, "inv_adj": {20}, "fwd_adj": {21} if mode == "zero" else {8}})
    assert len(ev["fwd"]) == 1 and len(ev["inv"]) == 1 and ids(ev, "inv_adj") == [("fwd", 20)], ev
    if mode == "zero":
        assert ids(ev, "fwd_adj") == [("inv", 21)], ev["fwd_adj"]
    ev, _ = run(case, create_graph=True)
    assert len(ev["fwd_adj"]) == 3 and len(ev["inv_adj"]) == 3, ev


@pytest.mark.parametrize("fn,mode", SMALL_ODD)
def test_small_planes_odd_extents(fn, mode):
    """6 x 95 x 81 db3 level 3 on the small-plane kernels wherever they can run (MIFWT_OPT_PYRAMID_MODE 3)."""
    case = Case(fn, (6, 95, 81), "db3", mode, 3, f32, seed=3)
    opts = ((_engine.OPT_PYRAMID_MODE, 3),)
    ev, _ = run(case, opts, expect={"fwd": {20}, "inv": {21}, "inv_adj": {20}, "fwd_adj": {21} if mode == "zero" else ()})
    assert len(ev["fwd"]) == 1 and len(ev["inv"]) == 1, ev


# ---- 2-D float32: one level through 16 / 22 and the two border kernels ------------------------------------------------------------------
ONE_LEVEL = {"expect": {"fwd": {16}, "inv": {22}, "fwd_adj": {22}, "inv_adj": {16}}}
TILES = {"expect": {"fwd": {7}, "inv": {8}, "fwd_adj": {8}, "inv_adj": {7}}}
# (float32 planes of at most 10240 coefficients a band reconstruct on the small-plane kernel, one level included)
TILES_SMALL = {f32: {"expect": {"fwd": {7}, "inv": {21}, "fwd_adj": {8}, "inv_adj": {7}}}, f64: TILES}


@pytest.mark.parametrize("shape", WIDE)
@pytest.mark.parametrize("wavelet", ["db2", "db4", "sym8"])
def test_one_level_of_a_wide_plane(wavelet, shape):
    """db2 / db4: the streaming kernels with one level; the analysis adjoint = kernel 22 + a border kernel (db2: one thread per sample,
    db4: one thread group per border line, and again per sample under MIFWT_OPT_DEBUG 4096).  sym8 (16 taps): tiles + the line kernel."""
    for mode in MODES4:
        case = Case("wavedec2", shape, wavelet, mode, 1, f32, seed=4)
        run(case, **(TILES if wavelet == "sym8" else ONE_LEVEL))
        if wavelet == "db4":
            run(case, ((_engine.OPT_DEBUG, 4096),), **ONE_LEVEL)


# ---- 2-D: tile adjoints 8 / 7 plus border, float32 and float64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [f32, f64])
@pytest.mark.parametrize("shape,wavelet", TILE_SHAPES)
def test_tile_adjoints_and_border(shape, wavelet, dtype):
    """One level on the LDS tiles (float32 reconstructions: the small-plane kernel 21; float64 db10: the axis kernels 3 / 4; coif5, 30
    taps: the generic passes, whose analysis adjoint still is synthesis + line kernel), every boundary mode; the per-sample border kernel
    again under MIFWT_OPT_DEBUG 4096."""
    for mode in MODES4 + ("zero",):
        case = Case("wavedec2", shape, wavelet, mode, 1, dtype, seed=5)
        if wavelet == "coif5":
            ev, kids = run(case, generic=LEGS)
            assert all(kids[leg] == {0} for leg in LEGS), ev
        elif wavelet == "db10" and dtype == f64:
            run(case)
        else:
            run(case, **TILES_SMALL[dtype])
        if mode == "symmetric" and D.filt_len(wavelet) >= 8:
            run(case, ((_engine.OPT_DEBUG, 4096),), generic=LEGS if wavelet == "coif5" else ())


def edge_shapes(wavelet):
    n = 2 * (D.filt_len(wavelet) + 1)
    return [(2, n, n), (2, n, n - 1), (2, n - 1, n)]


@pytest.mark.parametrize("dtype", [f32, f64])
@pytest.mark.parametrize("wavelet", ["db2", "db4"])
def test_edge_of_the_border_route(wavelet, dtype):
    """Extents of exactly 2 (L + 1): the border route; 2 (L + 1) - 1 on one axis: the generic adjoint passes (id 0), still right."""
    inside, *outside = edge_shapes(wavelet)
    for mode in MODES4:
        ev, kids = run(Case("wavedec2", inside, wavelet, mode, 1, dtype, seed=6), **TILES_SMALL[dtype])
        assert kids["fwd_adj"] == {8}, ev
        for shape in outside:
            ev, kids = run(Case("wavedec2", shape, wavelet, mode, 1, dtype, seed=6), generic=("fwd_adj",),
                           expect={"fwd": {7}, "inv_adj": {7}})
            assert kids["fwd_adj"] == {0}, ev


@pytest.mark.parametrize("shape,wavelet,level", [((2, 64, 70), "db4", 2), ((16, 64, 64), "db2", 3), ((2, 300, 520), "db4", 2)])
def test_float64_goes_level_by_level(shape, wavelet, level):
    """The fused routes are float32 only: a float64 pyramid is one launch per level on every leg."""
    for mode in ("zero", "reflect"):
        ev, kids = run(Case("wavedec2", shape, wavelet, mode, level, f64, seed=7))
        assert all(len(ev[leg]) == level for leg in LEGS), ev
        assert not (set().union(*kids.values()) & {12, 13, 16, 20, 21, 22}), ev


# ---- 1-D --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [f32, f64])
@pytest.mark.parametrize("shape,wavelet,level", ROWS)
def test_rows(shape, wavelet, level, dtype):
    """The multi-level 1-D launches (14 / 17 forward and on the plain synthesis backward, 15 / 18 on the reconstruction), and with every
    multi-level launch off (MIFWT_OPT_PAIR_MODE 2) the axis kernels 3 / 4 plus the 1-D border kernel."""
    for mode in MODES_1D:
        case = Case("wavedec", shape, wavelet, mode, level, dtype, seed=8)
        ev, kids = run(case, expect={"fwd_adj": {4}})
        assert kids["fwd"] & {14, 17} and kids["inv"] & {15, 18} and kids["inv_adj"] & {14, 17}, ev
        if mode in ("zero", "reflect"):
            ev, kids = run(case, ((_engine.OPT_PAIR_MODE, 2),), expect={"fwd": {3}, "inv": {4}, "fwd_adj": {4}, "inv_adj": {3}})
            assert all(len(ev[leg]) == level for leg in LEGS), ev


def test_rows_long_and_tail_kernels_both_ran():
    """(file order: after test_rows) float32 rows of 5001 / 40000 samples take the chunked kernels 17 / 18 first and the one-workgroup
    kernels 14 / 15 for the deep levels."""
    for leg, want in (("fwd", {14, 17}), ("inv", {15, 18}), ("inv_adj", {14, 17})):
        assert {(leg, k) for k in want} <= REACHED, (leg, sorted(REACHED))


# ---- batches over the 32768-image split of the border launch ------------------------------------------------------------------------------
def test_border_launch_split_1d():
    """33000 rows of 24 samples, db2 level 1 reflect: the 1-D border kernel in two launches (grid.y is 16 bits).  128 distinct rows,
    repeated; every GPU row against the reference of its source row."""
    run(Case("wavedec", (128, 24), "db2", "reflect", 1, f32, seed=9), rows=33000, expect={"fwd": {3}, "inv": {4}, "fwd_adj": {4}, "inv_adj": {3}})


def test_border_launch_split_2d():
    """32800 planes of 18 x 20, db4 level 1 symmetric: the line border kernel in two launches, and the per-sample one under
    MIFWT_OPT_DEBUG 4096."""
    case = Case("wavedec2", (128, 18, 20), "db4", "symmetric", 1, f32, seed=10)
    run(case, rows=32800, expect={"fwd_adj": {8}})  # (so many planes: forward and reconstruction on the small-plane kernels 20 / 21)
    run(case, ((_engine.OPT_DEBUG, 4096),), rows=32800, expect={"fwd_adj": {8}})


# ---- 3-D --------------------------------------------------------------------------------------------------------------------------------
BRICKS = {"expect": {"fwd": {9}, "inv": {10}, "fwd_adj": {10}, "inv_adj": {9}}}
WALK = {"expect": {"fwd": {24}, "inv": {25}, "fwd_adj": {25}, "inv_adj": {24}}}


@pytest.mark.parametrize("shape,wavelet", BRICK_SHAPES)
def test_bricks(shape, wavelet):
    for mode in ("zero", "reflect", "symmetric"):
        case = Case("wavedec3", shape, wavelet, mode, 1, f32, seed=11)
        run(case, **BRICKS)
        if mode == "reflect":  # the same small volume on the walking kernels wherever they can run
            run(case, ((_engine.OPT_TILE_MODE, 4),), **WALK)


def test_composed_route():
    for mode in ("zero", "symmetric", "periodic"):
        run(Case("wavedec3", (1, 40, 33, 36), "db3", mode, 1, f64, seed=12), expect={"fwd": {5}, "inv": {6}, "fwd_adj": {6}, "inv_adj": {5}})


def test_walking_kernels_float64():
    """2 x 40 x 41 x 42 db2 level 2: the first level on the walking kernels, the second on the composed route."""
    for mode in ("zero", "reflect", "constant"):
        run(Case("wavedec3", (2, 40, 41, 42), "db2", mode, 2, f64, seed=13),
            expect={"fwd": {24, 5}, "inv": {25, 6}, "fwd_adj": {25, 6}, "inv_adj": {24, 5}})


def test_walking_kernels_float32():
    """16 x 47^3 db3: the analysis (and the synthesis adjoint) on kernel 24, the synthesis side on the bricks."""
    for mode in ("zero", "symmetric"):
        run(Case("wavedec3", (16, 47, 47, 47), "db3", mode, 1, f32, seed=14), expect={"fwd": {24}, "inv": {10}, "fwd_adj": {10}, "inv_adj": {24}})


def test_walking_kernel_slab_form():
    """Eight taps on rows of 100 samples: kernel 24 in its slab form (MIFWT_OPT_TILE_MODE 4 selects the walking kernels on this small
    volume), and in its strip form (the MIFWT_OPT_DEBUG routing bit) against the same reference."""
    for mode in ("zero", "reflect"):
        case = Case("wavedec3", (2, 40, 44, 100), "db4", mode, 1, f32, seed=15)
        run(case, ((_engine.OPT_TILE_MODE, 4),), expect={"fwd": {24}, "inv_adj": {24}})
        run(case, ((_engine.OPT_TILE_MODE, 4), (_engine.OPT_DEBUG, STRIPS)), expect={"fwd": {24}, "inv_adj": {24}})


def test_separable_3d():
    for mode in ("reflect", "zero"):
        run(Case("fswavedec3", (2, 24, 26, 31), "db2", mode, 1, f32, seed=16), **BRICKS)


# ---- layout -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [Case("wavedec2", (2, 64, 70), "db4", "reflect", 1, f32, seed=5),
                                  Case("wavedec2", (4, 600, 520), "db4", "zero", 3, f32),
                                  Case("wavedec2", (4, 600, 520), "db4", "reflect", 3, f32),
                                  Case("wavedec3", (2, 24, 26, 31), "db2", "reflect", 1, f32, seed=11),
                                  Case("wavedec", (3, 5001), "db4", "reflect", 5, f32, seed=8)])
def test_transposed_input(case):
    """x as a transposed view: the first analysis level reads a signal whose innermost stride is not 1, which only the generic passes
    take; everything after it is on the case's usual kernels."""
    ev, kids = run(case, layout="transposed", generic=("fwd",))
    assert [k for _, k, _ in ev["fwd"]].count(0) == 1 and ev["fwd"][0][1] == 0, ev["fwd"]


def test_axes_arguments():
    run(Case("wavedec2", (2, 140, 3, 150), "db2", "symmetric", 2, f32, axes=(1, 3), seed=17))
    run(Case("wavedec2", (2, 40, 3, 44), "db2", "reflect", 2, f64, axes=(1, 3), seed=17))
    run(Case("wavedec", (3, 301, 5), "db3", "reflect", 2, f32, axes=1, seed=18))
    run(Case("wavedec", (3, 2000, 5), "db3", "zero", 4, f64, axes=1, seed=18))


LOSS_CASES = [Case("wavedec2", (4, 600, 520), "db4", "zero", 3, f32), Case("wavedec2", (4, 600, 520), "db4", "reflect", 3, f32),
              Case("wavedec2", (16, 64, 64), "db2", "zero", 3, f32, seed=2), Case("wavedec2", (2, 64, 70), "db4", "reflect", 1, f64, seed=5),
              Case("wavedec", (3, 5001), "db4", "reflect", 5, f32, seed=8), Case("wavedec3", (2, 24, 26, 31), "db2", "symmetric", 1, f32, seed=11)]


@pytest.mark.parametrize("case", LOSS_CASES)
def test_stride_zero_cotangents(case):
    """A loss ``sum_i c_i.sum()``: autograd hands the backward an expanded (stride-0) cotangent for every band."""
    run(case, loss="sum")


@pytest.mark.parametrize("case", LOSS_CASES)
def test_single_band_loss(case):
    """A loss that uses one detail band of one level: the other cotangents arrive as materialised zeros.  The finest level's last band and
    the coarsest level's first detail band."""
    nb = (1 << D.FNS[case.fn][1]) - 1
    run(case, loss=1 + nb * case.level - 1)
    run(case, loss=1)


@pytest.mark.parametrize("shape,wavelet,level", [((2, 256, 1030), "db4", 1), ((2, 64, 70), "db4", 1), ((16, 64, 64), "db2", 3),
                                                 ((4, 600, 520), "db4", 3)])
def test_leaves_that_are_views_of_one_level_buffer(shape, wavelet, level):
    """The coefficients of a level as planes of ONE buffer (what the analysis itself returns): the reconstruction reads strided bands and
    the gradient arrives per buffer."""
    case = Case("wavedec2", shape, wavelet, "reflect", level, f32, seed={1030: 4, 70: 5, 64: 2, 520: 0}[shape[-1]])
    inp, want = reference(case)
    lv = inp["leaves"]
    groups = [[0, 1, 2, 3]] + [[1 + 3 * l + j for j in range(3)] for l in range(1, level)]
    bufs = [torch.stack([lv[i] for i in g], 1).to(dev()).requires_grad_(True) for g in groups]
    planes = [b[:, j] for b in bufs for j in range(b.shape[1])]
    ev = {}
    with recording(ev, "inv"):
        y = ptwt_amd.waverec2(D.rebuild(inp["template"], planes), wavelet)
    with recording(ev, "inv_adj"):
        gb = torch.autograd.grad((inp["v"].to(dev()) * y).sum(), bufs)
    check(y, want["rec"], f32, ("views: reconstruction", shape))
    got = [g[:, j] for g in gb for j in range(g.shape[1])]
    for i, (a, b) in enumerate(zip(got, want["gleaves"])):
        check(a, b, f32, ("views: d/dleaf", shape, i))
    assert all(k != 0 for leg in ev for _, k, _ in ev[leg]), ev


# ---- packets ------------------------------------------------------------------------------------------------------------------------------
def _packet_reference(x, wavelet, mode, maxlevel, ndim):
    """The leaves of the packet tree from ``R.wavedec2`` / ``R.wavedec`` with ``level=1`` per node, in key-product order."""
    nodes = {"": x}
    for _ in range(maxlevel):
        nxt = {}
        for key, t in nodes.items():
            if ndim == 2:
                a, (h, v, d) = R.wavedec2(t, wavelet, mode=mode, level=1)
                nxt.update({key + "a": a, key + "h": h, key + "v": v, key + "d": d})
            else:
                a, d = R.wavedec(t, wavelet, mode=mode, level=1)
                nxt.update({key + "a": a, key + "d": d})
        nodes = nxt
    return nodes


@pytest.mark.parametrize("ndim,shape,wavelet,mode,maxlevel", [(2, (2, 64, 70), "db2", "symmetric", 2), (1, (3, 200), "db3", "reflect", 3)])
@pytest.mark.parametrize("dtype", [f32, f64])
def test_packet_trees(ndim, shape, wavelet, mode, maxlevel, dtype):
    """d/dx of a Gaussian-weighted loss over all leaves of WaveletPacket2D / WaveletPacket against the same tree built from level-1
    reference transforms."""
    x = D.gaussian(shape, 60 + ndim, dtype)
    xr = x.double().requires_grad_(True)
    ref = _packet_reference(xr, wavelet, mode, maxlevel, ndim)
    ws = {k: D.gaussian(t.shape, 70 + i, dtype) for i, (k, t) in enumerate(ref.items())}
    (want,) = torch.autograd.grad(sum((ws[k].double() * t).sum() for k, t in ref.items()), xr)
    xd = x.to(dev()).requires_grad_(True)
    tree = (ptwt_amd.WaveletPacket2D if ndim == 2 else ptwt_amd.WaveletPacket)(xd, wavelet, mode=mode, maxlevel=maxlevel)
    total = 0
    for k, t in ref.items():
        node = tree[k]
        check(node, t.detach(), dtype, ("packet node", ndim, k))
        total = total + (ws[k].to(dev()) * node).sum()
    (gx,) = torch.autograd.grad(total, xd)
    axes = tuple(range(1, 1 + ndim))
    check(gx, want, dtype, ("packet d/dx", ndim), mask=D.border_mask(shape, axes, D.filt_len(wavelet)))


# ---- routes of the module -----------------------------------------------------------------------------------------------------------------
def test_routes_of_the_module():
    """Runs last (file order): every kernel id of the lists below was reached on the leg it is listed for, and so were both 2-D border
    kernels (and the 1-D and 3-D one)."""
    assert REACHED, "run the whole module"
    want = {"fwd": {3, 5, 7, 9, 14, 16, 17, 20, 24}, "inv": {0, 4, 6, 8, 10, 15, 18, 21, 22, 25},
            "fwd_adj": {0, 4, 6, 8, 10, 21, 22, 25}, "inv_adj": {3, 5, 7, 9, 14, 16, 17, 20, 24}}
    got = {leg: {k for l, k in REACHED if l == leg} for leg in LEGS + ("border",)}
    print("\n(leg, kernel id) pairs reached:", {leg: sorted(map(str, v)) for leg, v in got.items()})
    for dt in (f32, f64):
        print(f"worst errors {dt}:", {k: f"{v:.3e}" for k, v in WORST[dt].items()}, "bounds:", {k: f"{v:.3e}" for k, v in BOUNDS[dt].items()})
    missing = [c for c in F32_CASES if c not in f32_cases()]
    assert not missing, ("float32 cases the yardstick of the bounds does not cover", missing)
    for leg in LEGS:
        assert want[leg] <= got[leg], (leg, sorted(want[leg] - got[leg]))
    assert {"line", "sample", "1d", "3d"} <= got["border"], got["border"]


# ---- the float32 yardstick (CPU): python -m tests.test_gpu_data_gradients ----------------------------------------------------------------
def f32_cases():
    """Every float32 case of the module with Gaussian cotangents (the parametrisations above, written out; test_routes_of_the_module
    asserts that no such case ran that is missing here).  The variants of a case — routing options, create_graph, layouts, the other
    losses — share its inputs and are not listed again; the hand-made leaves of the crop test and the packet trees are no chains of
    ``R`` calls and are left out."""
    c = [Case(fn, (4, 600, 520), "db4", m, 3, f32) for fn in FN2 for m in MODES5]
    c += [Case(fn, (3, 403, 611), "db2", m, 3, f32, seed=1) for fn in FN2 for m in ("zero", "symmetric")]
    c += [Case("wavedec2", (16, 64, 64), "db2", m, 3, f32, seed=2) for m in ("zero", "reflect", "periodic")]
    c += [Case(fn, (6, 95, 81), "db3", m, 3, f32, seed=3) for fn, m in SMALL_ODD]
    c += [Case("wavedec2", s, w, m, 1, f32, seed=4) for s in WIDE for w in ("db2", "db4", "sym8") for m in MODES4]
    c += [Case("wavedec2", s, w, m, 1, f32, seed=5) for s, w in TILE_SHAPES for m in MODES4 + ("zero",)]
    c += [Case("wavedec2", s, w, m, 1, f32, seed=6) for w in ("db2", "db4") for s in edge_shapes(w) for m in MODES4]
    c += [Case("wavedec", s, w, m, l, f32, seed=8) for s, w, l in ROWS for m in MODES_1D]
    c += [Case("wavedec", (128, 24), "db2", "reflect", 1, f32, seed=9), Case("wavedec2", (128, 18, 20), "db4", "symmetric", 1, f32, seed=10)]
    c += [Case("wavedec3", s, w, m, 1, f32, seed=11) for s, w in BRICK_SHAPES for m in ("zero", "reflect", "symmetric")]
    c += [Case("wavedec3", (16, 47, 47, 47), "db3", m, 1, f32, seed=14) for m in ("zero", "symmetric")]
    c += [Case("wavedec3", (2, 40, 44, 100), "db4", m, 1, f32, seed=15) for m in ("zero", "reflect")]
    c += [Case("fswavedec3", (2, 24, 26, 31), "db2", m, 1, f32, seed=16) for m in ("reflect", "zero")]
    c += [Case("wavedec2", (2, 140, 3, 150), "db2", "symmetric", 2, f32, axes=(1, 3), seed=17),
          Case("wavedec", (3, 301, 5), "db3", "reflect", 2, f32, axes=1, seed=18)]
    return c


def measure_f32_reference(cases=None, verbose=True):
    """The worst deviation of the float32 reference from the float64 reference per measure over ``cases``."""
    worst = {m: 0.0 for m in D.MEASURES}
    for case in f32_cases() if cases is None else cases:
        got = D.reference_deviation(case.fn, case.shape, case.wavelet, case.mode, case.level, case.axes, case.seed)
        if verbose:
            print(tuple(case), {k: f"{v:.2e}" for k, v in got.items()}, flush=True)
        for k, v in got.items():
            worst[k] = max(worst[k], v)
    return worst


if __name__ == "__main__":
    w = measure_f32_reference()
    print("worst float32 reference deviation: " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()))
    print("bounds (10 x): " + "  ".join(f"{k} {10 * v:.2e}" for k, v in w.items()))
