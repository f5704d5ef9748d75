"""GPU tests (``-m gpu``) of every padded-transform route with banks of four INDEPENDENT random filters: values, data gradients and
reconstructions of ``wavedec*`` / ``waverec*`` / ``fswavedec*`` / ``fswaverec*`` through the harness of tests/_grad_ref.py (the one of
tests/test_gpu_data_gradients.py), tensor by tensor against the float64 differentiable CPU reference on the same quantised inputs.

Why.  In an orthogonal bank ``rec = flip(dec)``, ``hi[k] = +-lo[L-1-k]``, ``sum lo^2 = 1`` and ``sum hi = 0``: a route that runs the
inverse where the adjoint is meant, takes ``rec_*`` for ``flip(dec_*)``, derives the high-pass from the low-pass or drops a flip is
right for every named wavelet the rest of the suite uses (tests/test_independent_banks_host.py pins that blind spot on the CPU).  Here
the four filters of a case are ``np.random.default_rng(6000 + seed).standard_normal(L) / sqrt(L)``, one draw per filter, handed over as
four tuples of floats; no perfect reconstruction exists and none is asserted.

The table.  ``ROWS`` lists one differentiable call per row: route (the kernel ids it is about), function, shape, filter length, mode,
level, dtype, routing options and the ids expected on the legs that are the row's point (``fwd``, ``inv``, ``fwd_adj`` = backward of the
analysis, ``inv_adj`` = backward of the synthesis; ``_engine.level_events`` is recorded per leg).  Per kernel every filter length it is
instantiated for (``KERNEL_CLAIMS``; the coverage test counts only rows that EXPECT the kernel on the leg), each with zero mode and one
mirrored mode, the other modes rotated through the lengths.  Routes that only calls without a graph take (two levels per launch
12 / 13, the wave-strip kernels 1 / 2 at their own threshold) and the float16 storage rows run values only (coefficients and
reconstruction); every other float32 / float64 row runs with gradients.  The lengths, from the kernels' instance lists: 16 / 22 take 2,
4, 6, 8 and, with ONE level per launch on planes whose plan has twelve waves (1000 columns), ten taps; the matrix-core kernels 11 / 23
every even length 18 .. 32; the tiles 7 / 8 every even length up to 16 plus 18, 20, 24, 32 in float32 (float64: up to 16, beyond that the
axis kernels 3 / 4); the wave strips 1 / 2 every even length up to 16; the chunked 1-D kernels 17 / 18 every even length up to 20, the
one-workgroup 1-D kernels 14 / 15 every even length up to 32 (a run-time loop); the bricks 2, 4, 6 (synthesis: 8 too); the walking
kernels 2 .. 10 (synthesis: up to 8); the small-plane kernels every even length up to 20.

Shapes.  Those of the modules that are known to reach each route, shrunk where the route still holds; the wave strips 1 / 2 serve
sixteen taps by themselves only from 2^21 samples a plane on (1 x 1024 x 2048, one case: it cannot be smaller) and are reached on
2 x 256 x 1030 / 2 x 257 x 1031 at every length with MIFWT_OPT_TILE_MODE 2 and MIFWT_OPT_PYRAMID_MODE 2.  Dense 3-D references of ten
and more taps stay on volumes of at most 2 x 23 x 37 x 141 samples (a 1000-tap float64 correlation per output).

Bounds.  None is chosen from a kernel's output.  float64: ``F64_BOUNDS`` of tests/test_gpu_data_gradients.py as they are.  float32:
that module's rule — ten times what the float32 run of the REFERENCE ITSELF deviates from its float64 run on the same quantised inputs,
per measure, the worst over every float32 row below.  ``python -m tests.test_gpu_independent_banks`` measures it on the CPU; it printed

    worst float32 reference deviation: norm 1.86e-06  maxabs 5.68e-06  border 1.21e-06

(``F32_REF`` below; the bounds are 10 x that: 1.86e-5 / 5.68e-5 / 1.21e-5.  The first two come from 2 x 70 x 90 with 102 taps, a dense
10404-tap float32 correlation per output of the reference, the third from 2 x 18 x 20 x 19 with 16 taps in 3-D, 4096 taps per output; the
1-D and short-filter 2-D rows deviate 1.2e-7 .. 4.5e-7 norm-wise, the next-worst rows 8.5e-7).  float16 storage: 5e-4 norm-wise per level against float64 on the float16-quantised inputs, the bound of the
float16 tests of tests/test_gpu_parity.py for the same kernels (output rounding 2.1e-4 plus one rounding of the intermediate image);
one level per row.  The worst errors of the MI355X run are in ``WORST_ON_MI355X`` (a record, not a bound) and in EXPERIMENTS.md.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, _wavelets
from tests import _grad_ref as D
from tests import test_gpu_data_gradients as G

pytestmark = pytest.mark.gpu

f16, f32, f64 = torch.float16, torch.float32, torch.float64
# worst deviation of the float32 reference from the float64 reference over the float32 rows of this module (see the docstring)
F32_REF = {"norm": 1.86e-06, "maxabs": 5.68e-06, "border": 1.21e-06}
F32_BOUNDS = {m: 10 * v for m, v in F32_REF.items()}
F64_BOUNDS = G.F64_BOUNDS
F16_BOUNDS = {"norm": 5e-4, "maxabs": math.inf, "border": math.inf}  # (tests/test_gpu_parity.py bounds the norm-wise error only)
BOUNDS = {f32: F32_BOUNDS, f64: F64_BOUNDS, f16: F16_BOUNDS}
# worst errors of this module on an MI355X (printed by its last test); a record, not a bound
WORST_ON_MI355X = {f32: {"norm": 7.00e-07, "maxabs": 2.75e-06, "border": 5.08e-07}, f64: {"norm": 2.11e-15, "maxabs": 5.28e-15, "border": 1.75e-15},
                   f16: {"norm": 3.15e-04}}
LEGS = D.LEGS
MODES5 = ("zero", "constant", "reflect", "periodic", "symmetric")
MIRRORED = ("reflect", "symmetric")
STRIPS = G.STRIPS
Case = D.Case
H = D.Harness(BOUNDS, count_raises=True)

Row = namedtuple("Row", "route case opts expect generic grads create_graph half any_of")


@functools.lru_cache(maxsize=None)
def bank(flen, seed):
    """Four independent filters of ``flen`` taps as tuples of floats (hashable: part of a case's key)."""
    rng = np.random.default_rng(6000 + seed)
    return tuple(tuple(float(v) for v in rng.standard_normal(flen) / np.sqrt(flen)) for _ in range(4))


def cells(lengths, modes=MODES5):
    """(length, mode) pairs of a route: zero mode and one mirrored mode at every length, the other modes the route serves rotated
    through the first lengths."""
    out = []
    extra = [m for m in modes if m not in ("zero",) + MIRRORED]
    for i, flen in enumerate(lengths):
        out += [(flen, m) for m in ("zero", MIRRORED[i % 2]) if m in modes]
        if i < len(extra):
            out.append((flen, extra[i]))
    return out


ROWS = []


def border_route_fits(fn, shape, flen, level, axes=None):
    """Whether every level's analysis adjoint takes synthesis kernel + border kernel: all transformed extents of at least 2 (L + 1)
    samples (adjoint_border_supported of csrc/mifwt_adjoint_border.hip); below that the generic adjoint passes serve the level."""
    ns = [shape[a] for a in D.norm_axes(fn, len(shape), axes)]
    for _ in range(level):
        if flen > 32 or any(n < 2 * (flen + 1) for n in ns):
            return False
        ns = [(n + flen - 1) // 2 for n in ns]
    return True


def row(route, fn, shape, flen, mode, level, dtype, seed, opts=(), expect=None, generic=(), grads=True, create_graph=False, half=False,
        any_of=None, axes=None):
    if grads and mode != "zero" and not border_route_fits(fn, shape, flen, level, axes) and "fwd_adj" not in generic:
        # (a level too small for the border route: its analysis adjoint is the generic passes, whatever the row expects elsewhere)
        generic = tuple(generic) + ("fwd_adj",)
        expect = {leg: k for leg, k in (expect or {}).items() if leg != "fwd_adj"}
    ROWS.append(Row(route, Case(fn, shape, bank(flen, seed), mode, level, dtype, axes, seed), tuple(opts), expect or {}, tuple(generic), grads,
                    create_graph, half, any_of or {}))


PYR1 = ((_engine.OPT_PYRAMID_MODE, 1),)
PYR3 = ((_engine.OPT_PYRAMID_MODE, 3),)
WALK4 = ((_engine.OPT_TILE_MODE, 4),)
NO_TILES = ((_engine.OPT_TILE_MODE, 2), (_engine.OPT_PYRAMID_MODE, 2))  # neither the tiles nor the one-level form of 16 / 22
FN2 = ("wavedec2", "fswavedec2")
TILES = {"fwd": {7}, "inv": {8}, "fwd_adj": {8}, "inv_adj": {7}}

# ---- streaming multi-level 2-D (16 / 22): zero mode backward = one 22 launch ---------------------------------------------------------------
for i, (flen, mode) in enumerate(cells((2, 4, 6, 8))):
    fwd = {7} if mode == "periodic" else {16}  # (the streaming analysis serves every mode but periodic; the reconstruction has no mode)
    row("16/22", FN2[i % 2], (2, 300, 520), flen, mode, 3, f32, 100 + i,
        expect={"fwd": fwd, "inv": {22}, "fwd_adj": {22} if mode == "zero" else {8}, "inv_adj": {16}})
for i, (flen, mode) in enumerate(cells((2, 4, 6, 8), ("zero",) + MIRRORED + ("constant",))):
    # odd extents at every level (203 -> 10x -> 5x, 307 -> 15x -> 7x): every crop of the reconstruction
    row("16/22", FN2[(i + 1) % 2], (2, 203, 307), flen, mode, 2, f32, 120 + i, PYR1,
        expect={"fwd": {16}, "inv": {22}, "fwd_adj": {22} if mode == "zero" else (), "inv_adj": {16}})
row("16/22", "wavedec2", (2, 300, 520), 8, "zero", 3, f32, 140, create_graph=True, expect={"fwd": {16}, "inv": {22}, "fwd_adj": {8}, "inv_adj": {7}})
row("16/22", "wavedec2", (2, 300, 520), 6, "symmetric", 3, f32, 141, create_graph=True, expect={"fwd": {16}, "inv": {22}, "fwd_adj": {8}, "inv_adj": {7}})

# ---- two levels per launch (12 / 13): calls without a graph only; the same rows again with gradients go level by level on the tiles ----
for i, (flen, mode) in enumerate(cells((2, 4, 6, 8))):
    for grads in (False, True):
        expect = TILES if grads else {"fwd": {7} if mode == "periodic" else {12}, "inv": {13}}
        row("12/13", FN2[i % 2], (5, 200, 300), flen, mode, 3, f32, 200 + i, grads=grads, expect=expect)

# ---- small-plane pyramid (20 / 21) -------------------------------------------------------------------------------------------------------
for i, (flen, mode) in enumerate(cells((2, 4, 6, 8, 10, 12, 14, 16, 18, 20))):
    shape, opts = (((16, 64, 64), ()), ((6, 95, 81), PYR3))[i % 2]
    row("20/21", FN2[(i // 2) % 2], shape, flen, mode, 3, f32, 300 + i, opts,
        expect={"fwd": {20}, "inv": {21}, "inv_adj": {20}, "fwd_adj": {21} if mode == "zero" else ()})

# ---- LDS tiles (7 / 8), float32 and float64 ---------------------------------------------------------------------------------------------
TILE_SHAPES = ((2, 64, 70), (1, 131, 67), (2, 45, 42))
for i, (flen, mode) in enumerate(cells((2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 24, 32))):
    shape = (2, 70, 90) if flen > 20 else ((2, 45, 42) if flen == 20 else TILE_SHAPES[i % 2])  # (the border route needs 2 (L + 1) samples)
    # (float32 planes of at most 10240 coefficients a band may reconstruct on the small-plane kernel 21; the wider plane below takes 8)
    row("7/8", FN2[i % 2], shape, flen, mode, 1, f32, 400 + i, expect={"fwd": {7}, "fwd_adj": {8}, "inv_adj": {7}}, any_of={"inv": {8, 21}})
for i, (flen, mode) in enumerate(cells((2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 24, 32))):
    row("7/8", "wavedec2", (1, 150, 302), flen, mode, 1, f32, 430 + i, expect=TILES)
for i, (flen, mode) in enumerate(cells((2, 4, 6, 8, 10, 12, 14, 16))):
    row("7/8", FN2[i % 2], (2, 90, 150), flen, mode, 1, f64, 460 + i, expect={"fwd": {7}, "inv": {8}, "fwd_adj": {8}, "inv_adj": {7}})
for i, (flen, mode) in enumerate(cells((18, 20, 24, 32))):  # float64 beyond 16 taps: the axis kernels
    row("3/4", "wavedec2", (2, 90, 150), flen, mode, 1, f64, 480 + i, expect={"fwd": {3}, "inv": {4}, "fwd_adj": {4}, "inv_adj": {3}})

# ---- one level of a wide plane: 16 / 22 with one level, the wave strips 1 / 2, both 2-D border kernels ------------------------------------
WIDE = ((2, 256, 1030), (2, 257, 1031))
for i, (flen, mode) in enumerate(cells((2, 4, 6, 8))):
    one = {"fwd": {16}, "inv": {22}, "fwd_adj": {22}, "inv_adj": {16}}  # (one level: the streaming analysis serves periodic mode too)
    row("16/22", "wavedec2", WIDE[i % 2], flen, mode, 1, f32, 500 + i, expect=one)
    if flen == 8 and mode != "zero":  # (eight taps: one thread group per border line; per sample under MIFWT_OPT_DEBUG 4096)
        row("16/22", "wavedec2", WIDE[i % 2], flen, mode, 1, f32, 500 + i, ((_engine.OPT_DEBUG, 4096),), expect=one)
# ten taps: one level per launch, on planes whose plan has twelve waves (1000 columns; 1030 columns take the tiles for the analysis)
for i, mode in enumerate(("zero", "reflect", "periodic", "symmetric", "constant")):
    row("16/22", FN2[i % 2], ((2, 256, 1000), (2, 257, 1001))[i % 2], 10, mode, 1, f32, 510 + i, expect={"fwd": {16}, "inv": {22}, "fwd_adj": {22}, "inv_adj": {16}})
row("16/22", "wavedec2", WIDE[0], 10, "zero", 1, f32, 520, expect={"fwd": {7}, "inv": {22}, "fwd_adj": {22}, "inv_adj": {7}})
row("16/22", "wavedec2", WIDE[1], 10, "reflect", 1, f32, 521, expect={"fwd": {7}, "inv": {22}, "fwd_adj": {22}, "inv_adj": {7}})
for i, (flen, mode) in enumerate(cells((2, 4, 6, 8, 10, 12, 14, 16))):
    row("1/2", FN2[i % 2], WIDE[i % 2], flen, mode, 1, f32, 540 + i, NO_TILES, expect={"fwd": {1}, "inv": {2}, "fwd_adj": {2}, "inv_adj": {1}})
row("1/2", "wavedec2", (1, 1024, 2048), 16, "reflect", 1, f32, 560, grads=False, expect={"fwd": {1}, "inv": {2}})

# ---- generic passes (0) --------------------------------------------------------------------------------------------------------------------
# (102 taps on 70 x 90: the reflect and periodic pads do not fit; those modes meet the route at 34 taps and on the rows)
for i, (fn, shape, flen, mode) in enumerate([("wavedec2", (2, 70, 90), 34, "zero"), ("wavedec2", (2, 70, 90), 34, "reflect"),
                                             ("fswavedec2", (2, 70, 90), 34, "periodic"), ("wavedec2", (2, 70, 90), 102, "zero"),
                                             ("wavedec2", (2, 70, 90), 102, "symmetric"), ("fswavedec2", (2, 70, 90), 102, "constant"),
                                             ("wavedec", (2, 513), 34, "zero"), ("wavedec", (2, 513), 34, "symmetric"),
                                             ("wavedec", (2, 513), 34, "constant"), ("wavedec", (2, 513), 102, "zero"),
                                             ("wavedec", (2, 513), 102, "reflect"), ("wavedec", (2, 513), 102, "periodic")]):
    row("0", fn, shape, flen, mode, 1, (f32, f64)[i % 2], 600 + i, generic=LEGS, expect={leg: {0} for leg in LEGS})

# ---- 1-D: rows 3 / 4, tails 14 / 15, long rows 17 / 18 (_AnalysisTail / _SynthesisChain1d) ------------------------------------------------
for i, (flen, mode) in enumerate(cells((2, 4, 6, 8, 10, 12, 14, 16, 18, 20, 24, 32))):
    row("3/4", "wavedec", (7, 999), flen, mode, 1, (f32, f64)[i % 2], 700 + i, expect={"fwd": {3}, "inv": {4}, "fwd_adj": {4}, "inv_adj": {3}})
LONG = {"fwd": {17}, "inv": {18}, "fwd_adj": {4}, "inv_adj": {17}}
TAIL = {"fwd": {14}, "inv": {15}, "fwd_adj": {4}, "inv_adj": {14}}
# (long rows: the chunked kernels 17 / 18 first — instantiated for every even length up to 20 —, whatever serves the deep levels after them)
for i, (flen, mode) in enumerate(cells(tuple(range(2, 21, 2)))):
    row("17/18", "wavedec", (3, 40001), flen, mode, 6, f32, 740 + i, expect=LONG)
for i, (flen, mode) in enumerate(cells((2, 4, 8, 10))):
    row("17/18", "wavedec", (5, 4097), flen, mode, 4, f32, 770 + i, expect=LONG)
# (one workgroup per row: many short rows; the taps are a run-time loop, every even length up to 32)
for i, (flen, mode) in enumerate(cells(tuple(range(2, 33, 2)))):
    if flen in (22, 26, 28, 30):  # (lengths the axis kernels 3 / 4 are not instantiated for: the per-level analysis adjoint is generic)
        row("14/15", "wavedec", (600, 700), flen, mode, 3, f32, 1200 + i, expect=dict(TAIL, fwd_adj={0}), generic=("fwd_adj",))
    else:
        row("14/15", "wavedec", (600, 700), flen, mode, 3, f32, 1200 + i, expect=TAIL)
row("14/15", "wavedec", (5, 4097), 32, "zero", 4, f32, 780, expect=TAIL)
row("14/15", "wavedec", (5, 4097), 32, "symmetric", 4, f32, 781, expect=TAIL)
for i, (flen, mode) in enumerate(cells((2, 8, 16, 32))):  # (float64: the tail analysis, the chunked or the tail synthesis)
    row("14/15", "wavedec", (2, 3001), flen, mode, 3, f64, 790 + i, expect={"fwd": {14}, "fwd_adj": {4}, "inv_adj": {14}}, any_of={"inv": {15, 18}})
for i, (flen, mode) in enumerate(cells((4, 10, 20))):
    row("14/15", "wavedec", (300, 700), flen, mode, 3, f64, 1250 + i, expect=TAIL)

# ---- 3-D bricks (9 / 10) ------------------------------------------------------------------------------------------------------------------
BRICKS = ((2, 24, 26, 31), (2, 18, 20, 19))
for i, (flen, mode) in enumerate(cells((2, 4, 6))):
    row("9/10", ("wavedec3", "fswavedec3")[i % 2], BRICKS[i % 2], flen, mode, 1, f32, 800 + i, expect={"fwd": {9}, "inv": {10}, "fwd_adj": {10}, "inv_adj": {9}})
for i, (flen, mode) in enumerate(cells((8,))):  # eight taps: the synthesis bricks under the composed analysis
    row("9/10", "wavedec3", BRICKS[i % 2], flen, mode, 1, f32, 820 + i, expect={"fwd": {5}, "inv": {10}, "fwd_adj": {10}, "inv_adj": {5}})

# ---- 3-D composed (5 / 6) ---------------------------------------------------------------------------------------------------------------
COMPOSED = {"fwd": {5}, "inv": {6}, "fwd_adj": {6}, "inv_adj": {5}}
for i, (flen, mode) in enumerate(cells((6, 8, 10))):
    row("5/6", "wavedec3", (1, 40, 33, 36), flen, mode, 1, f64, 840 + i, expect=COMPOSED)
for i, (flen, mode) in enumerate(cells((10, 12, 14, 16, 18, 20))):
    # (up to 14 taps 33 samples still take the border route; the dense reference of 16 taps stays on the smallest volume)
    row("5/6", "wavedec3", (1, 40, 33, 36) if flen <= 14 else BRICKS[1 if flen == 16 else 0], flen, mode, 1, f32, 860 + i, expect=COMPOSED)
for i, (flen, mode) in enumerate(cells((24, 32))):
    row("5/6", "wavedec3", (1, 40, 33, 36), flen, mode, 1, f32, 880 + i, expect=COMPOSED)

# ---- 3-D walk (24 / 25) under MIFWT_OPT_TILE_MODE 4: strip and slab form, float32 and float64 -----------------------------------------------
for i, (flen, mode) in enumerate(cells((2, 4, 6, 8, 10))):
    walk = {"fwd": {24}, "inv": {25} if flen <= 8 else {6}, "fwd_adj": {25} if flen <= 8 else {6}, "inv_adj": {24}}
    # (rows of 141 samples: the strip form; 23 planes: ten taps still take the border route)
    row("24/25", "wavedec3", (2, 21 if flen < 10 else 23, 37, 141), flen, mode, 1, f32, 900 + i, WALK4, expect=walk)
for i, (flen, mode) in enumerate(cells((8, 10), ("zero",) + MIRRORED)):
    shape = (2, 40, 44, 100) if flen == 8 else (3, 17, 23, 128)
    for opts in (WALK4, WALK4 + ((_engine.OPT_DEBUG, STRIPS),)):  # the slab form, and the strip form of the same case
        row("24/25", "wavedec3", shape, flen, mode, 1, f32, 920 + i, opts, expect={"fwd": {24}, "inv_adj": {24}})
row("24/25", "wavedec3", (3, 17, 23, 128), 8, "constant", 1, f32, 930, WALK4, expect={"fwd": {24}, "inv": {25}, "fwd_adj": {25}, "inv_adj": {24}})
row("24/25", "wavedec3", (3, 17, 23, 128), 8, "periodic", 1, f32, 931, WALK4, expect={"fwd": {24}, "inv": {25}, "fwd_adj": {25}, "inv_adj": {24}})
for i, (flen, mode) in enumerate(cells((2, 4, 6, 8))):
    row("24/25", "wavedec3", (2, 40, 41, 42), flen, mode, 1, f64, 940 + i, WALK4, expect={"fwd": {24}, "inv": {25}, "fwd_adj": {25}, "inv_adj": {24}})
row("24/25", "wavedec3", (2, 40, 41, 42), 10, "zero", 1, f64, 950, WALK4, expect={"fwd": {24}, "inv": {6}, "fwd_adj": {6}, "inv_adj": {24}})
row("24/25", "wavedec3", (2, 40, 41, 42), 10, "symmetric", 1, f64, 951, WALK4, expect={"fwd": {24}, "inv": {6}, "fwd_adj": {6}, "inv_adj": {24}})

# ---- float16 storage: matrix-core kernels 11 / 23 and the float16 tiles; values only --------------------------------------------------------
MFMA_SHAPES = {32: (2, 300, 420), 24: (2, 200, 260)}
for i, (flen, mode) in enumerate(cells((18, 20, 22, 24, 26, 28, 30, 32))):
    row("11/23", FN2[(i + 1) % 2], MFMA_SHAPES.get(flen, (3, 130, 170)), flen, mode, 1, f16, 1000 + i, grads=False, half=True, expect={"fwd": {11}, "inv": {23}})
for i, (flen, mode) in enumerate(cells((4, 8, 16))):
    row("7/8 f16", FN2[i % 2], (3, 130, 170), flen, mode, 1, f16, 1020 + i, grads=False, half=True, expect={"fwd": {7}, "inv": {8}})
for i, (flen, mode) in enumerate(cells((18, 20, 24, 32))):  # (MIFWT_OPT_MFMA_MODE 2: the vector tile kernel also for the long filters)
    row("7/8 f16", "wavedec2", (3, 130, 170), flen, mode, 1, f16, 1040 + i, ((_engine.OPT_MFMA_MODE, 2),), grads=False, half=True, expect={"fwd": {7}})

# ---- a non-default axes argument ----------------------------------------------------------------------------------------------------------
row("axes", "wavedec2", (2, 140, 3, 150), 6, "symmetric", 2, f32, 1100, axes=(1, 3))
row("axes", "wavedec", (3, 301, 5), 8, "reflect", 2, f64, 1101, axes=1)

# what the coverage test holds the table to.  Per kernel: (route, leg, kernel id, filter lengths) — at every length a zero-mode row and a
# mirrored-mode row that EXPECT that id on that leg (a row's label alone covers nothing); per route: the modes and dtypes it meets.
EVEN16, EVEN20, TILE_LENGTHS = tuple(range(2, 17, 2)), tuple(range(2, 21, 2)), tuple(range(2, 17, 2)) + (18, 20, 24, 32)
KERNEL_CLAIMS = [
    ("16/22", "fwd", 16, (2, 4, 6, 8, 10)), ("16/22", "inv", 22, (2, 4, 6, 8, 10)), ("16/22", "inv_adj", 16, (2, 4, 6, 8, 10)),
    ("16/22", "fwd_adj", 22, (2, 4, 6, 8, 10)),
    ("12/13", "fwd", 12, (2, 4, 6, 8)), ("12/13", "inv", 13, (2, 4, 6, 8)),
    ("20/21", "fwd", 20, EVEN20), ("20/21", "inv", 21, EVEN20), ("20/21", "inv_adj", 20, EVEN20), ("20/21", "fwd_adj", 21, EVEN20),
    ("7/8", "fwd", 7, TILE_LENGTHS), ("7/8", "inv", 8, TILE_LENGTHS), ("7/8", "fwd_adj", 8, TILE_LENGTHS), ("7/8", "inv_adj", 7, TILE_LENGTHS),
    ("1/2", "fwd", 1, EVEN16), ("1/2", "inv", 2, EVEN16), ("1/2", "fwd_adj", 2, EVEN16), ("1/2", "inv_adj", 1, EVEN16),
    ("0", "fwd", 0, (34, 102)), ("0", "inv", 0, (34, 102)), ("0", "fwd_adj", 0, (34, 102)), ("0", "inv_adj", 0, (34, 102)),
    ("3/4", "fwd", 3, EVEN20 + (24, 32)), ("3/4", "inv", 4, EVEN20 + (24, 32)), ("3/4", "fwd_adj", 4, EVEN20 + (24, 32)),
    ("3/4", "inv_adj", 3, EVEN20 + (24, 32)),
    ("14/15", "fwd", 14, tuple(range(2, 33, 2))), ("14/15", "inv", 15, tuple(range(2, 33, 2))), ("14/15", "inv_adj", 14, tuple(range(2, 33, 2))),
    ("17/18", "fwd", 17, EVEN20), ("17/18", "inv", 18, EVEN20), ("17/18", "inv_adj", 17, EVEN20),
    ("9/10", "fwd", 9, (2, 4, 6)), ("9/10", "inv", 10, (2, 4, 6, 8)), ("9/10", "fwd_adj", 10, (2, 4, 6, 8)), ("9/10", "inv_adj", 9, (2, 4, 6)),
    ("5/6", "fwd", 5, (6, 8, 10, 12, 14, 16, 18, 20, 24, 32)), ("5/6", "inv", 6, (6, 8, 10, 12, 14, 16, 18, 20, 24, 32)),
    ("5/6", "inv_adj", 5, (6, 8, 10, 12, 14, 16, 18, 20, 24, 32)), ("5/6", "fwd_adj", 6, (6, 8, 10, 12, 14)),
    ("24/25", "fwd", 24, (2, 4, 6, 8, 10)), ("24/25", "inv", 25, (2, 4, 6, 8)), ("24/25", "fwd_adj", 25, (2, 4, 6, 8)),
    ("24/25", "inv_adj", 24, (2, 4, 6, 8, 10)),
    ("11/23", "fwd", 11, tuple(range(18, 33, 2))), ("11/23", "inv", 23, tuple(range(18, 33, 2))),
    ("7/8 f16", "fwd", 7, (4, 8, 16, 18, 20, 24, 32)), ("7/8 f16", "inv", 8, (4, 8, 16)),
]
ROUTE_CLAIMS = {route: (MODES5, dtypes) for route, dtypes in (("16/22", (f32,)), ("12/13", (f32,)), ("20/21", (f32,)), ("7/8", (f32, f64)),
                                                              ("1/2", (f32,)), ("0", (f32, f64)), ("3/4", (f32, f64)), ("14/15", (f32, f64)),
                                                              ("17/18", (f32,)), ("9/10", (f32,)), ("5/6", (f32, f64)), ("24/25", (f32, f64)),
                                                              ("11/23", (f16,)), ("7/8 f16", (f16,)))}


def row_id(r):
    c = r.case
    tag = "-".join(f"{k}={v}" for k, v in r.opts)
    return "-".join(str(p) for p in (r.route, c.fn, "x".join(map(str, c.shape)), f"{len(c.wavelet[0])}taps", c.mode, f"L{c.level}",
                                     str(c.dtype).split(".")[-1], "grads" if r.grads else "values", "graph" if r.create_graph else "", tag) if p != "")


def run_row(r, **kw):
    scope = ptwt_amd.half_storage() if r.half else _null()
    with scope:
        ev, kids = H.run(r.case, r.opts, create_graph=r.create_graph, expect=r.expect, generic=r.generic, grads=r.grads, **kw)
    for leg, some in r.any_of.items():
        assert kids[leg] & set(some), (row_id(r), leg, "one of", some, "ran", ev[leg])
    return ev, kids


class _null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@pytest.mark.parametrize("r", ROWS, ids=row_id)
def test_route(r):
    """One row of the table: every tensor of the call against the float64 reference at the dtype's bounds, then the kernel ids of its
    legs."""
    run_row(r)


def test_the_table_covers_what_it_claims():
    """No GPU work: for every kernel of ``KERNEL_CLAIMS`` and every filter length listed there the table holds a zero-mode and a
    mirrored-mode row that expect that kernel on that leg (a backward leg: at least one row); every route meets every mode and both dtypes where it has both; both
    separable containers, a create_graph row on 16 / 22 and a non-default axes row occur; a row's key is unique."""
    keys = [(r.route, r.case, r.opts, r.grads, r.create_graph) for r in ROWS]
    assert len(keys) == len(set(keys))
    for route, leg, kid, lengths in KERNEL_CLAIMS:
        rows = [r for r in ROWS if r.route == route and kid in r.expect.get(leg, ())]
        for flen in lengths:
            seen = {r.case.mode for r in rows if len(r.case.wavelet[0]) == flen}
            # (a kernel serves a backward leg in the modes its route gives it — 21 / 22 after several levels in zero mode only, the
            # one-launch shortcut; the border kernels in the others — so a backward leg needs a row, a forward leg both kinds)
            assert seen and (leg.endswith("_adj") or ("zero" in seen and seen & set(MIRRORED))), (route, leg, kid, flen, seen)
    for route, (modes, dtypes) in ROUTE_CLAIMS.items():
        rows = [r for r in ROWS if r.route == route]
        assert {r.case.mode for r in rows} >= set(modes), (route, {r.case.mode for r in rows})
        assert {r.case.dtype for r in rows} == set(dtypes), (route, {r.case.dtype for r in rows})
    assert set(ROUTE_CLAIMS) | {"axes"} == {r.route for r in ROWS} and {c[0] for c in KERNEL_CLAIMS} == set(ROUTE_CLAIMS)
    for r in ROWS:
        flen = len(r.case.wavelet[0])
        assert all(len(f) == flen for f in r.case.wavelet) and len(set(r.case.wavelet)) == 4  # four filters, no two alike
        assert r.grads == (r.case.dtype != f16) or r.route in ("12/13", "1/2"), row_id(r)  # float32 / float64 rows run with gradients
        assert r.half == (r.case.dtype == f16)
    assert {"fswavedec2", "fswavedec3", "wavedec", "wavedec2", "wavedec3"} == {r.case.fn for r in ROWS}
    assert any(r.create_graph and r.route == "16/22" for r in ROWS) and any(r.case.axes is not None for r in ROWS)
    # the banks are what the docstring says, and independent: far from every relation of an orthogonal bank
    b = bank(8, 3)
    rng = np.random.default_rng(6003)
    assert b == tuple(tuple(float(v) for v in rng.standard_normal(8) / np.sqrt(8)) for _ in range(4))
    lo, hi, rlo, rhi = (np.array(f) for f in b)
    assert np.abs(rlo - lo[::-1]).max() > 0.05 and np.abs(rhi - hi[::-1]).max() > 0.05
    assert min(np.abs(hi - s * lo[::-1] * (-1.0) ** np.arange(8)).max() for s in (1, -1)) > 0.05


def test_device_resident_bank_takes_the_same_routes_bit_for_bit():
    """The bank as four CUDA tensors that require no gradient, device taps on "auto": read to the host once per call — the same fused ids
    on every leg and bit-identical tensors as with the tuples of floats (16 / 22 in zero mode, and the tiles with their border kernel)."""
    keep = _wavelets._device_taps_mode
    ptwt_amd.set_device_taps("auto")
    try:
        _device_bank_rows()
    finally:
        ptwt_amd.set_device_taps(keep)


def _device_bank_rows():
    for r in (next(r for r in ROWS if r.route == "16/22" and r.case.mode == "zero" and r.case.level == 3),
              next(r for r in ROWS if r.route == "7/8" and r.case.mode == "reflect" and r.case.dtype == f32)):
        ev_a, _ = run_row(r)
        a = H.last
        dev_bank = tuple(torch.tensor(f, dtype=torch.float64, device="cuda:0") for f in r.case.wavelet)
        ev_b, _ = run_row(r, bank=dev_bank)
        b = H.last
        assert [D.ids(ev_a, leg) for leg in LEGS] == [D.ids(ev_b, leg) for leg in LEGS], (ev_a, ev_b)
        for key in ("coeffs", "gleaves"):
            assert all(torch.equal(s, t) for s, t in zip(a[key], b[key])), (row_id(r), key)
        assert torch.equal(a["gx"], b["gx"]) and torch.equal(a["rec"], b["rec"]), row_id(r)


def test_routes_of_the_module():
    """Runs last (file order): the module as a whole reached every kernel id of the dispatcher on the forward and inverse legs, every
    backward id the closing test of tests/test_gpu_data_gradients.py lists, and the four border kernels; no row was skipped — no
    reference raised (a row whose reference raises must raise in the library too and is counted: the allowed share is zero)."""
    assert H.reached, "run the whole module"
    got = {leg: {k for l, k in H.reached if l == leg} for leg in LEGS + ("border",)}
    print("\n(leg, kernel id) pairs reached:", {leg: sorted(map(str, v)) for leg, v in got.items()})
    for dt in (f32, f64, f16):
        print(f"worst errors {dt}:", {k: f"{v:.3e}" for k, v in H.worst[dt].items()}, "bounds:", {k: f"{v:.3e}" for k, v in BOUNDS[dt].items()})
    assert not H.raised, ("rows whose reference raised: nothing was compared", H.raised)
    ran = set(H.ran)
    missing = [row_id(r) for r in ROWS if r.case not in ran]
    assert not missing, ("rows that did not run", missing)
    listed = f32_cases()
    assert not [c for c in H.f32_cases if c not in listed], "float32 cases the yardstick of the bounds does not cover"
    every = set(range(0, 19)) | set(range(20, 26))
    assert every <= got["fwd"] | got["inv"], sorted(every - (got["fwd"] | got["inv"]))
    want = {"fwd": {0, 1, 3, 5, 7, 9, 11, 12, 14, 16, 17, 20, 24}, "inv": {0, 2, 4, 6, 8, 10, 13, 15, 18, 21, 22, 23, 25},
            "fwd_adj": {0, 4, 6, 8, 10, 21, 22, 25}, "inv_adj": {3, 5, 7, 9, 14, 16, 17, 20, 24}}  # (the backward ids of test_gpu_data_gradients)
    for leg in LEGS:
        assert want[leg] <= got[leg], (leg, sorted(want[leg] - got[leg]))
    assert {"line", "sample", "1d", "3d"} <= got["border"], got["border"]


# ---- the float32 yardstick (CPU): python -m tests.test_gpu_independent_banks ---------------------------------------------------------------
def f32_cases():
    """Every float32 row of the table that runs with Gaussian cotangents, once (route variants of a case share its inputs)."""
    out = []
    for r in ROWS:
        if r.case.dtype == f32 and r.case not in out:
            out.append(r.case)
    return out


def measure_f32_reference(cases=None, verbose=True):
    """The worst deviation of the float32 reference from the float64 reference per measure over ``cases`` (default: every float32 row)."""
    worst = {m: 0.0 for m in D.MEASURES}
    for case in f32_cases() if cases is None else cases:
        got = D.reference_deviation(case.fn, case.shape, case.wavelet, case.mode, case.level, case.axes, case.seed)
        if verbose:
            print(case.fn, case.shape, D.describe(case.wavelet), *case[3:], {k: f"{v:.2e}" for k, v in got.items()}, flush=True)
        for k, v in got.items():
            worst[k] = max(worst[k], v)
    return worst


if __name__ == "__main__":
    w = measure_f32_reference()
    print("worst float32 reference deviation: " + "  ".join(f"{k} {v:.2e}" for k, v in w.items()))
    print("bounds (10 x): " + "  ".join(f"{k} {10 * v:.2e}" for k, v in w.items()))
