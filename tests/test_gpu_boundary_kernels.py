"""GPU tests (``-m gpu``) of the boundary-wavelet kernels (csrc/mifwt_bwt.hip: the fused kernels 26 / 27 and the generic per-axis
passes 28 / 29) against the float64 level operators built on the host, at the extents the tile geometry makes interesting.

The reference of every comparison is tests/_boundary_ref.py: ``ptwt_amd._boundary.level_coo`` (numpy, float64, never a kernel)
applied with torch on the CPU in float64, sparse for rows and dense for planes; tests/test_boundary_host.py pins it to the reference
library's goldens at L = 2 .. 20 and at mid sizes.

1. Single level calls: ``_bwt.rows_level`` / ``_bwt.transposed_level`` with banks from ``_bwt.bank`` against the operator applied to
   the same, already quantised, inputs.  Every fused length 2 .. 20 in float32 and float64 (the fused kernel id must have run) and the
   generic lengths 22, 34, 76, 128 (the generic id must have run); banks of four INDEPENDENT random filters scaled by 1 / sqrt(L) (for
   a pywt bank hi is the alternating flip of lo and, for orthogonal ones, synthesis is analysis transposed: a kernel that reads the
   wrong filter of a pair or the wrong band's table row can still give the expected numbers), used as "analysis" and as "synthesis"
   banks, and the pywt banks db7, db9, sym7, coif3, bior4.4, rbio2.4.  1-D coefficient counts M around the tile width T of the kernel
   under test (TILE1 below): L - 1, T - 1, T, T + 1, T + NB, T + NB + 1 (a last tile of boundary rows only), T + L/2 + 2 (either side of
   the synthesis kernels' edge condition) and 2 T + 3, each with n = 2 M and with n = 2 M - 1 under the five odd-extent modes.  2-D planes
   with a seam on each axis in turn and on both, ragged and exact last tiles, a last tile of boundary rows only, M = L - 1 next to a
   wide axis, odd extents on either axis and on both under every mode.  Batches of 1 and 3 and one cell of a few hundred per kernel.
   Layouts: contiguous; a column slice of a wider tensor at an odd element offset (misaligned: the scalar path); a row stride that is
   not a multiple of the 16-byte width; a batch slice; for synthesis the planes of one level buffer, separate tensors with different
   strides (the copying branch of ``transposed_level``) and detail bands at misaligned addresses.  Synthesis inputs are random
   coefficient sets, not images of an analysis.  One generic cell per direction and dtype has more outputs than the 8192 x 256 threads
   of the largest grid, so that the grid-stride loop takes a second trip.
2. The public classes at real sizes: MatrixWavedec / MatrixWaverec db5 level 10 on 32 x 1 000 000 and MatrixWavedec2 / MatrixWaverec2
   db4 level 3 on 64 x 1024 x 1024 — the float32 run against the library's float64 run over the whole batch, and rows 0, 17, 31 /
   images 0, 29, 63 of both against the CPU operators; 4 x 1001 x 999 level 3 (bior4.4, 10 taps, and db9, 18 taps) and 3 x 40961
   level 5 under every ``odd_coeff_padding_mode``, and 8 x 512 x 768, with the data gradient through the analysis and the coefficient-
   leaf gradients through the synthesis (cosine weights) against torch autograd over the CPU operators.  Synthesis is fed random
   coefficients as well as the analysis output.  For the biorthogonal bank the synthesis is not the inverse of the analysis; the target
   of every synthesis here is the CPU synthesis operator on the same coefficients, never the input.

Bounds, norm-wise per output plane plus a max-abs companion of 10 x bound x the largest value: float64 1e-12 (values) / 1e-11
(gradients) — the figures of test_gpu_boundary.py; float32 values 1e-6 per level call and 2e-6 for the multi-level
classes.  For a fused float32 level cell the operator's entries (taps and table rows) are rounded to float32 first, as the kernels
hold them; the generic pass holds them, and accumulates, in double.  The float32 GRADIENT bounds come from the reference alone:
``python -m tests.test_gpu_boundary_kernels`` runs the CPU operators in float32 over GRAD_CELLS and prints their worst norm-wise
errors against their own float64 run, and each bound is ten times its figure, because the GPU reduces in another order:
  data gradient (through the analysis)                      1.16e-7 (3 x 40961, db9)        F32_GRAD_X_TOL = 1.16e-6
  coefficient-leaf gradients (through the synthesis), plane 1.73e-5 (3 x 40961, db9)        F32_GRAD_C_TOL = 1.73e-4
  the same, all planes of a case taken as one vector         2.15e-7 (4 x 1001 x 999, db9)   F32_GRAD_C_ALL_TOL = 2.15e-6
The per-plane figure of the coefficient gradients is that large because the gradient of a detail plane is the high-pass analysis of
the smooth cosine weight, which cancels to 1e-5 .. 1e-7 of its terms (nine vanishing moments for db9); measured against all planes of
the case together the same run is at 2e-7, and that bound is the one with teeth.

No cell is skipped: a cell whose reference raises must raise in the library too and is counted, and the last test fails on a non-zero
count of skipped cells and prints WORST.  The only cells that raise are the expected ones — "reflect" on an odd extent of one sample
(L = 2, M = L - 1 = 1), which the reference's reflection padding refuses; they are checked to raise ValueError on both sides and
counted as "raised", not as skipped.
"""
import json

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _boundary, _bwt, _engine
from ptwt_amd._wavelets import host_taps
from tests import _boundary_ref as BR
from tests import _golden as G

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = (F32, F64)
LEVEL_TOL = {F64: 1e-12, F32: 1e-6}
API_TOL = {F64: 1e-12, F32: 2e-6}
F64_GRAD_TOL = 1e-11
# 10 x the float32 reference's own worst gradient errors (module docstring; ``python -m tests.test_gpu_boundary_kernels`` prints them)
F32_GRAD_X_TOL = 1.16e-6      # d/dx through the analysis
F32_GRAD_C_TOL = 1.73e-4      # d/dcoefficient through the synthesis, per plane (the detail planes cancel)
F32_GRAD_C_ALL_TOL = 2.15e-6  # d/dcoefficient, all planes of a case as one vector
# worst norm-wise errors of the module on the MI355X, as its last test prints them.  EMPTY: the module has not run on the device yet
# (EXPERIMENTS.md part B); fill it from the first run's printout
WORST_ON_MI355X = {
}

# ---- tile geometry, in coefficients (csrc/mifwt_bwt.hip; E = 4 float32 / 2 float64 elements per 16-byte access) ----------------------
#   FwdTile: TC1 = 256 E (1-D), TR = 8 rows x TC = 16 E columns (2-D)
#   InvTile: TQ1 = 128 E (1-D), TQ = 16 rows x TQC = (L <= 12 ? 16 : 8) E columns (2-D)
# (tests/test_boundary_host.py reads this table against the source, without a GPU)
E = {F32: 4, F64: 2}
TILE1 = {("fwd", F32): 1024, ("fwd", F64): 512, ("inv", F32): 512, ("inv", F64): 256}
GENERIC_GRID = 8192 * 256  # threads of the largest grid of bwt_axis_generic


def tile2(direction, dtype, flen):
    if direction == "fwd":
        return 8, 16 * E[dtype]
    return 16, (16 if flen <= 12 else 8) * E[dtype]


FUSED = list(range(2, 21, 2))
GENERIC = [22, 34, 76, 128]
PYWT_BANKS = ("db7", "db9", "sym7", "coif3", "bior4.4", "rbio2.4")
WORST = {}
COUNTS = {"cells": 0, "skipped": 0, "raised": 0}


def dev():
    return torch.device("cuda:0")


def tag(dtype):
    return str(dtype).split(".")[-1]


def weight(t, i):
    return torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64, device=t.device) + i).reshape(t.shape).to(t.dtype)


def random_bank(flen, seed=0):
    """Four independent filters scaled by 1 / sqrt(L) as (dec_lo, dec_hi, rec_lo, rec_hi)."""
    g = np.random.default_rng(7000 + 131 * seed + flen)
    return tuple(tuple(float(v) for v in g.standard_normal(flen) / np.sqrt(flen)) for _ in range(4))


def _note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), float(err))


def _check(got, want, tol, what, key=None):
    """Norm-wise error below ``tol`` and max-abs error below 10 x tol x the largest value; evaluated where ``got`` lives."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    got = got.detach().double()
    want = want.detach().double().to(got.device)
    den = float(torch.linalg.vector_norm(want))
    num = float(torch.linalg.vector_norm(got - want))
    err = num / den if den > 0 else num
    if key is not None:
        _note(key, err)
    assert err < tol, (what, err)
    if want.numel():
        assert float((got - want).abs().max()) <= 10 * tol * max(float(want.abs().max()), 1e-30), (what, "max-abs")
    return err


# ---- 1. single level calls -----------------------------------------------------------------------------------------------------------
SIG_LAYOUTS = ("contiguous", "colslice", "rowstride", "batchslice")
BAND_LAYOUTS = ("contiguous", "planes", "mixed", "misaligned")


def _rnd(gen, dtype, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype).to(dev())


def _signal(gen, dtype, batch, sig, layout):
    """x [batch, *sig] with contiguous samples: dense; a column slice of a wider tensor (row stride n + 7, odd element offset 3: a
    misaligned base); rows of a wider tensor from its first column on (aligned base, row stride = 1 mod 4 elements); every other
    entry of a longer batch, from the second one on."""
    n = sig[-1]
    if layout == "contiguous":
        return _rnd(gen, dtype, batch, *sig)
    if layout == "colslice":
        return _rnd(gen, dtype, batch, *sig[:-1], n + 7)[..., 3:3 + n]
    if layout == "rowstride":
        return _rnd(gen, dtype, batch, *sig[:-1], n + ((1 - n) % 4 or 4))[..., :n]
    assert layout == "batchslice"
    return _rnd(gen, dtype, 2 * batch + 1, *sig)[1::2]


def _bands(gen, dtype, batch, coef, layout):
    """The 2^d bands [batch, *coef]: separate dense tensors; the planes of one level buffer; tensors with different strides (dense, a
    column slice, a plane of a buffer); the detail bands one element into wider tensors of one width (equal strides, so they reach
    the kernel as they are, at misaligned addresses)."""
    nb, m = 1 << len(coef), coef[-1]
    if layout == "contiguous":
        return [_rnd(gen, dtype, batch, *coef) for _ in range(nb)]
    if layout == "planes":
        buf = _rnd(gen, dtype, batch, nb, *coef)
        return [buf[:, s] for s in range(nb)]
    if layout == "mixed":
        out = [_rnd(gen, dtype, batch, *coef), _rnd(gen, dtype, batch, *coef[:-1], m + 6)[..., 2:2 + m]]
        if nb == 4:
            out = [out[0], _rnd(gen, dtype, batch, *coef), out[1], _rnd(gen, dtype, batch, 3, *coef)[:, 1]]
            assert len({t.stride() for t in out[1:]}) == 3
        return out
    assert layout == "misaligned"
    return [_rnd(gen, dtype, batch, *coef)] + [_rnd(gen, dtype, batch, *coef[:-1], m + 4)[..., 1:1 + m] for _ in range(nb - 1)]


def _cell_name(direction, dtype, flen, sig, batch, mode, layout, which, bank_name):
    return "%s-%s-L%d-n%s-B%d-%s-%s-%s-%s" % (direction, tag(dtype), flen, "x".join(map(str, sig)), batch, mode, layout, which, bank_name)


def _run_level(direction, dtype, taps, which, sig, batch, mode, layout, bank_name="random", fused=True):
    """One cell: ``rows_level`` (direction "fwd") or ``transposed_level`` ("inv") against the float64 operator."""
    flen, ndim = len(taps[0]), len(sig)
    name = _cell_name(direction, dtype, flen, sig, batch, mode, layout, which, bank_name)
    gen = torch.Generator().manual_seed(flen * 100003 + 17 * sum(sig) + batch)
    bk = _bwt.bank(taps, "gramschmidt", which)
    coef = [(n + 1) // 2 for n in sig]
    kw = {"round32": dtype == F32 and fused}
    if direction == "fwd":
        ops = [_signal(gen, dtype, batch, sig, layout)]
        assert tuple(ops[0].shape) == (batch, *sig) and ops[0].stride(-1) == 1

        def call():
            return _bwt.rows_level(ops[0], bk, _engine.MODE_IDS[mode])

        def reference():
            return BR.rows_level(ops[0].double().cpu(), taps, which, mode, **kw)
    else:
        ops = _bands(gen, dtype, batch, coef, layout)
        assert all(tuple(t.shape) == (batch, *coef) and t.stride(-1) == 1 for t in ops)

        def call():
            return _bwt.transposed_level(ops, bk, sig)

        def reference():
            return BR.transposed_level([t.double().cpu() for t in ops], taps, which, sig, **kw)
    keep = [t.clone() for t in ops]
    COUNTS["cells"] += 1
    if direction == "fwd" and mode == "reflect" and 1 in sig:
        # an odd extent of ONE sample (L = 2, M = L - 1) has nothing to reflect: the reference's padding refuses it, so must both sides
        with pytest.raises(ValueError):
            reference()
        with pytest.raises(ValueError):
            call()
        COUNTS["raised"] += 1
        return
    try:
        want = reference()
    except Exception:
        COUNTS["skipped"] += 1
        with pytest.raises(Exception):
            call()
            torch.cuda.synchronize()
        return
    assert want.dtype == torch.float64
    _engine.level_events = []
    try:
        got = call()
        kids = {e[1] for e in _engine.level_events}
    finally:
        _engine.level_events = None
    torch.cuda.synchronize()
    want_kid = (_bwt.KID_FWD if fused else _bwt.KID_AXIS_FWD) if direction == "fwd" else (_bwt.KID_INV if fused else _bwt.KID_AXIS_INV)
    assert kids == {want_kid}, (name, kids)
    assert got.dtype == dtype and got.is_contiguous(), name
    for a, b in zip(ops, keep):
        assert torch.equal(a, b), (name, "an input was modified")
    key = "level %s %dd %s %s" % (direction, ndim, "fused" if fused else "generic", tag(dtype))
    if direction == "fwd":
        assert tuple(got.shape) == (batch, 1 << ndim, *coef), name
        for s in range(1 << ndim):
            _check(got[:, s], want[:, s], LEVEL_TOL[dtype], (name, "band", s), key)
    else:
        assert tuple(got.shape) == (batch, *sig), name
        _check(got, want, LEVEL_TOL[dtype], name, key)


def counts_1d(direction, dtype, flen):
    """The 1-D coefficient counts of a fused length: around the tile width of the kernel under test."""
    t, nb = TILE1[(direction, dtype)], _boundary.boundary_rows(flen)[1]
    return sorted({flen - 1, t - 1, t, t + 1, t + nb, t + nb + 1, t + flen // 2 + 2, 2 * t + 3})


def extents(direction, m):
    """(n, mode) of a coefficient count: n = 2 M, and n = 2 M - 1 under each odd-extent mode (a synthesis has no mode)."""
    if direction == "inv":
        return [(2 * m, "zero"), (2 * m - 1, "zero")]
    return [(2 * m, "zero")] + [(2 * m - 1, mode) for mode in BR.MODES]


def planes(direction, dtype, flen):
    """The (M_r, M_c) pairs of a fused length, from the tile of the kernel under test."""
    tr, tc = tile2(direction, dtype, flen)
    nb, lo = _boundary.boundary_rows(flen)[1], flen - 1
    kr, kc = max(1, -(-(lo - nb) // tr)), max(1, -(-(lo - nb) // tc))
    return [
        (max(lo, 2 * tr + 3), max(lo, tc - 5)),          # a seam along the rows axis (one ragged column tile where L - 1 allows)
        (max(lo, tr - 3), max(lo, 2 * tc + 5)),          # seams along the columns axis
        (max(lo, 2 * tr + 3), max(lo, 2 * tc + 3)),      # both, ragged last tiles on both axes
        (max(lo, 2 * tr), max(lo, 2 * tc)),              # both, whole tiles
        (kr * tr + nb, kc * tc + nb),                    # last tiles that hold boundary rows only, on both axes
        (lo, 3 * tc + 1),                                # the smallest fused extent next to a wide one
        (3 * tr + 1, lo),
    ]


ODD_AXES = ((1, 0), (0, 1), (1, 1))


def cells_2d(direction, dtype, flen):
    """(sig, mode) per plane: even x even everywhere; on the plane with seams on both axes every (mode, odd rows / columns / both);
    one of those combinations, rotating, on each of the other planes."""
    out = []
    modes = BR.MODES if direction == "fwd" else ("zero",)
    combos = [(mode, odd) for mode in modes for odd in ODD_AXES]
    for i, (mr, mc) in enumerate(planes(direction, dtype, flen)):
        out.append(((2 * mr, 2 * mc), "zero"))
        for mode, odd in (combos if i == 2 else [combos[(i + flen // 2) % len(combos)]]):
            out.append(((2 * mr - odd[0], 2 * mc - odd[1]), mode))
    return out


def _rotate(i, direction):
    """(batch, layout, bank direction) of the i-th cell of a test: periods 8, 4 and 3."""
    layouts = SIG_LAYOUTS if direction == "fwd" else BAND_LAYOUTS
    return (1, 3)[(i // 4) % 2], layouts[i % 4], ("analysis", "synthesis")[i % 3 == 1]


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("flen", FUSED)
@pytest.mark.parametrize("direction", ["fwd", "inv"])
def test_fused_1d_level_vs_float64_operator(direction, flen, dtype):
    taps = random_bank(flen)
    i = flen
    seen = set()
    for m in counts_1d(direction, dtype, flen):
        for n, mode in extents(direction, m):
            batch, layout, which = _rotate(i, direction)
            seen.add((batch, layout, which))
            _run_level(direction, dtype, taps, which, (n,), batch, mode, layout)
            i += 1
    assert {s[1] for s in seen} == set(SIG_LAYOUTS if direction == "fwd" else BAND_LAYOUTS) and {s[0] for s in seen} == {1, 3}
    assert {s[2] for s in seen} == {"analysis", "synthesis"}


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("flen", FUSED)
@pytest.mark.parametrize("direction", ["fwd", "inv"])
def test_fused_2d_level_vs_float64_operator(direction, flen, dtype):
    taps = random_bank(flen, 1)
    i = flen + 1
    seen = set()
    for sig, mode in cells_2d(direction, dtype, flen):
        batch, layout, which = _rotate(i, direction)
        seen.add((batch, layout, which))
        _run_level(direction, dtype, taps, which, sig, batch, mode, layout)
        i += 1
    assert {s[1] for s in seen} == set(SIG_LAYOUTS if direction == "fwd" else BAND_LAYOUTS) and {s[0] for s in seen} == {1, 3}


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("name", PYWT_BANKS)
@pytest.mark.parametrize("direction", ["fwd", "inv"])
def test_fused_level_with_pywt_banks(direction, name, dtype):
    """The pywt banks of the lengths the goldens miss (14, 18) and two biorthogonal ones, as "analysis" and as "synthesis" banks."""
    taps = host_taps(name)
    flen = len(taps[0])
    t1 = TILE1[(direction, dtype)]
    tr, tc = tile2(direction, dtype, flen)
    i = 0
    for which in ("analysis", "synthesis"):
        for m in (flen - 1, t1 + 1, 2 * t1 + 3):
            for n, mode in ((2 * m, "zero"), (2 * m - 1, BR.MODES[i % 5])):
                batch, layout, _ = _rotate(i, direction)
                _run_level(direction, dtype, taps, which, (n,), batch, mode, layout, bank_name=name)
                i += 1
        for sig in ((2 * (2 * tr + 3), 2 * (2 * tc + 3)), (2 * (2 * tr + 3) - 1, 2 * (2 * tc + 3) - 1), (2 * (flen - 1), 2 * (tc + 1) - 1)):
            batch, layout, _ = _rotate(i, direction)
            _run_level(direction, dtype, taps, which, sig, batch, BR.MODES[i % 5], layout, bank_name=name)
            i += 1


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("flen", GENERIC)
@pytest.mark.parametrize("direction", ["fwd", "inv"])
def test_generic_level_vs_float64_operator(direction, flen, dtype):
    """L > 20: one launch of ``bwt_axis_generic`` per axis (double taps, double accumulation: the operator is not rounded)."""
    taps = random_bank(flen, 2)
    i = flen // 2
    for m in (flen - 1, flen + 172, 1031):
        for n, mode in extents(direction, m):
            batch, layout, which = _rotate(i, direction)
            _run_level(direction, dtype, taps, which, (n,), batch, mode, layout, fused=False)
            i += 1
    lo = flen - 1
    for j, (mr, mc) in enumerate(((lo, lo + 40), (lo + 9, lo), (lo + 21, lo + 30))):
        for odd in ((0, 0), ODD_AXES[j]):
            batch, layout, which = _rotate(i, direction)
            _run_level(direction, dtype, taps, which, (2 * mr - odd[0], 2 * mc - odd[1]), batch, BR.MODES[i % 5], layout, fused=False)
            i += 1


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("direction", ["fwd", "inv"])
def test_generic_pass_second_trip_of_the_grid_stride_loop(direction, dtype):
    """5 x 1 000 000 at L = 22: 2.5 M analysis / 5 M synthesis outputs for a grid of 8192 x 256 threads."""
    batch, n, flen = 5, 1000000, 22
    assert batch * (n // 2) > GENERIC_GRID
    _run_level(direction, dtype, random_bank(flen, 3), "analysis", (n,), batch, "zero", "contiguous", fused=False)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("kernel", ["fwd1", "inv1", "fwd2", "inv2"])
def test_a_few_hundred_rows_or_planes_per_kernel(kernel, dtype):
    direction, ndim = kernel[:3], int(kernel[3])
    if ndim == 1:
        flen = 8
        _run_level(direction, dtype, random_bank(flen, 4), "analysis", (2 * (TILE1[(direction, dtype)] + 3) - 1,), 300, "symmetric", "contiguous")
    else:
        flen = 6
        tr, tc = tile2(direction, dtype, flen)
        _run_level(direction, dtype, random_bank(flen, 4), "synthesis", (2 * (tr + 3), 2 * (tc + 3) - 1), 200, "reflect", "contiguous")


def test_composed_passes_launch_in_the_documented_order():
    """The composed route is one loop over the axes: analysis runs the last axis first and doubles its planes per pass (1 + 2 + 4
    launches of pass 28), synthesis mirrors it (4 + 2 + 1 of pass 29).  The recorded (kernel id, extent) lists are pinned, and the
    values compared with the float64 operators."""
    fwd, inv = _bwt.KID_AXIS_FWD, _bwt.KID_AXIS_INV
    assert (fwd, inv) == (28, 29)
    cases = [
        (random_bank(22, 5), (50,), False, [(fwd, (50,))], [(inv, (50,))]),
        (random_bank(22, 5), (44, 50), False, [(fwd, (50,))] + [(fwd, (44,))] * 2, [(inv, (44,))] * 2 + [(inv, (50,))]),
        (random_bank(6, 5), (12, 14, 20), True, [(fwd, (20,))] + [(fwd, (14,))] * 2 + [(fwd, (12,))] * 4,
         [(inv, (12,))] * 4 + [(inv, (14,))] * 2 + [(inv, (20,))]),
    ]
    gen = torch.Generator().manual_seed(2024)

    def recorded(call):
        _engine.level_events = []
        try:
            out = call()
            events = [(e[1], e[2]) for e in _engine.level_events]
        finally:
            _engine.level_events = None
        torch.cuda.synchronize()
        return out, events

    for taps, sig, force, want_fwd, want_inv in cases:
        x = _rnd(gen, F32, 2, *sig)
        bands = [_rnd(gen, F32, 2, *(n // 2 for n in sig)) for _ in range(1 << len(sig))]
        keep = _bwt.FORCE_COMPOSED3
        _bwt.FORCE_COMPOSED3 = force
        try:
            got, events = recorded(lambda: _bwt.rows_level(x, _bwt.bank(taps, "gramschmidt", "analysis"), _engine.MODE_IDS["zero"]))
            assert events == want_fwd, (sig, events)
            rec, events = recorded(lambda: _bwt.transposed_level(bands, _bwt.bank(taps, "gramschmidt", "synthesis"), sig))
            assert events == want_inv, (sig, events)
        finally:
            _bwt.FORCE_COMPOSED3 = keep
        want = BR.rows_level(x.double().cpu(), taps, "analysis", "zero")
        for s in range(1 << len(sig)):
            _check(got[:, s], want[:, s], LEVEL_TOL[F32], ("composed fwd", sig, "band", s))
        _check(rec, BR.transposed_level([t.double().cpu() for t in bands], taps, "synthesis", sig), LEVEL_TOL[F32], ("composed inv", sig))


def test_the_cell_lists_cover_what_they_claim():
    """(no GPU work) the 1-D counts sit on both sides of the synthesis kernels' edge condition 2 (qc0 + T) + L + 2 >= 2 M and include
    a last tile of boundary rows only; the planes put seams on each axis alone and on both, for both tile shapes."""
    for dtype in DTYPES:
        for flen in FUSED:
            nt, nb = _boundary.boundary_rows(flen)
            for direction in ("fwd", "inv"):
                t = TILE1[(direction, dtype)]
                ms = counts_1d(direction, dtype, flen)
                assert ms[0] == flen - 1 and {t - 1, t, t + 1, 2 * t + 3} <= set(ms)
                assert any(2 * t + flen + 2 >= 2 * m > 2 * t for m in ms) and any(2 * t + flen + 2 < 2 * m for m in ms)
                if nb:
                    assert any(0 < m - t <= nb for m in ms)  # the last tile holds boundary rows only
                tr, tc = tile2(direction, dtype, flen)
                ps = planes(direction, dtype, flen)
                assert any(mr > tr and mc > tc for mr, mc in ps) and any(mr > tr and mc <= max(tc, flen - 1) for mr, mc in ps)
                assert any(mr == flen - 1 and mc > 2 * tc for mr, mc in ps) and any(mc == flen - 1 and mr > 2 * tr for mr, mc in ps)
                assert any(mr % tr and mc % tc for mr, mc in ps)
                cells = cells_2d(direction, dtype, flen)
                if direction == "fwd":
                    odd = {(mode, sig[0] % 2, sig[1] % 2) for sig, mode in cells if sig[0] % 2 or sig[1] % 2}
                    assert odd >= {(mode, *o) for mode in BR.MODES for o in ODD_AXES}
        assert tile2("inv", dtype, 12)[1] == 2 * tile2("inv", dtype, 14)[1]  # the narrower synthesis tile for L > 12


# ---- 2. the public classes at real sizes ----------------------------------------------------------------------------------------------
def classes(ndim):
    return (ptwt_amd.MatrixWavedec, ptwt_amd.MatrixWaverec) if ndim == 1 else (ptwt_amd.MatrixWavedec2, ptwt_amd.MatrixWaverec2)


def flat(coeffs):
    out = []
    for c in coeffs:
        out.extend(c if isinstance(c, tuple) else [c])
    return out


def rebuild(ndim, leaves):
    if ndim == 1:
        return list(leaves)
    return (leaves[0], *[ptwt_amd.WaveletDetailTuple2d(*leaves[i:i + 3]) for i in range(1, len(leaves), 3)])


def _big_case(ndim, shape, wavelet, level, subset, dtype):
    """The float32 run against the library's float64 run on the same float32 inputs over the whole batch (two instantiations
    cross-checked; skipped for the float64 run itself), and the entries ``subset`` of the batch against the CPU operators."""
    Dec, Rec = classes(ndim)
    taps = host_taps(wavelet)
    gen = torch.Generator(device=dev()).manual_seed(11)
    x = torch.randn(*shape, generator=gen, device=dev(), dtype=torch.float32).to(dtype)  # float32 values in either dtype
    key = "api %dd values %s" % (ndim, tag(dtype))
    tol = API_TOL[dtype]
    COUNTS["cells"] += 1
    c = flat(Dec(wavelet, level)(x))
    assert all(t.dtype == dtype for t in c)
    leaves = [torch.randn(t.shape, generator=gen, device=dev(), dtype=torch.float32).to(dtype) for t in c]
    y_own = Rec(wavelet)(rebuild(ndim, c))
    y_rnd = Rec(wavelet)(rebuild(ndim, leaves))
    assert y_own.shape == x.shape == y_rnd.shape and y_own.dtype == dtype
    if dtype == F32:
        c64 = flat(Dec(wavelet, level)(x.double()))
        for i, (a, b) in enumerate(zip(c, c64)):
            _check(a, b, tol, (wavelet, shape, "float32 vs float64 run, coefficient", i), "api %dd float32 vs float64 run" % ndim)
        del c64
        y64 = Rec(wavelet)(rebuild(ndim, [t.double() for t in leaves]))
        _check(y_rnd, y64, tol, (wavelet, shape, "float32 vs float64 run, synthesis"), "api %dd float32 vs float64 run" % ndim)
        del y64
    sel = torch.tensor(subset, device=dev())
    want_c = BR.wavedec(x[sel].double().cpu(), taps, level)
    assert len(want_c) == len(c)
    for i, (a, b) in enumerate(zip(c, want_c)):
        _check(a[sel], b, tol, (wavelet, shape, "coefficient", i), key)
    want_own = BR.waverec([t[sel].double().cpu() for t in c], taps, ndim)
    _check(y_own[sel], want_own, tol, (wavelet, shape, "synthesis of the analysis output"), key)
    want_rnd = BR.waverec([t[sel].double().cpu() for t in leaves], taps, ndim)
    _check(y_rnd[sel], want_rnd, tol, (wavelet, shape, "synthesis of random coefficients"), key)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_matrix_wavedec_db5_level_10_on_32_x_1000000(dtype):
    """The shape of README's timing.  CPU operators on rows 0, 17 and 31 (sparse, ten levels: seconds)."""
    _big_case(1, (32, 1000000), "db5", 10, [0, 17, 31], dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_matrix_wavedec2_db4_level_3_on_64_x_1024_x_1024(dtype):
    """CPU operators on images 0, 29 and 63 (dense 1024 x 1024 matrices)."""
    _big_case(2, (64, 1024, 1024), "db4", 3, [0, 29, 63], dtype)


# (name, ndim, shape, wavelet, level, modes)
GRAD_CASES = [
    ("4x1001x999-bior4.4", 2, (4, 1001, 999), "bior4.4", 3, BR.MODES),
    ("4x1001x999-db9", 2, (4, 1001, 999), "db9", 3, BR.MODES),
    ("3x40961-db5", 1, (3, 40961), "db5", 5, BR.MODES),
    ("3x40961-bior4.4", 1, (3, 40961), "bior4.4", 5, BR.MODES),
    ("3x40961-db9", 1, (3, 40961), "db9", 5, ("reflect",)),
    ("8x512x768-db4", 2, (8, 512, 768), "db4", 3, ("zero",)),
    ("8x512x768-bior4.4", 2, (8, 512, 768), "bior4.4", 3, ("zero",)),
]
GRAD_CELLS = [(c, mode) for c in GRAD_CASES for mode in c[5]]


def _grad_inputs(case, dtype):
    name, ndim, shape, wavelet, level, _ = case
    gen = torch.Generator().manual_seed(len(name) + shape[-1])
    x = torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype)
    shapes = [t.shape for t in BR.wavedec(torch.zeros(1, *shape[1:], dtype=torch.float64), host_taps(wavelet), level)]
    leaves = [torch.randn(shape[0], *s[1:], generator=gen, dtype=torch.float64).to(dtype) for s in shapes]
    return x, leaves


def _grad_run(dec, rec, x, leaves):
    """Coefficients, the synthesis of the given leaves, and the gradients of the cosine-weighted sums w.r.t. x and the leaves."""
    x = x.detach().requires_grad_(True)
    leaves = [t.detach().clone().requires_grad_(True) for t in leaves]
    c = dec(x)
    y = rec(leaves)
    loss = sum((weight(t, i) * t).sum() for i, t in enumerate(c)) + (weight(y, 7) * y).sum()
    grads = torch.autograd.grad(loss, [x] + leaves)
    return [t.detach() for t in c], y.detach(), grads[0], list(grads[1:])


def _reference_run(case, mode, x, leaves, **kw):
    taps = host_taps(case[3])
    return _grad_run(lambda t: BR.wavedec(t, taps, case[4], mode, **kw), lambda ls: BR.waverec(ls, taps, case[1], **kw), x, leaves)


def _joined(tensors):
    return torch.cat([t.reshape(-1) for t in tensors])


def measure_reference_f32():
    """The CPU operators in float32 against their own float64 run over GRAD_CELLS, on the same float32 inputs: the worst norm-wise
    errors of the values and of the gradients.  The F32_GRAD_* bounds are ten times the gradient figures this prints."""
    worst = {"values": 0.0, "data gradients": 0.0, "coefficient gradients": 0.0, "coefficient gradients, all planes as one": 0.0}
    for case, mode in GRAD_CELLS:
        x, leaves = _grad_inputs(case, F32)
        c64, y64, gx64, gl64 = _reference_run(case, mode, x.double(), [t.double() for t in leaves])
        c32, y32, gx32, gl32 = _reference_run(case, mode, x, leaves)
        assert gx32.dtype == F32
        e_v = max(G.relerr(a.numpy(), b.numpy()) for a, b in zip(c32 + [y32], c64 + [y64]))
        e_x = G.relerr(gx32.numpy(), gx64.numpy())
        e_c = max(G.relerr(a.numpy(), b.numpy()) for a, b in zip(gl32, gl64))
        e_j = G.relerr(_joined(gl32).numpy(), _joined(gl64).numpy())
        print("%-22s %-10s values %.2e  data gradients %.2e  coefficient gradients %.2e, as one %.2e" % (case[0], mode, e_v, e_x, e_c, e_j))
        for k, e in zip(worst, (e_v, e_x, e_c, e_j)):
            worst[k] = max(worst[k], e)
    print("worst:", {k: "%.2e" % v for k, v in worst.items()})
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("cell", GRAD_CELLS, ids=lambda c: "%s-%s" % (c[0][0], c[1]))
def test_classes_values_and_gradients_vs_cpu_operators(cell, dtype):
    case, mode = cell
    name, ndim, shape, wavelet, level, _ = case
    Dec, Rec = classes(ndim)
    x, leaves = _grad_inputs(case, dtype)
    COUNTS["cells"] += 1
    try:
        want = _reference_run(case, mode, x.double(), [t.double() for t in leaves])
    except Exception:
        COUNTS["skipped"] += 1
        with pytest.raises(Exception):
            Dec(wavelet, level, odd_coeff_padding_mode=mode)(x.to(dev()))
        return
    dec, rec = Dec(wavelet, level, odd_coeff_padding_mode=mode), Rec(wavelet)
    got = _grad_run(lambda t: flat(dec(t)), lambda ls: rec(rebuild(ndim, ls)), x.to(dev()), [t.to(dev()) for t in leaves])
    torch.cuda.synchronize()
    v_tol = API_TOL[dtype]
    x_tol, c_tol, all_tol = (F64_GRAD_TOL,) * 3 if dtype == F64 else (F32_GRAD_X_TOL, F32_GRAD_C_TOL, F32_GRAD_C_ALL_TOL)
    what = (name, mode, tag(dtype))
    assert len(got[0]) == len(want[0])
    for i, (a, b) in enumerate(zip(got[0], want[0])):
        assert a.dtype == dtype
        _check(a, b, v_tol, (*what, "coefficient", i), "api %dd values %s" % (ndim, tag(dtype)))
    _check(got[1], want[1], v_tol, (*what, "synthesis of random coefficients"), "api %dd values %s" % (ndim, tag(dtype)))
    _check(got[2], want[2], x_tol, (*what, "d/dx"), "api %dd data gradient %s" % (ndim, tag(dtype)))
    for i, (a, b) in enumerate(zip(got[3], want[3])):
        _check(a, b, c_tol, (*what, "d/dcoefficient", i), "api %dd coefficient gradients %s" % (ndim, tag(dtype)))
    _check(_joined(got[3]), _joined(want[3]), all_tol, (*what, "d/dcoefficient, all planes"), "api %dd coefficient gradients as one %s" % (ndim, tag(dtype)))
    # the synthesis of the library's own coefficients: the CPU synthesis operator on them (for bior4.4 that is S A x, not x)
    y_own = rec(rebuild(ndim, got[0]))
    want_own = BR.waverec([t.double().cpu() for t in got[0]], host_taps(wavelet), ndim)
    _check(y_own, want_own, v_tol, (*what, "synthesis of the analysis output"), "api %dd values %s" % (ndim, tag(dtype)))


def test_no_cell_was_skipped():
    """Runs last (file order): the share of skipped cells is zero."""
    least = sum(len(counts_1d(d, t, f)) * len(extents(d, 1)) + len(cells_2d(d, t, f)) for d in ("fwd", "inv") for t in DTYPES for f in FUSED)
    assert COUNTS["cells"] >= least + 2 * len(GRAD_CELLS) + 4, "run the whole module"
    assert COUNTS["skipped"] == 0, COUNTS
    assert 2 <= COUNTS["raised"] <= 16, COUNTS  # (float32 and float64: the 1-D cell L = 2, n = 1, "reflect", and 2-D ones with such an axis)
    print("\ncells:", COUNTS)
    print("worst norm-wise errors vs the float64 operators:", json.dumps({k: float("%.2g" % v) for k, v in sorted(WORST.items())}))


if __name__ == "__main__":
    measure_reference_f32()
