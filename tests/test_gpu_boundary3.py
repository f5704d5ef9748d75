"""GPU tests (``-m gpu``) of the 3-D boundary-wavelet levels (csrc/mifwt_bwt3.hip: the fused brick kernels 30 / 31; the composed route
through the per-axis passes 28 / 29; the dense route) and of MatrixWavedec3 / MatrixWaverec3, against the float64 level operators built
on the host and applied on the CPU (tests/_boundary3_ref.py, pinned to the reference library's goldens by tests/test_boundary3_host.py).

1. Single level calls, fused: ``_bwt.rows_level`` / ``_bwt.transposed_level`` with id 30 / 31 asserted through ``level_events`` (the
   routing table ``_bwt.COMPOSED3_CELLS`` emptied for these cells, so that every kernel instance is tested whatever it routes).  Every
   fused length (2, 4, 6, 8) in float32 and float64 with banks of four INDEPENDENT random filters scaled by 1 / sqrt(L), used as
   "analysis" and as "synthesis" banks (a pywt bank can hide a swapped filter or table row), plus db3 and bior2.2 (rbio2.4 has ten
   taps: outside the envelope).  With T the brick extent along the axis varied (``tile3`` below) and NB the bottom boundary rows, the
   coefficient extents M in {L-1, T-1, T, T+1, T+NB+1 (a last brick of boundary rows only; where NB > 0), 2T+3} on one axis at a time —
   those of them with M >= L-1, the shortest axis a fused level has — the other two axes at the smallest value >= L-1 that is no
   multiple of their brick extent; one cell with all three axes ragged.  Each with n = 2 M and with n = 2 M - 1 (the mode cycling
   through the five), and at the base extents n = 2 M - 1 under each of the five modes on each axis in turn and on all three together.
   Batches of 1 and 3; one cell of (2 TD + 3) x (2 TR + 3) x (2 TC + 3) coefficients x 9 volumes = 243 workgroups.  Layouts:
   contiguous; a width slice at an odd element offset (the scalar path); a row stride and a slice stride that are no multiples of 16
   bytes; a batch slice; for synthesis the eight planes of one level buffer, eight separate tensors with differing strides and detail
   bands at misaligned addresses.  Synthesis inputs are random coefficients, never the image of an analysis.
2. Composed and dense routes: L in {22, 34} and a fused-length cell with ``_bwt.FORCE_COMPOSED3`` on: ids {28} / {29}, seven launches
   per level call; db4 on 12 x 40 x 40: the dense route, no launch recorded.
3. The public classes: the goldens (float64 at 1e-12, float32 from the same inputs at API_TOL); 2 x 96 x 128 x 160 db2 level 3 and db4
   level 2 in both dtypes and 3 x 63 x 77 x 101 bior2.2 level 2 under every ``odd_coeff_padding_mode`` against the CPU chain;
   2 x 256^3 db2 level 3, the float32 run against the library's own float64 run.  Synthesis is fed random coefficients as well as the
   analysis output; the target of every synthesis is the CPU synthesis operator on the same coefficients, never the input.
4. Gradients on every 3 x 63 x 77 x 101 and 2 x 96 x 128 x 160 case of 3.: the data gradient through the analysis and the coefficient-leaf
   gradients through the synthesis (cosine weights) against torch autograd over the CPU chain.
5. ``ptwt_amd.capture`` of ``dec(x)`` and ``rec(dec(x))`` replays bit-identically; guard bytes around every allocation ``_bwt`` makes
   and around the input leave results bit-equal to ordinary allocations.

Bounds, norm-wise per output plane plus a max-abs companion of 10 x bound x the largest value: float64 1e-12 (values) / 1e-11
(gradients); float32 values 1e-6 per level call and 2e-6 for the multi-level classes, unless the CPU run below says otherwise.  For a fused float32 level cell
the operator's entries are rounded to float32 first, as the kernels hold them.  ``python -m tests.test_gpu_boundary3`` runs the CPU
chain in float32 against its own float64 run over the cells of 1. (largest extents of every fused length) and the cases of 3. / 4. and
prints the worst norm-wise figures.  Where a figure exceeds a tenth of the project's bound, the bound is ten times the figure (the
margin for the GPU's other summation order), per filter length for the level calls:
  level calls  an axis of ONE coefficient (L = 2 only)
                       1.40e-6  (analysis, 2 x 2 x 2 samples, batch 1: one coefficient per band, which cancels)  LEVEL_TOL32_ONE = 1.40e-5
               L = 2   6.11e-8  (analysis, 10 x 18 x 66; every other haar cell): below a tenth                   LEVEL_TOL32[2] = 1e-6
               L = 4   1.28e-7  (analysis, 6 x 6 x 6)                                                            LEVEL_TOL32[4] = 1.29e-6
               L = 6   9.92e-8  (analysis, 22 x 10 x 10): below a tenth                                          LEVEL_TOL32[6] = 1e-6
               L = 8   1.08e-7  (analysis, 14 x 13 x 14, periodic)                                               LEVEL_TOL32[8] = 1.09e-6
  classes, values      2.61e-7  (3 x 63 x 77 x 101 bior2.2 level 2, zero: aaa)                                   API_TOL[float32] = 2.61e-6
(the composed route accumulates in double and keeps 1e-6).  The float32 GRADIENT bounds are ten times the same run's worst figures
over all seven class cases:
  data gradient (through the analysis)                       1.709e-7 (3 x 63 x 77 x 101, zero)      F32_GRAD_X_TOL = 1.709e-6
  coefficient-leaf gradients (through the synthesis), plane  5.071e-5 (the same case, plane 10)      F32_GRAD_C_TOL = 5.071e-4
  the same, all planes of a case taken as one vector         1.135e-7 (2 x 96 x 128 x 160, db4)      F32_GRAD_C_ALL_TOL = 1.135e-6
(the per-plane figure of the coefficient gradients is large because the gradient of a detail plane is the high-pass analysis of the
smooth cosine weight, which cancels; the all-planes bound is the one with teeth, as in tests/test_gpu_boundary_kernels.py).

No cell is skipped: a cell whose reference raises ("reflect" on an odd extent of one sample: L = 2, M = 1) must raise ValueError in
the library too and is counted as raised; the last test fails on a non-zero count of skipped cells and prints WORST.
"""
import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _boundary, _bwt, _engine
from ptwt_amd._wavelets import host_taps
from tests import _boundary3_ref as B3
from tests import _golden as G

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = (F32, F64)
LEVEL_TOL = {F64: 1e-12, F32: 1e-6}
LEVEL_TOL32 = {2: 1e-6, 4: 1.29e-6, 6: 1e-6, 8: 1.09e-6}  # fused float32 level calls, per filter length (module docstring)
LEVEL_TOL32_ONE = 1.40e-5  # ... cells with an axis of one coefficient (L = 2, M = 1): a single cancelling value per band
API_TOL = {F64: 1e-12, F32: 2.61e-6}
F64_GRAD_TOL = 1e-11
# 10 x the float32 CPU chain's own worst gradient errors against its float64 run (``python -m tests.test_gpu_boundary3`` prints them)
F32_GRAD_X_TOL = 1.709e-6      # d/dx through the analysis
F32_GRAD_C_TOL = 5.071e-4      # d/dcoefficient through the synthesis, per plane (the detail planes cancel)
F32_GRAD_C_ALL_TOL = 1.135e-6  # d/dcoefficient, all planes of a case as one vector
# worst norm-wise errors of the module on the MI355X, as its last test prints them.  EMPTY: the module has not run on the device yet
# (EXPERIMENTS.md part B); fill it from the first run's printout
WORST_ON_MI355X = {
}

# ---- brick geometry, in coefficients (csrc/mifwt_bwt3.hip; E = 4 float32 / 2 float64 elements per 16-byte access) -----------------------
#   Fwd3Tile: TD = 4 (L <= 6), 3 (L = 8);  TR = 8 (L <= 4), 6 (L = 6), 4 (L = 8, float32), 3 (L = 8, float64);  TC = 8 E
#   Inv3Tile: TQD = 4 (L = 2), 2;  TQR = 8 (L = 2), 4, 2 (L = 8, float64);  TQC = 8 E
# (tests/test_boundary3_host.py evaluates this table against the source, without a GPU)
E = {F32: 4, F64: 2}
FUSED = [2, 4, 6, 8]
COMPOSED = [22, 34]


def tile3(direction, dtype, flen):
    e = E[dtype]
    if direction == "fwd":
        return (4 if flen <= 6 else 3), (8 if flen <= 4 else (6 if flen == 6 else (4 if e == 4 else 3))), 8 * e
    return (4 if flen <= 2 else 2), (8 if flen <= 2 else (2 if flen == 8 and e == 2 else 4)), 8 * e


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
    g = np.random.default_rng(9000 + 131 * seed + flen)
    return tuple(tuple(float(v) for v in g.standard_normal(flen) / np.sqrt(flen)) for _ in range(4))


def _err(got, want):
    got, want = got.detach().double(), want.detach().double().to(got.device)
    den = float(torch.linalg.vector_norm(want))
    num = float(torch.linalg.vector_norm(got - want))
    return num / den if den > 0 else num


def _check(got, want, tol, what, key=None):
    """Norm-wise error below ``tol`` and max-abs error below 10 x tol x the largest value; evaluated where ``got`` lives."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = _err(got, want)
    if key is not None:
        WORST[key] = max(WORST.get(key, 0.0), err)
    assert err < tol, (what, err)
    if want.numel():
        diff = float((got.detach().double() - want.detach().double().to(got.device)).abs().max())
        assert diff <= 10 * tol * max(float(want.abs().max()), 1e-30), (what, "max-abs")
    return err


# ---- 1. single level calls -----------------------------------------------------------------------------------------------------------------
SIG_LAYOUTS = ("contiguous", "colslice", "rowstride", "slicestride", "batchslice")
BAND_LAYOUTS = ("contiguous", "planes", "mixed", "misaligned")


def _rnd(gen, dtype, *shape, device=None):
    t = torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype)
    return t.to(dev() if device is None else device)


def _signal(gen, dtype, batch, sig, layout, device=None):
    """x [batch, d, h, n] with contiguous samples: dense; a width slice of a wider tensor (row stride n + 7, odd element offset 3: a
    misaligned base); rows of a wider tensor (aligned base, row stride = 1 mod 4 elements); slices one or two elements apart from dense
    (row stride a multiple of 4 elements where n is, slice stride always odd); every other entry of a longer batch."""
    d, h, n = sig
    if layout == "contiguous":
        return _rnd(gen, dtype, batch, d, h, n, device=device)
    if layout == "colslice":
        return _rnd(gen, dtype, batch, d, h, n + 7, device=device)[..., 3:3 + n]
    if layout == "rowstride":
        return _rnd(gen, dtype, batch, d, h, n + ((1 - n) % 4 or 4), device=device)[..., :n]
    if layout == "slicestride":
        pad = 1 if (h * n) % 2 == 0 else 2  # (an odd slice stride: no multiple of 2 or 4 elements)
        return _rnd(gen, dtype, batch, d, h * n + pad, device=device)[..., : h * n].unflatten(-1, (h, n))
    assert layout == "batchslice"
    return _rnd(gen, dtype, 2 * batch + 1, d, h, n, device=device)[1::2]


def _bands(gen, dtype, batch, coef, layout, device=None):
    """The eight bands [batch, *coef]: separate dense tensors; the planes of one level buffer; tensors with differing strides (the
    copying branch of ``transposed_level``); the detail bands one element into wider tensors of one width (equal strides, so they reach
    the kernel as they are, at misaligned addresses)."""
    m = coef[-1]
    r = lambda *shape: _rnd(gen, dtype, *shape, device=device)  # noqa: E731
    if layout == "contiguous":
        return [r(batch, *coef) for _ in range(8)]
    if layout == "planes":
        buf = r(batch, 8, *coef)
        return [buf[:, s] for s in range(8)]
    if layout == "mixed":
        out = [r(batch, *coef), r(batch, *coef[:-1], m + 6)[..., 2:2 + m], r(batch, *coef), r(batch, 3, *coef)[:, 1]]
        out += [r(batch, *coef[:-1], m + 5)[..., :m], r(batch, *coef), r(2 * batch, *coef)[::2], r(batch, *coef)]
        assert len({t.stride() for t in out[1:]}) >= 4
        return out
    assert layout == "misaligned"
    return [r(batch, *coef)] + [r(batch, *coef[:-1], m + 4)[..., 1:1 + m] for _ in range(7)]


def _level_ops(direction, dtype, taps, which, sig, batch, mode, layout, round32, device=None):
    """The operands of one cell and its float64 reference as a thunk."""
    flen = len(taps[0])
    gen = torch.Generator().manual_seed(flen * 100003 + 17 * sum(sig) + 1009 * sig[0] + batch)
    coef = [(n + 1) // 2 for n in sig]
    kw = {"round32": round32}
    if direction == "fwd":
        ops = [_signal(gen, dtype, batch, sig, layout, device)]
        assert tuple(ops[0].shape) == (batch, *sig) and ops[0].stride(-1) == 1
        return ops, lambda: B3.rows_level(ops[0].double().cpu(), taps, which, mode, **kw)
    ops = _bands(gen, dtype, batch, coef, layout, device)
    assert all(tuple(t.shape) == (batch, *coef) and t.stride(-1) == 1 for t in ops)
    return ops, lambda: B3.transposed_level([t.double().cpu() for t in ops], taps, which, sig, **kw)


@pytest.fixture
def every_cell_fused(monkeypatch):
    """The single-level cells test the brick kernels themselves: every cell of the envelope goes to ids 30 / 31, also those the routing
    table ``_bwt.COMPOSED3_CELLS`` keeps on the axis passes by default."""
    monkeypatch.setattr(_bwt, "COMPOSED3_CELLS", set())


def _run_level(direction, dtype, taps, which, sig, batch=1, mode="zero", layout="contiguous", bank_name="random", route="fused"):
    """One cell: ``rows_level`` (direction "fwd") or ``transposed_level`` ("inv") against the float64 operators."""
    flen = len(taps[0])
    name = "%s-%s-L%d-n%s-B%d-%s-%s-%s-%s-%s" % (direction, tag(dtype), flen, "x".join(map(str, sig)), batch, mode, layout, which, bank_name, route)
    bk = _bwt.bank(taps, "gramschmidt", which)
    coef = [(n + 1) // 2 for n in sig]
    ops, reference = _level_ops(direction, dtype, taps, which, sig, batch, mode, layout, dtype == F32 and route == "fused")
    call = (lambda: _bwt.rows_level(ops[0], bk, _engine.MODE_IDS[mode])) if direction == "fwd" else (lambda: _bwt.transposed_level(ops, bk, sig))
    keep = [t.clone() for t in ops]
    COUNTS["cells"] += 1
    if direction == "fwd" and mode == "reflect" and any(n == 1 for n in sig):
        # an odd extent of ONE sample (L = 2, M = 1) has nothing to reflect: the reference's padding refuses it, so must both sides
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
        raise
    assert want.dtype == torch.float64
    _engine.level_events = []
    try:
        got = call()
        kids = [e[1] for e in _engine.level_events]
    finally:
        _engine.level_events = None
    torch.cuda.synchronize()
    fwd = direction == "fwd"
    if route == "fused":
        assert kids == [_bwt.KID_FWD3 if fwd else _bwt.KID_INV3], (name, kids)
    elif route == "composed":
        assert kids == [_bwt.KID_AXIS_FWD if fwd else _bwt.KID_AXIS_INV] * 7, (name, kids)
    else:
        assert kids == [], (name, kids)
    assert got.dtype == dtype, name
    for a, b in zip(ops, keep):
        assert torch.equal(a, b), (name, "an input was modified")
    key = "level %s %s %s" % (direction, route, tag(dtype))
    tol = LEVEL_TOL[dtype]
    if dtype == F32 and route == "fused":
        tol = LEVEL_TOL32_ONE if 1 in coef else LEVEL_TOL32[flen]
    if fwd:
        assert tuple(got.shape) == (batch, 8, *coef), name
        for s in range(8):
            _check(got[:, s], want[:, s], tol, (name, "band", s), key)
    else:
        assert tuple(got.shape) == (batch, *sig), name
        _check(got, want, tol, name, key)


def base_extents(direction, dtype, flen):
    """Per axis the smallest coefficient extent >= L - 1 (and >= 1) that is no multiple of the brick extent."""
    out = []
    for t in tile3(direction, dtype, flen):
        m = max(flen - 1, 1)
        while m % t == 0:
            m += 1
        out.append(m)
    return out


def axis_counts(direction, dtype, flen, axis):
    t, nb = tile3(direction, dtype, flen)[axis], _boundary.boundary_rows(flen)[1]
    cand = {flen - 1, t - 1, t, t + 1, 2 * t + 3} | ({t + nb + 1} if nb else set())
    return sorted(m for m in cand if m >= max(flen - 1, 1))


def level_cells(direction, dtype, flen):
    """(coefficient extents, signal extents, mode, batch) of the fused cells of one kernel instance."""
    base = base_extents(direction, dtype, flen)
    cells, turn = [], 0
    for axis in range(3):
        for m in axis_counts(direction, dtype, flen, axis):
            coef = list(base)
            coef[axis] = m
            cells.append((list(2 * c for c in coef), "zero", 1))
            odd = [2 * c for c in coef]
            odd[axis] -= 1
            cells.append((odd, B3.MODES[turn % 5] if direction == "fwd" else "zero", 3 if turn % 4 == 0 else 1))
            turn += 1
    t = tile3(direction, dtype, flen)
    ragged = [max(x + 1, flen - 1) for x in t]
    cells.append(([2 * c for c in ragged], "zero", 3))
    modes = B3.MODES if direction == "fwd" else ("zero",)
    for mode in modes:
        for axes in ((0,), (1,), (2,), (0, 1, 2)):
            cells.append(([2 * c - (a in axes) for a, c in enumerate(base)], mode, 1))
    return cells


@pytest.mark.parametrize("flen", FUSED)
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("direction", ["fwd", "inv"])
def test_fused_level_extents_and_odd_modes(direction, dtype, flen, every_cell_fused):
    for seed, which in enumerate(("analysis", "synthesis")):
        taps = random_bank(flen, seed)
        for sig, mode, batch in level_cells(direction, dtype, flen):
            _run_level(direction, dtype, taps, which, sig, batch, mode)


@pytest.mark.parametrize("flen", FUSED)
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("direction", ["fwd", "inv"])
def test_fused_level_layouts_and_many_workgroups(direction, dtype, flen, every_cell_fused):
    t = tile3(direction, dtype, flen)
    coef = [max(x + 1, flen - 1) for x in t]
    taps = random_bank(flen, 2)
    which = "analysis" if direction == "fwd" else "synthesis"
    for layout in (SIG_LAYOUTS if direction == "fwd" else BAND_LAYOUTS):
        for sig, mode in (([2 * c for c in coef], "zero"), ([2 * c - 1 for c in coef], "symmetric" if direction == "fwd" else "zero")):
            _run_level(direction, dtype, taps, which, sig, 3, mode, layout)
    big = [2 * x + 3 for x in t]
    _run_level(direction, dtype, taps, which, [2 * c - 1 for c in big], 9, "periodic" if direction == "fwd" else "zero")  # 243 workgroups


@pytest.mark.parametrize("wavelet", ["db3", "bior2.2"])
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_fused_level_pywt_banks(dtype, wavelet, every_cell_fused):
    taps = host_taps(wavelet)
    flen = len(taps[0])
    for direction, which in (("fwd", "analysis"), ("inv", "synthesis"), ("fwd", "synthesis"), ("inv", "analysis")):
        coef = [2 * x + 1 for x in tile3(direction, dtype, flen)]
        _run_level(direction, dtype, taps, which, [2 * c for c in coef], 2, "zero", bank_name=wavelet)
        _run_level(direction, dtype, taps, which, [2 * c - 1 for c in coef], 1, "reflect" if direction == "fwd" else "zero", bank_name=wavelet)


# ---- 2. composed and dense routes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_composed_and_dense_routes(dtype, monkeypatch):
    for flen in COMPOSED:
        taps = random_bank(flen, 3)
        m = flen - 1
        for direction, which in (("fwd", "analysis"), ("inv", "synthesis")):
            _run_level(direction, dtype, taps, which, [2 * m, 2 * m + 3, 2 * m + 10], 2, "constant" if direction == "fwd" else "zero", route="composed")
    monkeypatch.setattr(_bwt, "FORCE_COMPOSED3", True)
    taps = random_bank(6, 4)
    for direction, which in (("fwd", "synthesis"), ("inv", "analysis")):
        _run_level(direction, dtype, taps, which, [21, 30, 77], 3, "reflect" if direction == "fwd" else "zero", route="composed")
        _run_level(direction, dtype, taps, which, [20, 31, 76], 1, "periodic" if direction == "fwd" else "zero", layout="colslice" if direction == "fwd" else "mixed", route="composed")
    monkeypatch.setattr(_bwt, "FORCE_COMPOSED3", False)
    taps = host_taps("db4")
    for direction, which in (("fwd", "analysis"), ("inv", "synthesis")):
        _run_level(direction, dtype, taps, which, [12, 40, 40], 2, route="dense", bank_name="db4")
        _run_level(direction, dtype, taps, which, [40, 39, 11], 1, "symmetric" if direction == "fwd" else "zero", route="dense", bank_name="db4")


# ---- 3. the public classes -------------------------------------------------------------------------------------------------------------------
def flat(coeffs):
    out = [coeffs[0]]
    for c in coeffs[1:]:
        out.extend(c[k] for k in B3.KEYS)
    return out


def nested(leaves):
    return [leaves[0]] + [dict(zip(B3.KEYS, leaves[p:p + 7])) for p in range(1, len(leaves), 7)]


def fold(t, axes):
    if axes is not None:
        t = torch.movedim(t, tuple(axes), (-3, -2, -1))
    return t.reshape(-1, *t.shape[-3:])


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_classes_reproduce_the_reference_goldens(dtype):
    z, idx = G.load("ptwt_ref_boundary3.npz")
    for case in idx:
        COUNTS["cells"] += 1
        if case["stride"]:
            x64 = torch.from_numpy(B3.formula_input(case["shape"], case["seed"]))
        else:
            x64 = torch.from_numpy(z[case["key"] + "_x"]).double()
        keep = (lambda t: t.reshape(-1)[:: case["stride"]]) if case["stride"] else (lambda t: t)
        axes = case["kw"].get("axes")
        dec = ptwt_amd.MatrixWavedec3(case["wavelet"], case["level"], **case["kw"])
        rec = ptwt_amd.MatrixWaverec3(case["wavelet"], **({"axes": axes} if axes is not None else {}))
        c = dec(x64.to(dtype).to(dev()))
        got = flat(c)
        assert len(got) == case["ncoef"] and dec.padded == case["padded"] and [list(s) for s in dec.size_list] == case["size_list"]
        key = "classes goldens %s" % tag(dtype)
        want = [torch.from_numpy(z["%s_c%d" % (case["key"], i)]) for i in range(case["ncoef"])]
        for i, (a, b) in enumerate(zip(got, want)):
            assert list(a.shape) == case["coef_shapes"][i] and a.dtype == dtype
            _check(keep(a), b, API_TOL[dtype], (case["key"], "coefficient", i), key)
        if case["stride"]:
            leaves = [t.detach() for t in got]  # (checked above on the kept samples; the reconstruction below is from the same values)
        else:
            leaves = [t.to(dtype).to(dev()) for t in want]
        y = rec(nested(leaves))
        assert list(y.shape) == case["rec_shape"]
        _check(keep(y), torch.from_numpy(z[case["key"] + "_rec"]), 2 * API_TOL[dtype] if case["stride"] else API_TOL[dtype],
               (case["key"], "reconstruction"), key)
        if case["grads"] and dtype == F64:
            xg = x64.to(dev()).requires_grad_(True)
            cg = flat(dec(xg))
            (gx,) = torch.autograd.grad(sum((weight(t, i) * t).sum() for i, t in enumerate(cg)), xg)
            _check(gx, torch.from_numpy(z[case["key"] + "_gx"]), F64_GRAD_TOL, (case["key"], "gx"), "classes goldens grads")
            lv = [t.clone().requires_grad_(True) for t in leaves]
            yg = rec(nested(lv))
            gl = torch.autograd.grad((weight(yg, 7) * yg).sum(), lv)
            for i, g in enumerate(gl):
                _check(g, torch.from_numpy(z["%s_gc%d" % (case["key"], i)]), F64_GRAD_TOL, (case["key"], "gc", i), "classes goldens grads")


CLASS_CASES = [("big-db2", (2, 96, 128, 160), "db2", 3, "zero"), ("big-db4", (2, 96, 128, 160), "db4", 2, "zero")] + \
              [("odd-" + m, (3, 63, 77, 101), "bior2.2", 2, m) for m in B3.MODES]
_REF = {}


def class_reference(name, shape, wavelet, level, mode):
    """Inputs and float64 CPU results of one class case, computed once and shared (never modified): x, the coefficients of x, random
    coefficients of the same shapes and their synthesis, and — for the gradient cases — the gradients of the cosine-weighted sums."""
    hit = _REF.get(name)
    if hit is None:
        taps = host_taps(wavelet)
        g = torch.Generator().manual_seed(len(name) + sum(shape))
        x = torch.randn(*shape, generator=g, dtype=torch.float64).float().double()  # (float32-representable: both dtypes see one input)
        xg = x.clone().requires_grad_(True)
        c = B3.wavedec3(xg, taps, level, mode)
        rnd = [torch.randn(*t.shape, generator=g, dtype=torch.float64).float().double().requires_grad_(True) for t in c]
        y = B3.waverec3(rnd, taps)
        hit = dict(x=x, c=[t.detach() for t in c], rnd=[t.detach() for t in rnd], y=y.detach(), y_of_c=B3.waverec3([t.detach() for t in c], taps))
        if name in GRAD_CASES:
            (hit["gx"],) = torch.autograd.grad(sum((weight(t, i) * t).sum() for i, t in enumerate(c)), xg)
            hit["gc"] = list(torch.autograd.grad((weight(y, 7) * y).sum(), rnd))
        _REF[name] = hit
    return hit


GRAD_CASES = tuple(c[0] for c in CLASS_CASES)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("case", CLASS_CASES, ids=lambda c: c[0])
def test_classes_against_the_cpu_chain(case, dtype):
    name, shape, wavelet, level, mode = case
    COUNTS["cells"] += 1
    ref = class_reference(*case)
    dec, rec = ptwt_amd.MatrixWavedec3(wavelet, level, odd_coeff_padding_mode=mode), ptwt_amd.MatrixWaverec3(wavelet)
    key = "classes %s %s" % (name.split("-")[0], tag(dtype))
    c = dec(ref["x"].to(dtype).to(dev()))
    got = flat(c)
    assert len(got) == len(ref["c"])
    for i, (a, b) in enumerate(zip(got, ref["c"])):
        _check(a, b, API_TOL[dtype], (name, "coefficient", i), key)
    y = rec(nested([t.to(dtype).to(dev()) for t in ref["rnd"]]))
    _check(y, ref["y"], API_TOL[dtype], (name, "synthesis of random coefficients"), key)
    y2 = rec(nested([t.to(dtype).to(dev()) for t in ref["c"]]))
    _check(y2, ref["y_of_c"], API_TOL[dtype], (name, "synthesis of the analysis output"), key)


def test_float32_against_the_librarys_float64_on_256_cubed():
    COUNTS["cells"] += 1
    x = torch.randn(2, 256, 256, 256, device=dev(), generator=torch.Generator(device=dev()).manual_seed(5))
    dec, rec = ptwt_amd.MatrixWavedec3("db2", 3), ptwt_amd.MatrixWaverec3("db2")
    c32, c64 = flat(dec(x)), flat(dec(x.double()))
    for i, (a, b) in enumerate(zip(c32, c64)):
        _check(a, b, API_TOL[F32], ("256^3", "coefficient", i), "classes 256^3 float32 vs float64")
    rnd = [torch.randn_like(t) for t in c32]
    _check(rec(nested(rnd)), rec(nested([t.double() for t in rnd])), API_TOL[F32], ("256^3", "synthesis"), "classes 256^3 float32 vs float64")


# ---- 4. gradients ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("name", GRAD_CASES)
def test_gradients_against_autograd_over_the_cpu_chain(name, dtype):
    case = [c for c in CLASS_CASES if c[0] == name][0]
    _, shape, wavelet, level, mode = case
    COUNTS["cells"] += 1
    ref = class_reference(*case)
    dec, rec = ptwt_amd.MatrixWavedec3(wavelet, level, odd_coeff_padding_mode=mode), ptwt_amd.MatrixWaverec3(wavelet)
    x = ref["x"].to(dtype).to(dev()).requires_grad_(True)
    c = flat(dec(x))
    (gx,) = torch.autograd.grad(sum((weight(t, i) * t).sum() for i, t in enumerate(c)), x)
    leaves = [t.to(dtype).to(dev()).requires_grad_(True) for t in ref["rnd"]]
    y = rec(nested(leaves))
    gl = torch.autograd.grad((weight(y, 7) * y).sum(), leaves)
    key = "gradients %s" % tag(dtype)
    if dtype == F64:
        _check(gx, ref["gx"], F64_GRAD_TOL, (name, "gx"), key + " x")
        for i, g in enumerate(gl):
            _check(g, ref["gc"][i], F64_GRAD_TOL, (name, "gc", i), key + " c")
        return
    _check(gx, ref["gx"], F32_GRAD_X_TOL, (name, "gx"), key + " x")
    for i, g in enumerate(gl):
        _check(g, ref["gc"][i], F32_GRAD_C_TOL, (name, "gc", i), key + " c plane")
    _check(torch.cat([g.reshape(-1) for g in gl]), torch.cat([g.reshape(-1) for g in ref["gc"]]), F32_GRAD_C_ALL_TOL, (name, "gc all"), key + " c all")


# ---- 5. capture and canaries -----------------------------------------------------------------------------------------------------------------
def test_capture_replays_bit_identically():
    COUNTS["cells"] += 1
    dec, rec = ptwt_amd.MatrixWavedec3("db3", level=2, odd_coeff_padding_mode="reflect"), ptwt_amd.MatrixWaverec3("db3")
    x0 = torch.randn(3, 45, 50, 67, device=dev())
    x1 = torch.randn(3, 45, 50, 67, device=dev())
    rec(dec(x0))  # warm call: the tables become resident
    torch.cuda.synchronize()
    eager = dec(x1)
    back = rec(eager)
    fwd = ptwt_amd.capture(lambda t: dec(t), x0)
    for a, b in zip(flat(fwd(x1)), flat(eager)):
        assert torch.equal(a, b)
    inv = ptwt_amd.capture(lambda t: rec(dec(t)), x0)
    assert torch.equal(inv(x1), back)


@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
def test_canaries_around_outputs_and_inputs(monkeypatch, dtype):
    from tests.test_gpu_boundary import _GuardedTorch

    guard = _GuardedTorch()
    scenarios = [((3, 18, 22, 70), "db4", False), ((2, 17, 19, 67), "db2", False), ((3, 9, 17, 33), "haar", False),
                 ((2, 23, 21, 37), "db3", False), ((2, 21, 26, 45), "db3", True), ((1, 12, 40, 41), "db4", False)]
    for shape, wavelet, composed in scenarios:
        COUNTS["cells"] += 1
        dec, rec = ptwt_amd.MatrixWavedec3(wavelet, level=1, odd_coeff_padding_mode="symmetric"), ptwt_amd.MatrixWaverec3(wavelet)
        monkeypatch.setattr(_bwt, "FORCE_COMPOSED3", composed)
        # the input sits inside a guarded block as well (a read before / past it would show as a wrong result below)
        x = guard.empty(shape, dtype=dtype, device=dev())
        x.copy_(torch.randn(*shape, device=dev(), dtype=dtype))
        x_before = x.clone()
        want_c = dec(x)
        want_y = rec(want_c)
        monkeypatch.setattr(_bwt, "torch", guard)
        try:
            c = dec(x)
            y = rec(c)
        finally:
            monkeypatch.setattr(_bwt, "torch", torch)
        guard.check((shape, wavelet, dtype))
        assert torch.equal(x, x_before)
        assert all(torch.equal(a, b) for a, b in zip(flat(c), flat(want_c))) and torch.equal(y, want_y)
        assert list(y.shape[-3:]) == [n + n % 2 for n in shape[-3:]]
    monkeypatch.setattr(_bwt, "FORCE_COMPOSED3", False)


# ---- 6. no skipped cells ---------------------------------------------------------------------------------------------------------------------
def test_zz_no_cell_was_skipped_and_report_worst():
    print("\ntests/test_gpu_boundary3.py: cells", COUNTS)
    for key in sorted(WORST):
        print("  WORST %-48s %.3e" % (key, WORST[key]))
    assert COUNTS["skipped"] == 0, COUNTS
    assert COUNTS["cells"] > 0


# ---- the CPU chain in float32 against its own float64 run (``python -m tests.test_gpu_boundary3``; no GPU) --------------------------------
def _cpu_float32_figures():
    worst = {}

    def note(key, err, what):
        if err > worst.get(key, (0.0, None))[0]:
            worst[key] = (err, what)

    def rel(a, b):
        return float(torch.linalg.vector_norm(a.double() - b) / torch.linalg.vector_norm(b))

    def lkey(flen, sig):
        return "level M=1" if any((n + 1) // 2 == 1 for n in sig) else "level L=%d" % flen

    for flen in FUSED:
        for direction in ("fwd", "inv"):
            for seed, which in enumerate(("analysis", "synthesis")):
                taps = random_bank(flen, seed)
                for sig, mode, batch in level_cells(direction, F32, flen):
                    if mode == "reflect" and 1 in sig:
                        continue
                    ops, reference = _level_ops(direction, F32, taps, which, sig, batch, mode, "contiguous", True, device="cpu")
                    want = reference()
                    if direction == "fwd":
                        got = B3.rows_level(ops[0], taps, which, mode, round32=True)
                        for s in range(8):
                            note(lkey(flen, sig), rel(got[:, s], want[:, s]), (direction, flen, sig, mode, s))
                    else:
                        got = B3.transposed_level(ops, taps, which, sig, round32=True)
                        note(lkey(flen, sig), rel(got, want), (direction, flen, sig))
    for case in CLASS_CASES:
        name, shape, wavelet, level, mode = case
        ref = class_reference(*case)
        taps = host_taps(wavelet)
        x = ref["x"].float().requires_grad_(True)
        c = B3.wavedec3(x, taps, level, mode)
        for i, (a, b) in enumerate(zip(c, ref["c"])):
            note("classes", rel(a.detach(), b), (name, "coefficient", i))
        leaves = [t.float().requires_grad_(True) for t in ref["rnd"]]
        y = B3.waverec3(leaves, taps)
        note("classes", rel(y.detach(), ref["y"]), (name, "synthesis"))
        if name in GRAD_CASES:
            (gx,) = torch.autograd.grad(sum((weight(t, i) * t).sum() for i, t in enumerate(c)), x)
            note("grad x", rel(gx, ref["gx"]), name)
            gl = torch.autograd.grad((weight(y, 7) * y).sum(), leaves)
            for i, g in enumerate(gl):
                note("grad c plane", rel(g, ref["gc"][i]), (name, i))
            note("grad c all", rel(torch.cat([g.reshape(-1) for g in gl]), torch.cat([g.reshape(-1) for g in ref["gc"]])), name)
    for key, (err, what) in sorted(worst.items()):
        print("%-14s %.3e  %s" % (key, err, what))


if __name__ == "__main__":
    _cpu_float32_figures()
