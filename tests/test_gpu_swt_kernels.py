"""GPU tests (``-m gpu``) of the stationary-transform kernels (csrc/mifwt_swt.hip, ``mifwt_tap_correlate_dilated`` of
csrc/mifwt_tapgrad.hip) against float64 references, at the shapes the lane layout makes interesting.

1. Single level calls.  ``stationary_transform._level_fwd`` / ``_level_inv`` (the ctypes binding: any dilation, any scale, any dtype)
   against the numpy stand-ins ``swt_level_fwd`` / ``swt_level_inv`` of tests/_oracle_engine.py evaluated in float64 on the same,
   already quantised, inputs (tests/test_torch_autograd_ref.py pins the stand-ins to the differentiable reference, and that to the
   reference library's goldens).  A lane owns E = 4 / 2 / 4 samples (float32 / float64 / float16) and a wave 64 E, so the extents are
   1, 2, 3, 5 (rows shorter than a lane's run), 255 .. 259 (a tail of 3 / 0 / 1 / 2 / 3 samples after one full float32 wave), 1001, 4098
   and 40960 (the vector path dominates); every unrolled length 2 .. 20 and the run-time lengths 22, 34, 76, 102 and 128 in every
   dtype; dilations 1 .. 1024 and 3; windows several rows long; banks of four INDEPENDENT random filters (for a pywt bank rec is dec
   reversed and hi the alternating flip of lo: a kernel that reads the wrong filter of a pair can still give the expected numbers) and
   the pywt banks of the lengths the goldens miss; contiguous rows, a column slice of a wider tensor at an odd element offset, the
   low-pass plane of a level buffer and, for synthesis, two operands with different row strides.  Inputs of ``_level_inv`` are random
   coefficient sets, not images of an analysis.  ``mifwt_tap_correlate_dilated`` is compared the same way with its closed form.
2. ``swt`` / ``iswt`` with the four taps as leaf tensors against ``swt`` / ``iswt`` of oracle/torch_autograd_ref.py: coefficients,
   reconstruction, the gradients w.r.t. the data, the coefficient leaves and all four filters from one backward, float32 and float64;
   one float64 double backward.

Bounds, norm-wise per output plane (``tests._golden.relerr``) plus a max-abs companion of 10 x bound x the largest value:
float64 1e-12 (values) / 1e-10 (gradients) / 1e-9 (second order); float32 values 1e-6; float16 5e-4 per level call
(output rounding, 2^-11; the oracle is fed the same float16 values).  Float32 taps and scales are rounded to float32 on
both sides.  The float32 GRADIENT bounds come from the reference alone: ``python -m tests.test_gpu_swt_kernels`` runs the reference in
float32 on the host over API_CASES and prints its worst norm-wise error against its own float64 run — 7.6e-7 for the data and
coefficient gradients (the 1 x 100000 case), 1.2e-6 for the tap gradients (the 64 x 520 case) — and the bounds are ten times those
figures, because the GPU reduces in a different order: F32_GRAD_TOL = 7.6e-6, F32_TAP_TOL = 1.2e-5.  On the MI355X the library's worst
float32 gradient errors were 8.4e-7 (data) and 7.6e-7 (taps); every figure of that run is in WORST_ON_MI355X below.

No cell is skipped: a cell whose oracle raises must raise in the library too and is counted, and the last test fails on a non-zero
count.
"""
import json
import os

import numpy as np
import pytest
import torch

import ptwt_amd
from oracle import torch_autograd_ref as R
from ptwt_amd import _engine
from ptwt_amd import stationary_transform as st
from tests import _golden as G
from tests import _oracle_engine as oe

pytestmark = pytest.mark.gpu

TAPS = ("dec_lo", "dec_hi", "rec_lo", "rec_hi")
VALUE_TOL = {torch.float64: 1e-12, torch.float32: 1e-6, torch.float16: 5e-4}
F64_TOL = 1e-10
F32_GRAD_TOL = 7.6e-6  # 10 x the float32 reference's own worst data / coefficient gradient error (module docstring)
F32_TAP_TOL = 1.2e-5   # 10 x the float32 reference's own worst tap gradient error
# worst norm-wise errors the module showed on the MI355X (printed by its last test).  The float32 synthesis figure is the cell N = 1,
# L = 34: three output samples, each a sum of 68 products that cancel; the cells with whole rows stay below 3e-7.
WORST_ON_MI355X = {
    "level fwd float64": 5.7e-16, "level fwd float32": 2.2e-7, "level fwd float16": 3.3e-4,
    "level inv float64": 6.7e-16, "level inv float32": 9.7e-7, "level inv float16": 3.2e-4,
    "tap reduction float64": 2.6e-15, "tap reduction float32": 4.4e-8,
    "swt values float64": 5.6e-16, "swt values float32": 2.8e-7,
    "swt data gradients float64": 1.7e-15, "swt data gradients float32": 8.4e-7,
    "swt tap gradients float64": 3.5e-15, "swt tap gradients float32": 7.6e-7,
    "swt second order float64": 5.6e-16,
}

WORST = {}
COUNTS = {"cells": 0, "skipped": 0}
MAX_FILT = 128  # MIFWT_MAX_FILT (include/mifwt.h)


def dev():
    return torch.device("cuda:0")


def weight(t, i):
    return torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64, device=t.device) + i).reshape(t.shape).to(t.dtype)


def random_bank(flen, seed):
    """Four independent filters scaled by 1 / sqrt(L) (outputs of the size of the inputs: float16 stays in range)."""
    g = np.random.default_rng(4000 + seed)
    return [g.standard_normal(flen) / np.sqrt(flen) for _ in range(4)]


def pywt_bank(name):
    with open(os.path.join(G.GOLDEN, "pywt_filter_banks.json")) as f:
        b = json.load(f)[name]
    return [np.asarray(b[k], dtype=np.float64) for k in TAPS]


def _note(key, err):
    WORST[key] = max(WORST.get(key, 0.0), float(err))


def _check(got, want, tol, what, key=None):
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = G.relerr(got.numpy(), want.numpy())
    if key is not None:
        _note(key, err)
    assert err < tol, (what, err)
    if want.numel():
        assert float((got - want).abs().max()) <= 10 * tol * max(float(want.abs().max()), 1e-30), (what, "max-abs")
    return err


def _quantised(values, dtype):
    """Taps / scale as the kernel will see them: float32 accumulation for float32 and float16 storage."""
    if dtype == torch.float64:
        return [float(v) for v in values]
    return [float(np.float32(v)) for v in values]


# ---- 1. single level calls ------------------------------------------------------------------------------------------------------------
SCALES = (1.0, 0.5, float(np.pi / 7))
LAYOUTS = ("contiguous", "slice", "plane", "mixed")
DTYPES = (torch.float32, torch.float64, torch.float16)
UNROLLED = list(range(2, 21, 2))
RUNTIME = [22, 34, 76, 102, MAX_FILT]


def _operand(rows, n, layout, dtype, gen):
    """A [rows, n] operand with contiguous samples: dense, a column slice of a wider tensor (row stride n + 7, odd element offset), or
    the low-pass / high-pass plane of a [rows, 2, n] level buffer (row stride 2 n)."""
    def rnd(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype).to(dev())

    if layout == "contiguous":
        return rnd(rows, n)
    if layout == "slice":
        return rnd(rows, n + 7)[:, 3:3 + n]
    if layout == "plane":
        return rnd(rows, 2, n)[:, 0]
    assert layout == "plane1"
    return rnd(rows, 2, n)[:, 1]


def _cells():
    cells = []

    def add(dtype, flen, n, dilation, rows=3, bank=None):
        i = len(cells)
        cells.append((dtype, flen, n, dilation, rows, LAYOUTS[i % 4], SCALES[i % 3], bank))

    for dtype in DTYPES:
        # every (dtype, L): a ragged extent, an odd extent of several waves, an extent where the vector path dominates
        for flen in UNROLLED + RUNTIME:
            add(dtype, flen, 259, 1)
            add(dtype, flen, 1001, 2 if flen > 34 else 4)
            add(dtype, flen, 4098, 16 if flen > 34 else 64)
        # every (dtype, N) at an unrolled and a run-time length, the dilations spread over the cells
        for n, d_a, d_b in ((1, 1, 2), (2, 3, 1), (3, 1, 4), (5, 2, 3), (255, 4, 1), (256, 16, 2), (257, 3, 4), (258, 64, 1), (259, 2, 3),
                            (1001, 16, 4), (4098, 1024, 3), (40960, 1, 1024)):
            add(dtype, 8, n, d_a)
            add(dtype, 34, n, d_b)
        add(dtype, 20, 40960, 64)
        add(dtype, 4, 40960, 1024, rows=1)
        add(dtype, 16, 24, 4)             # D L > 2 N: every window wraps several times
        add(dtype, 8, 256, 64)            # D L/2 == N
        add(dtype, 6, 96, 32, rows=1)     # D L/2 == N, synthesis offset D (L/2 - 1) short of it
        add(dtype, 4, 258, 2, rows=3000)  # many rows
        add(dtype, 4, 258, 2, rows=3001)  # rows x segments not a multiple of the 4 waves of a workgroup: idle waves in the last one
        add(dtype, 10, 257, 1, rows=1)
        for name in ("db6", "db7", "db9", "db10"):
            add(dtype, len(pywt_bank(name)[0]), 258, 1, bank=name)
            add(dtype, len(pywt_bank(name)[0]), 1001, 4, bank=name)
    return cells


CELLS = _cells()


def _cell_id(c):
    return "%s-L%d-N%d-D%d-rows%d-%s-s%.3g-%s" % (str(c[0]).split(".")[-1], c[1], c[2], c[3], c[4], c[5], c[6], c[7] or "random")


def _run_cell(direction, cell):
    dtype, flen, n, dilation, rows, layout, scale, bank_name = cell
    bank = pywt_bank(bank_name) if bank_name else random_bank(flen, flen + n)
    assert len(bank[0]) == flen
    gen = torch.Generator().manual_seed(flen * 100003 + n + dilation)
    (scale,) = _quantised([scale], dtype)
    if direction == "fwd":
        lo, hi = _quantised(bank[0], dtype), _quantised(bank[1], dtype)
        ops = [_operand(rows, n, "slice" if layout == "mixed" else layout, dtype, gen)]
        oracle, call = oe.swt_level_fwd, st._level_fwd
    else:
        lo, hi = _quantised(bank[2], dtype), _quantised(bank[3], dtype)
        ops = [_operand(rows, n, "slice", dtype, gen), _operand(rows, n, "plane1", dtype, gen)] if layout == "mixed" else \
            [_operand(rows, n, layout, dtype, gen), _operand(rows, n, layout, dtype, gen)]
        oracle, call = oe.swt_level_inv, st._level_inv
    keep = [t.clone() for t in ops]
    COUNTS["cells"] += 1
    try:
        want = oracle(*[t.double().cpu() for t in ops], lo, hi, dilation, scale)
    except Exception:
        COUNTS["skipped"] += 1
        with pytest.raises(Exception):
            call(*ops, lo, hi, dilation, scale)
        return
    assert want.dtype == torch.float64
    with ptwt_amd.half_storage(dtype == torch.float16):
        got = call(*ops, lo, hi, dilation, scale)
    torch.cuda.synchronize()
    assert got.dtype == dtype and got.is_contiguous()
    for a, b in zip(ops, keep):
        assert torch.equal(a, b), "an input was modified"
    tol = VALUE_TOL[dtype]
    key = "level %s %s" % (direction, str(dtype).split(".")[-1])
    if direction == "fwd":
        assert got.shape == (rows, 2, n)
        _check(got[:, 0], want[:, 0], tol, (direction, _cell_id(cell), "lo"), key)
        _check(got[:, 1], want[:, 1], tol, (direction, _cell_id(cell), "hi"), key)
    else:
        _check(got, want, tol, (direction, _cell_id(cell)), key)


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_analysis_level_vs_float64_oracle(cell):
    _run_cell("fwd", cell)


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_synthesis_level_vs_float64_oracle(cell):
    _run_cell("inv", cell)


def test_the_matrix_covers_what_it_claims():
    """(no GPU work) every (dtype, L) pair has a ragged and an interior-dominated cell, every (dtype, N) two lengths, every dtype a cell
    with D L > 2 N and one with D L/2 a multiple of N; every layout and scale occurs in every dtype."""
    for dtype in DTYPES:
        mine = [c for c in CELLS if c[0] == dtype]
        for flen in UNROLLED + RUNTIME:
            ns = {c[2] for c in mine if c[1] == flen}
            assert {259, 4098} <= ns, (dtype, flen)
        for n in (1, 2, 3, 5, 255, 256, 257, 258, 259, 1001, 4098, 40960):
            assert len({c[1] for c in mine if c[2] == n}) >= 2, (dtype, n)
        assert {c[3] for c in mine} >= {1, 2, 3, 4, 16, 64, 1024}
        assert any(c[3] * c[1] > 2 * c[2] and c[2] > 5 for c in mine) and any((c[3] * c[1] // 2) % c[2] == 0 and c[2] > 5 for c in mine)
        assert {c[4] for c in mine} >= {1, 3, 3000, 3001}
        assert {c[5] for c in mine} == set(LAYOUTS) and {c[6] for c in mine} == set(SCALES)
        assert {c[7] for c in mine} >= {"db6", "db7", "db9", "db10"}
        wave = 64 * (2 if dtype == torch.float64 else 4)
        assert any((c[4] * -(-c[2] // wave)) % 4 for c in mine if c[4] > 1000)


def test_level_calls_refuse_bad_lengths_and_take_empty_batches():
    x = torch.randn(3, 64, device=dev())
    for flen in (3, 21, MAX_FILT + 2):
        taps = [0.1] * flen
        with pytest.raises(RuntimeError, match="libmifwt"):
            st._level_fwd(x, taps, taps, 1, 1.0)
        with pytest.raises(RuntimeError, match="libmifwt"):
            st._level_inv(x, x, taps, taps, 1, 0.5)
    for dtype in (torch.float32, torch.float64):
        e = torch.empty(0, 64, device=dev(), dtype=dtype)
        buf = st._level_fwd(e, [0.5, 0.5], [0.5, -0.5], 1, 1.0)
        assert buf.shape == (0, 2, 64) and buf.dtype == dtype
        y = st._level_inv(e, e, [0.5, 0.5], [0.5, -0.5], 1, 0.5)
        assert y.shape == (0, 64) and y.dtype == dtype


# ---- the tap reduction, directly --------------------------------------------------------------------------------------------------------
# (rows, N, L, D, layout): out[t] += sum a[row, k] b[row, (k + D L/2 - D t) mod N]
CORR_CELLS = [
    (2, 24, 16, 4, "contiguous"),     # offsets several periods outside the row (the general fallback of the index map)
    (3, 1, 4, 2, "contiguous"),       # N = 1: every offset is periods away
    (2, 6, 8, 2, "slice"),
    (5, 1001, 8, 3, "mixed"),         # odd N, two different row strides
    (3, 259, 20, 1, "plane"),
    (2, 3000, 102, 2, "slice"),       # four passes of 32 taps
    (1, 100000, 34, 2, "contiguous"),  # second pass
    (7, 100001, 6, 1024, "mixed"),    # more samples than threads in the grid: the grid-stride loop runs more than once
    (2, 40960, MAX_FILT, 64, "plane"),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("cell", CORR_CELLS, ids=lambda c: "rows%d-N%d-L%d-D%d-%s" % c)
def test_tap_correlate_dilated_vs_float64_closed_form(cell, dtype):
    """Bounds: float64 1e-12; float32 1e-6 — the products are float32 FMAs summed per thread (a handful of terms), everything above a
    thread is summed in double, so the error of a tap is that of plain float32 products."""
    rows, n, flen, dilation, layout = cell
    gen = torch.Generator().manual_seed(n + flen)
    a = _operand(rows, n, "slice" if layout == "mixed" else layout, dtype, gen)
    b = _operand(rows, n, "plane1" if layout == "mixed" else layout, dtype, gen)
    for c0 in (dilation * (flen // 2), dilation * (flen // 2 - 1)):
        out = torch.zeros(flen, dtype=torch.float64, device=dev())
        _engine.ENGINE.tap_correlate_dilated(a, b, flen, c0, -dilation, out)
        an, bn = a.double().cpu().numpy(), b.double().cpu().numpy()
        want = np.array([(an * bn[:, (np.arange(n) + c0 - dilation * t) % n]).sum() for t in range(flen)])
        # (the sums cancel: the error is measured against the size of the terms, sqrt(rows N) for unit-variance operands, as the
        # norm of a gradient that does not cancel would be)
        floor = np.sqrt(flen * rows * n)
        err = np.linalg.norm(out.cpu().numpy() - want) / max(np.linalg.norm(want), floor)
        _note("tap reduction %s" % str(dtype).split(".")[-1], err)
        assert err < VALUE_TOL[dtype], (cell, c0, err)
        out2 = out.clone()
        _engine.ENGINE.tap_correlate_dilated(a, b, flen, c0, -dilation, out2)  # accumulates
        assert np.linalg.norm(out2.cpu().numpy() - 2 * want) / max(np.linalg.norm(want), floor) < 2 * VALUE_TOL[dtype], cell


# ---- 2. swt / iswt with learnable taps vs the differentiable float64 reference ------------------------------------------------------------
def _view_input(wide):
    """A non-contiguous input whose rows are a column slice of a wider tensor (row stride N + 11, odd element offset)."""
    return wide[:, ::1][:, 5:wide.shape[1] - 6]


# (name, shape, L, level, keyword arguments, view of the input or None, seed of the bank)
API_CASES = [
    ("3x4098-L2", (3, 4098), 2, 1, {}, None, 0),
    ("5x1001-L4", (5, 1001), 4, 3, {}, None, 0),
    ("2x40960-L20", (2, 40960), 20, 5, {}, None, 0),
    ("7x8200-L12", (7, 8200), 12, 3, {}, None, 0),
    ("64x520-L6", (64, 520), 6, 3, {}, None, 0),
    ("2x24-L16", (2, 24), 16, 3, {}, None, 0),           # many wraps, also in the tap reduction
    ("3x1-L4", (3, 1), 4, 2, {}, None, 0),
    ("2x6-L8", (2, 6), 8, 2, {}, None, 0),
    ("1x100000-L34", (1, 100000), 34, 2, {}, None, 0),   # second tap pass of the reduction
    ("2x3000-L102", (2, 3000), 102, 2, {}, None, 0),
    ("axis1-4x520x3-L8", (4, 520, 3), 8, 3, {"axis": 1}, None, 0),
    ("view-3x1003-L10", (3, 1003), 10, 2, {}, _view_input, 0),
    ("1d-259-L14", (259,), 14, 2, {}, None, 0),
    ("3x777-L18", (3, 777), 18, 2, {}, None, 0),
]


def _api_inputs(case, dtype):
    """The input (host; ``view`` rebuilds the case's view of it on any device) and the four taps, in the case's dtype."""
    name, shape, flen, level, kw, view, seed = case
    gen = torch.Generator().manual_seed(flen * 1000 + shape[-1])
    x = torch.randn(*shape[:-1], shape[-1] + (11 if view else 0), generator=gen, dtype=torch.float64).to(dtype)
    taps = [torch.tensor(b, dtype=dtype) for b in random_bank(flen, 1000 * seed + flen)]
    return x, taps, (view or (lambda t: t))


def _api_run(mod, x, taps, leaves, level, kw):
    """The ``weight`` loss over all coefficients plus the reconstruction of given coefficient leaves, one backward."""
    x = x.detach().requires_grad_(True)
    taps = [t.detach().clone().requires_grad_(True) for t in taps]
    leaves = [t.detach().clone().requires_grad_(True) for t in leaves] if leaves is not None else None
    c = mod.swt(x, tuple(taps), level, **kw)
    if leaves is None:
        leaves = [t.detach().clone().requires_grad_(True) for t in c]
    y = mod.iswt(leaves, tuple(taps), **kw)
    loss = sum((weight(t, i) * t).sum() for i, t in enumerate(c)) + (weight(y, 7) * y).sum()
    grads = torch.autograd.grad(loss, [x] + leaves + taps)
    n = len(leaves)
    return ([t.detach() for t in c], y.detach(), grads[0], list(grads[1:1 + n]), list(grads[1 + n:]), [t.detach() for t in leaves])


def measure_reference_f32():
    """The float32 reference on the host against the float64 reference, over API_CASES on the same float32 inputs: the worst norm-wise
    errors of the values, of the data / coefficient gradients and of the tap gradients.  The float32 gradient bounds of this module are
    ten times what this prints."""
    worst = {"values": 0.0, "data gradients": 0.0, "tap gradients": 0.0}
    for case in API_CASES:
        x, taps, view = _api_inputs(case, torch.float32)
        leaves32 = [t.float() for t in _api_run(R, view(x.double()), [t.double() for t in taps], None, case[3], case[4])[5]]
        # (both runs reconstruct the same float32 coefficient leaves)
        c64, y64, gx64, gl64, gt64, _ = _api_run(R, view(x.double()), [t.double() for t in taps], [t.double() for t in leaves32], case[3], case[4])
        c32, y32, gx32, gl32, gt32, _ = _api_run(R, view(x), taps, leaves32, case[3], case[4])
        e_v = max(G.relerr(a.numpy(), b.numpy()) for a, b in zip(c32 + [y32], c64 + [y64]))
        e_d = max(G.relerr(a.numpy(), b.numpy()) for a, b in zip([gx32] + gl32, [gx64] + gl64))
        e_t = max(G.relerr(a.numpy(), b.numpy()) for a, b in zip(gt32, gt64))
        print("%-20s values %.2e  data gradients %.2e  tap gradients %.2e" % (case[0], e_v, e_d, e_t))
        for k, e in zip(worst, (e_v, e_d, e_t)):
            worst[k] = max(worst[k], e)
    print("worst:", {k: "%.2e" % v for k, v in worst.items()})
    return worst


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("case", API_CASES, ids=lambda c: c[0])
def test_swt_iswt_with_learnable_taps_vs_reference(case, dtype):
    name, shape, flen, level, kw, _, _ = case
    x, taps, view = _api_inputs(case, dtype)
    xd = view(x.to(dev()))
    # (the view case reaches the library as a non-contiguous tensor with contiguous samples: no copy in front of the kernel)
    assert case[5] is None or (not xd.is_contiguous() and xd.stride(-1) == 1)
    COUNTS["cells"] += 1
    try:
        first = _api_run(R, view(x.double()), [t.double() for t in taps], None, level, kw)
        leaves = [t.to(dtype) for t in first[5]]  # the library reconstructs the reference's coefficients, rounded to its dtype
        want = _api_run(R, view(x.double()), [t.double() for t in taps], [t.double() for t in leaves], level, kw)
    except Exception:
        COUNTS["skipped"] += 1
        with pytest.raises(Exception):
            _api_run(ptwt_amd, xd, [t.to(dev()) for t in taps], None, level, kw)
        return
    got = _api_run(ptwt_amd, xd, [t.to(dev()) for t in taps], [t.to(dev()) for t in leaves], level, kw)
    torch.cuda.synchronize()
    f64 = dtype == torch.float64
    v_tol, g_tol, t_tol = (VALUE_TOL[dtype], F64_TOL, F64_TOL) if f64 else (VALUE_TOL[dtype], F32_GRAD_TOL, F32_TAP_TOL)
    tag = str(dtype).split(".")[-1]
    assert len(got[0]) == len(want[0]) == level + 1
    for i, (a, b) in enumerate(zip(got[0], want[0])):
        assert a.dtype == dtype
        _check(a, b, v_tol, (name, tag, "coefficient", i), "swt values " + tag)
    _check(got[1], want[1], v_tol, (name, tag, "reconstruction"), "swt values " + tag)
    _check(got[2], want[2], g_tol, (name, tag, "d/dx"), "swt data gradients " + tag)
    for i, (a, b) in enumerate(zip(got[3], want[3])):
        _check(a, b, g_tol, (name, tag, "d/dcoefficient", i), "swt data gradients " + tag)
    for a, b, t, nme in zip(got[4], want[4], taps, TAPS):
        assert a.dtype == dtype and a.shape == t.shape
        _check(a, b, t_tol, (name, tag, "d/d" + nme), "swt tap gradients " + tag)


def test_swt_double_backward_vs_reference():
    """create_graph=True through a learnable stationary bank at an odd extent (the mixed data x taps second derivatives of
    ``_SwtLevelGrad`` / ``_IswtLevelGrad``) against the reference's own double backward, float64, at the 1e-9 of
    tests/test_host_logic.py::test_second_order_gradients_with_learnable_taps_vs_reference."""
    flen, level = 6, 2
    bank = random_bank(flen, 99)
    x = torch.randn(3, 1001, generator=torch.Generator().manual_seed(3), dtype=torch.float64)

    def second(mod, xx, taps):
        coeffs = mod.swt(xx, tuple(taps), level)
        f = sum((weight(t, i) * t.square()).sum() for i, t in enumerate(coeffs)) / 2
        y = mod.iswt(coeffs, tuple(taps))
        f = f + (weight(y, 7) * y.square()).sum() / 2
        first = torch.autograd.grad(f, [xx] + taps, create_graph=True)
        s = sum((gr * weight(gr, 11 + i)).sum() for i, gr in enumerate(first))
        return [t.detach() for t in first] + list(torch.autograd.grad(s, [xx] + taps))

    want = second(R, x.clone().requires_grad_(True), [torch.tensor(b).requires_grad_(True) for b in bank])
    got = second(ptwt_amd, x.to(dev()).requires_grad_(True), [torch.tensor(b, device=dev()).requires_grad_(True) for b in bank])
    for i, (a, b) in enumerate(zip(got, want)):
        _check(a, b, 1e-9, ("double backward", i), "swt second order float64")


def test_no_cell_was_skipped():
    """Runs last (file order): the share of skipped cells is zero."""
    assert COUNTS["cells"] >= 2 * len(CELLS) + 2 * len(API_CASES), "run the whole module"
    assert COUNTS["skipped"] == 0, COUNTS
    print("\nworst norm-wise errors vs the float64 references:", {k: "%.2e" % v for k, v in sorted(WORST.items())})


if __name__ == "__main__":
    measure_reference_f32()
