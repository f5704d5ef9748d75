"""GPU tests (``-m gpu``) of the fused 3-D stationary levels (csrc/mifwt_swt3.hip, kernel ids 36 / 37) and of ``ptwt_amd.swt3`` /
``iswt3`` against the float64 references of tests/_swt3_ref.py (composed from the 1-D stand-ins of tests/_oracle_engine.py, which
tests/test_torch_autograd_ref.py pins to the reference library's goldens).

1. Single level calls, ``stationary_transform._level3_fwd`` / ``_level3_inv``, on the same, already quantised, inputs.  A workgroup
   owns a tile of RT = 8 lattice rows (16: float32 synthesis up to 6 taps), a strip of 64 columns (128: float32 up to 4 taps) and a
   segment of lattice slices: volumes 1x1x1, 2x3x5, 1x7x9, 7x1x9, 7x9x1 (below a lane's run, single slices / rows / columns),
   5x17x65, 9x33x130, 33x8x64, 16x40x257, 70x9x66 (one past a strip, several strips, row tiles with tails, rows at and around the
   tile of 8) and 3x15x63, 2x16x128, 4x17x129 (rows and columns one below, at and one above the tile of 16 and the strips of 64 and
   128); every other cell runs with ``MIFWT_OPT_ROWS_PER_CHUNK`` = 3, which cuts the lattice slices into several segments with
   their warm-up; dilations 1, 2, 4, 8, 3 and, on the volumes whose every extent is below 64, 64; the lengths 2, 4, 8, 10
   (``mifwt_launch_count`` must show exactly one fused launch) and 20, 22, 34 (no fused instance: the composed route must have run,
   with the same bounds); banks of six INDEPENDENT random filters; 1 and 3 volumes; dense operands, slices of a larger tensor at an odd
   element offset, plane 0 / plane 5 of a level buffer and, for synthesis, eight operands with eight different stride sets; scales 1,
   1/8 and pi/7.  Synthesis inputs are random coefficient sets.  Every fused cell is also run on the composed route.
2. ``swt3`` / ``iswt3``: every returned tensor, the round trip, fused against composed, non-default axes and leading batch dims, the
   data gradients (of ``swt3`` w.r.t. the input, of ``iswt3`` w.r.t. every coefficient leaf) against float64 autograd of the torch
   reference, one float64 double backward, one case with the four taps as leaf tensors (composed route, four tap gradients).
3. Guard bands around output volumes embedded in a poisoned allocation; ``ptwt_amd.capture`` replays.

Bounds, norm-wise per band (``tests._golden.relerr``) with a max-abs companion of 10 x bound x the largest value, as
tests/test_gpu_swt2.py: float64 1e-12 (values) / 1e-10 (gradients, second order included); float32 values 1e-6.
The float32 GRADIENT bound comes from the reference alone: ``python -m tests.test_gpu_swt3`` runs the torch reference in float32 on
the host over API_CASES and prints its worst norm-wise error against its own float64 run on the same inputs — 1.05e-5 (the
2x5x9x33 db4 case; 7.7e-6 for 2x8x12x16 db11, 5.4e-6 for 8x12x20 sym5, 3.2e-6 and below elsewhere: the gradients w.r.t. the
approximation leaves are low-passed oscillating weights, sums that cancel; its worst VALUE error is 2.2e-7) — and the bound is ten
times that, because the GPU sums in another order: F32_GRAD_TOL = 1.05e-4.
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
from tests import _swt3_ref as R3

pytestmark = pytest.mark.gpu

VALUE_TOL = {torch.float64: 1e-12, torch.float32: 1e-6}
F64_GRAD_TOL = 1e-10
F32_GRAD_TOL = 1.05e-4  # 10 x the float32 reference's own worst data / coefficient gradient error (module docstring)
# worst norm-wise errors the module showed on the MI355X (printed by its last test)
WORST_ON_MI355X = {
    "level fwd fused float32": 1.30e-7, "level fwd fused float64": 3.21e-16, "level fwd composed float32": 1.77e-7, "level fwd composed float64": 4.68e-16,
    "level inv fused float32": 1.63e-7, "level inv fused float64": 3.87e-16, "level inv composed float32": 2.32e-7, "level inv composed float64": 5.43e-16,
    "swt3 values float32": 1.95e-7, "swt3 values float64": 5.51e-16, "swt3 composed float32": 1.95e-7, "swt3 composed float64": 5.51e-16,
    "swt3 round trip float32": 1.75e-7, "swt3 round trip float64": 6.86e-13,
    "swt3 data gradients float32": 1.04e-5, "swt3 data gradients float64": 2.30e-14,
    "swt3 second order float64": 4.43e-16, "swt3 tap gradients float64": 1.23e-15, "swt3 learnable values float64": 3.89e-16,
}

WORST = {}
COUNTS = {"cells": 0, "skipped": 0}
KEYS = R3.KEYS


def dev():
    return torch.device("cuda:0")


def weight(t, i):
    return torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64, device=t.device) + i).reshape(t.shape).to(t.dtype)


def random_bank(flen, seed):
    """Six independent filters of variance 1 / L, as tests/test_gpu_swt_kernels.py."""
    g = np.random.default_rng(5000 + seed)
    return [g.standard_normal(flen) / np.sqrt(flen) for _ in range(6)]


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
VOLUMES = [(1, 1, 1), (2, 3, 5), (1, 7, 9), (7, 1, 9), (7, 9, 1), (5, 17, 65), (9, 33, 130), (33, 8, 64), (16, 40, 257), (70, 9, 66),
           (3, 15, 63), (2, 16, 128), (4, 17, 129)]
SMALL_DILATIONS = (1, 2, 4, 8, 3)
BIG_DILATION = 64  # on the volumes whose every extent is below 64
FUSED_LENGTHS = (2, 4, 8, 10)
COMPOSED_LENGTHS = (20, 22, 34)
LENGTHS = FUSED_LENGTHS + COMPOSED_LENGTHS
SCALES = (1.0, 0.125, float(np.pi / 7))
LAYOUTS = ("contiguous", "slice", "plane", "mixed")
DTYPES = (torch.float32, torch.float64)
CHUNKS = (0, 3)  # MIFWT_OPT_ROWS_PER_CHUNK: the library's own segments / three lattice slices per segment


def _cells():
    """Not the full product: every volume meets every length, the other factors rotate through the cells; the dilation of 64 goes to the
    volumes whose every extent is below 64."""
    cells = []
    for dtype in DTYPES:
        for vi, (dz, h, w) in enumerate(VOLUMES):
            for li, flen in enumerate(LENGTHS):
                i = len(cells)
                dils = SMALL_DILATIONS + (BIG_DILATION,) if max(dz, h, w) < 64 else SMALL_DILATIONS
                cells.append((dtype, dz, h, w, flen, dils[(vi + li) % len(dils)], 1 if (vi + li) % 2 else 3, LAYOUTS[i % 4], SCALES[i % 3],
                              CHUNKS[(i // 4 + vi) % 2]))
    return cells


CELLS = _cells()


def _cell_id(c):
    return "%s-%dx%dx%d-L%d-D%d-B%d-%s-s%.3g-c%d" % (_name(c[0]), c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9])


def _operand(b, dz, h, w, layout, dtype, gen):
    """A [b, dz, h, w] operand with contiguous samples: dense; slices of larger tensors at an odd element offset; plane k of a
    [b, n, dz, h, w] buffer (``plane``: plane 0 of a level buffer, ``plane5``: its plane 5; ``k/n`` in general)."""
    def rnd(*shape):
        return torch.randn(*shape, generator=gen, dtype=torch.float64).to(dtype).to(dev())

    if layout == "contiguous":
        return rnd(b, dz, h, w)
    if layout in ("slice", "slice2"):
        pz, ph, pw = (1, 3, 7) if layout == "slice" else (2, 1, 5)
        big = rnd(b, dz + pz, h + ph, w + pw)
        c0 = pw - 3
        if ((pz * (h + ph) + ph - 1) * (w + pw) + c0) % 2 == 0:
            c0 -= 1
        t = big[:, pz:, ph - 1:ph - 1 + h, c0:c0 + w]
        assert t.storage_offset() % 2 == 1 and t.shape == (b, dz, h, w)
        return t
    if layout == "plane":
        return rnd(b, 8, dz, h, w)[:, 0]
    if layout == "plane5":
        return rnd(b, 8, dz, h, w)[:, 5]
    k, n = (int(v) for v in layout.split("/"))
    return rnd(b, n, dz, h, w)[:, k]


MIXED = ("slice", "plane5", "contiguous", "1/2", "2/4", "slice2", "1/3", "3/6")


def _run_cell(direction, cell):
    dtype, dz, h, w, flen, dilation, b, layout, scale, chunk = cell
    bank = random_bank(flen, 7 * flen + dz + h + w)
    taps = tuple(_quantised(t, dtype) for t in bank)
    (scale,) = _quantised([scale], dtype)
    gen = torch.Generator().manual_seed(flen * 100003 + 1009 * h + 31 * dz + w + dilation)
    if direction == "fwd":
        ops = [_operand(b, dz, h, w, "slice" if layout == "mixed" else layout, dtype, gen)]
        kid = st.KID_SWT3
    else:
        lay = MIXED if layout == "mixed" else ((layout,) * 3 + ("plane5",) + (layout,) * 4 if layout == "plane" else (layout,) * 8)
        ops = [_operand(b, dz, h, w, l, dtype, gen) for l in lay]
        if layout == "mixed" and min(dz, h, w) > 1:
            assert len({t.stride() for t in ops}) == 8
        kid = st.KID_ISWT3

    def call(composed):
        _engine.set_option(_engine.OPT_ROWS_PER_CHUNK, 0 if composed else chunk)
        try:
            if direction == "fwd":
                return st._level3_fwd(ops[0], taps, dilation, scale, composed=composed)
            return st._level3_inv(ops, taps, dilation, scale, composed=composed)
        finally:
            _engine.set_option(_engine.OPT_ROWS_PER_CHUNK, 0)

    keep = [t.clone() for t in ops]
    COUNTS["cells"] += 1
    host = [t.double().cpu().numpy() for t in ops]
    try:
        if direction == "fwd":
            want = np.stack(R3.level_fwd(host[0], taps, dilation, scale), axis=1)
        else:
            want = R3.level_inv(host, taps, dilation, scale)
    except Exception:
        COUNTS["skipped"] += 1
        with pytest.raises(Exception):
            call(False)
        return
    supported = bool(st._swt3_entries().mifwt_swt3_supported(_engine._DTYPE_IDS[dtype], flen, b, dz, h, w, dilation))
    assert supported == (flen in FUSED_LENGTHS), (flen, supported)
    n0 = _engine.launch_count(kid)
    got = call(False)
    torch.cuda.synchronize()
    ran = _engine.launch_count(kid) - n0
    assert ran == (1 if supported else 0), (_cell_id(cell), "fused launches", ran)
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
            assert res.shape == (b, 8, dz, h, w)
            for q, band in enumerate(R3.BANDS):
                _check(res[:, q], want[:, q], tol, (direction, route, _cell_id(cell), band), key)
        else:
            assert res.shape == (b, dz, h, w)
            _check(res, want, tol, (direction, route, _cell_id(cell)), key)


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_analysis_level_vs_float64_reference(cell):
    _run_cell("fwd", cell)


@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_synthesis_level_vs_float64_reference(cell):
    _run_cell("inv", cell)


def test_the_matrix_covers_what_it_claims():
    """(no GPU work) every value of every factor occurs in every dtype; the dilation of 64 meets the small volumes only; fused cells
    with several depth segments, wrapped windows, rows off the lattice and dilations beyond an extent exist."""
    for dtype in DTYPES:
        mine = [c for c in CELLS if c[0] == dtype]
        assert {(c[1], c[2], c[3]) for c in mine} == set(VOLUMES)
        assert {c[4] for c in mine} == set(LENGTHS)
        assert {c[5] for c in mine} == set(SMALL_DILATIONS) | {BIG_DILATION}
        assert {c[6] for c in mine} == {1, 3}
        assert {c[7] for c in mine} == set(LAYOUTS) and {c[8] for c in mine} == set(SCALES) and {c[9] for c in mine} == set(CHUNKS)
        assert all(max(c[1], c[2], c[3]) < 64 for c in mine if c[5] == BIG_DILATION)
        fused = [c for c in mine if c[4] in FUSED_LENGTHS]
        for flen in FUSED_LENGTHS:  # every fused length with both segmentations and on a volume of several strips
            assert {c[9] for c in fused if c[4] == flen} == set(CHUNKS)
            assert any(c[3] > 128 for c in fused if c[4] == flen)
        assert any(c[9] == 3 and -(-c[1] // c[5]) > 3 for c in fused)             # more lattice slices than one segment
        assert any(c[5] * c[4] > 2 * c[3] for c in fused)                          # windows that wrap several times
        assert any(c[2] % c[5] and c[5] < c[2] for c in fused) and any(c[1] % c[5] and c[5] < c[1] for c in fused)
        assert any(c[5] >= c[2] > 1 for c in fused) and any(c[5] >= c[1] > 1 for c in fused)
        assert any(-(-c[2] // c[5]) > 16 for c in fused)                            # more than one row tile, both tile heights


def test_level_calls_refuse_bad_lengths_and_take_empty_batches():
    x = torch.randn(2, 4, 8, 16, device=dev())
    for flen in (3, 130):
        taps = ([0.1] * flen,) * 6
        with pytest.raises(RuntimeError, match="libmifwt"):
            st._level3_fwd(x, taps, 1, 1.0)
        with pytest.raises(RuntimeError, match="libmifwt"):
            st._level3_inv((x,) * 8, taps, 1, 0.125)
    lib = st._swt3_entries()
    eight = st._vp8(*[x.data_ptr()] * 8)
    v8, s8, r8 = st._i64x8(*[512] * 8), st._i64x8(*[128] * 8), st._i64x8(*[16] * 8)
    t22 = st._taps6_array(([0.1] * 22,) * 6)
    # the C entries answer UNSUPPORTED (-2) where the query says no, and BADARG (-1) to odd lengths; nothing is launched
    n_f, n_i = _engine.launch_count(st.KID_SWT3), _engine.launch_count(st.KID_ISWT3)
    assert lib.mifwt_swt3_supported(0, 22, 2, 4, 8, 16, 1) == 0
    assert lib.mifwt_swt3_fwd(0, 22, 2, 4, 8, 16, 1, x.data_ptr(), 512, 128, 16, eight, v8, s8, r8, t22, 1.0, None) == -2
    assert lib.mifwt_swt3_inv(0, 22, 2, 4, 8, 16, 1, eight, v8, s8, r8, x.data_ptr(), 512, 128, 16, t22, 1.0, None) == -2
    assert lib.mifwt_swt3_fwd(0, 3, 2, 4, 8, 16, 1, x.data_ptr(), 512, 128, 16, eight, v8, s8, r8, t22, 1.0, None) == -1
    assert lib.mifwt_swt3_fwd(2, 8, 2, 4, 8, 16, 1, x.data_ptr(), 512, 128, 16, eight, v8, s8, r8, t22, 1.0, None) == -2
    torch.cuda.synchronize()
    assert (_engine.launch_count(st.KID_SWT3), _engine.launch_count(st.KID_ISWT3)) == (n_f, n_i)
    half = ((0.5, 0.5), (0.5, -0.5)) * 3
    for dtype in DTYPES:
        e = torch.empty(0, 4, 8, 16, device=dev(), dtype=dtype)
        assert st._level3_fwd(e, half, 1, 1.0).shape == (0, 8, 4, 8, 16)
        assert st._level3_inv((e,) * 8, half, 1, 0.125).shape == (0, 4, 8, 16)


# ---- 2. the public functions ----------------------------------------------------------------------------------------------------------
# (name, shape, wavelet, level, axes)
API_CASES = [
    ("2x16x24x40-db4-L2", (2, 16, 24, 40), "db4", 2, (-3, -2, -1)),
    ("8x12x20-sym5-auto", (8, 12, 20), "sym5", None, (-3, -2, -1)),
    ("axes(-1,-3,-2)-3x12x8x16-db2-L2", (3, 12, 8, 16), "db2", 2, (-1, -3, -2)),
    ("axes(0,2,4)-8x2x12x3x16-db3-L1", (8, 2, 12, 3, 16), "db3", 1, (0, 2, 4)),
    ("2x5x9x33-db4-L2", (2, 5, 9, 33), "db4", 2, (-3, -2, -1)),      # odd extents: slices, rows and columns wrap off the lattice
    ("2x8x12x16-db11-L2", (2, 8, 12, 16), "db11", 2, (-3, -2, -1)),  # 22 taps: no fused kernel, the composed route
]


def _flat(coeffs):
    return [coeffs[0]] + [c[k] for c in coeffs[1:] for k in KEYS]


def _nest(flat):
    return [flat[0]] + [dict(zip(KEYS, flat[1 + 7 * k:8 + 7 * k])) for k in range((len(flat) - 1) // 7)]


def _api_run(lib, x, wavelet, leaves, level, axes, dtype):
    """Coefficients, the reconstruction of given coefficient leaves, and the gradients of the ``weight`` loss w.r.t. the input and every
    leaf.  ``lib``: the library on the device, or the torch reference on the host in ``x``'s dtype."""
    x = x.detach().requires_grad_(True)
    if lib:
        c = _flat(ptwt_amd.swt3(x, wavelet, level, axes=axes))
    else:
        taps = [_quantised(t, dtype) for t in host_taps(wavelet)]
        c = _flat(R3.t_swt3(x, taps[0], taps[1], level, axes))
    if leaves is None:
        leaves = [t.detach().clone() for t in c]
    leaves = [t.detach().clone().requires_grad_(True) for t in leaves]
    y = ptwt_amd.iswt3(_nest(leaves), wavelet, axes=axes) if lib else R3.t_iswt3(_nest(leaves), taps[2], taps[3], axes)
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
        print("%-36s values %.2e  gradients %.2e" % (name, e_v, e_g))
        worst["values"], worst["gradients"] = max(worst["values"], e_v), max(worst["gradients"], e_g)
    print("worst:", {k: "%.2e" % v for k, v in worst.items()})
    return worst


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("case", API_CASES, ids=lambda c: c[0])
def test_swt3_iswt3_vs_reference(case, dtype):
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
    n_f, n_i = _engine.launch_count(st.KID_SWT3), _engine.launch_count(st.KID_ISWT3)
    got = _api_run(True, x.to(dev()), wavelet, [t.to(dev()) for t in leaves], level, axes, dtype)
    torch.cuda.synchronize()
    levels = (len(want[0]) - 1) // 7
    assert levels == (level if level is not None else min(R3.swt_max_level(shape[a]) for a in axes)) and levels >= 1
    # forward of each + backward of the other, per level: fused where the length has a kernel, none otherwise
    per = 2 * levels if flen <= 10 else 0
    assert _engine.launch_count(st.KID_SWT3) - n_f == per and _engine.launch_count(st.KID_ISWT3) - n_i == per
    v_tol, g_tol = VALUE_TOL[dtype], (F64_GRAD_TOL if dtype == torch.float64 else F32_GRAD_TOL)
    assert len(got[0]) == len(want[0])
    for i, (a, b) in enumerate(zip(got[0], want[0])):
        assert a.dtype == dtype and a.shape == x.shape
        _check(a, b, v_tol, (name, tag, "coefficient", i), "swt3 values " + tag)
    _check(got[1], want[1], v_tol, (name, tag, "reconstruction"), "swt3 values " + tag)
    _check(got[2], want[2], g_tol, (name, tag, "d/dx"), "swt3 data gradients " + tag)
    for i, (a, b) in enumerate(zip(got[3], want[3])):
        _check(a, b, g_tol, (name, tag, "d/dcoefficient", i), "swt3 data gradients " + tag)
    # the container, the round trip, and the composed route on the same call
    with torch.no_grad():
        xd = x.to(dev())
        coeffs = ptwt_amd.swt3(xd, wavelet, level, axes=axes)
        assert isinstance(coeffs, list) and isinstance(coeffs[0], torch.Tensor)
        assert all(isinstance(c, dict) and tuple(c.keys()) == KEYS for c in coeffs[1:])
        _check(ptwt_amd.iswt3(coeffs, wavelet, axes=axes), x, v_tol, (name, tag, "round trip"), "swt3 round trip " + tag)
        n_f, n_i = _engine.launch_count(st.KID_SWT3), _engine.launch_count(st.KID_ISWT3)
        st.FORCE_COMPOSED = True
        try:
            composed = ptwt_amd.swt3(xd, wavelet, level, axes=axes)
            rec = ptwt_amd.iswt3(_nest([t.to(dev()) for t in leaves]), wavelet, axes=axes)
        finally:
            st.FORCE_COMPOSED = False
        assert _engine.launch_count(st.KID_SWT3) == n_f and _engine.launch_count(st.KID_ISWT3) == n_i
        for i, (a, b) in enumerate(zip(_flat(composed), want[0])):
            _check(a, b, v_tol, (name, tag, "composed coefficient", i), "swt3 composed " + tag)
        _check(rec, want[1], v_tol, (name, tag, "composed reconstruction"), "swt3 composed " + tag)


def test_composed_cells_take_the_composed_route():
    """A (direction, dtype, length) cell listed in COMPOSED3_CELLS launches no fused kernel and gives the same level."""
    x = torch.randn(2, 6, 10, 70, generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dev())
    taps = tuple(_quantised(t, torch.float64) for t in random_bank(4, 1))
    fused = st._level3_fwd(x, taps, 2, 1.0)
    n_f = _engine.launch_count(st.KID_SWT3)
    st.COMPOSED3_CELLS.add(("fwd", torch.float64, 4))
    try:
        listed = st._level3_fwd(x, taps, 2, 1.0)
    finally:
        st.COMPOSED3_CELLS.discard(("fwd", torch.float64, 4))
    torch.cuda.synchronize()
    assert _engine.launch_count(st.KID_SWT3) == n_f
    _check(listed, fused, VALUE_TOL[torch.float64], "COMPOSED3_CELLS")


def test_swt3_double_backward_vs_reference():
    """create_graph=True through both transforms (each level op's backward is the other op), float64, odd extents."""
    wavelet, level = "db3", 2
    x = torch.randn(2, 6, 9, 20, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    taps = host_taps(wavelet)

    def second(lib, xx):
        coeffs = _flat(ptwt_amd.swt3(xx, wavelet, level) if lib else R3.t_swt3(xx, taps[0], taps[1], level))
        f = sum((weight(t, i) * t.square()).sum() for i, t in enumerate(coeffs)) / 2
        y = ptwt_amd.iswt3(_nest(coeffs), wavelet) if lib else R3.t_iswt3(_nest(coeffs), taps[2], taps[3])
        f = f + (weight(y, 7) * y.square()).sum() / 2
        (first,) = torch.autograd.grad(f, [xx], create_graph=True)
        s = (first * weight(first, 11)).sum()
        return [first.detach(), torch.autograd.grad(s, [xx])[0]]

    want = second(False, x.clone().requires_grad_(True))
    got = second(True, x.to(dev()).requires_grad_(True))
    for i, (a, b) in enumerate(zip(got, want)):
        _check(a, b, F64_GRAD_TOL, ("double backward", i), "swt3 second order float64")


def test_learnable_taps_take_the_composed_route():
    """The four taps as leaf tensors: no fused launch, and the four tap gradients (and the data gradient) match the reference."""
    flen, level = 6, 2
    bank = random_bank(flen, 99)[:4]
    x = torch.randn(2, 8, 12, 20, generator=torch.Generator().manual_seed(6), dtype=torch.float64)

    def run(lib, xx, taps):
        coeffs = ptwt_amd.swt3(xx, tuple(taps), level) if lib else R3.t_swt3(xx, taps[0], taps[1], level)
        y = ptwt_amd.iswt3(coeffs, tuple(taps)) if lib else R3.t_iswt3(coeffs, taps[2], taps[3])
        loss = sum((weight(t, i) * t).sum() for i, t in enumerate(_flat(coeffs))) + (weight(y, 7) * y.square()).sum()
        return [t.detach() for t in _flat(coeffs)] + [y.detach()], torch.autograd.grad(loss, [xx] + list(taps))

    want_v, want_g = run(False, x.clone().requires_grad_(True), [torch.tensor(b).requires_grad_(True) for b in bank])
    n_f, n_i = _engine.launch_count(st.KID_SWT3), _engine.launch_count(st.KID_ISWT3)
    got_v, got_g = run(True, x.to(dev()).requires_grad_(True), [torch.tensor(b, device=dev()).requires_grad_(True) for b in bank])
    torch.cuda.synchronize()
    assert _engine.launch_count(st.KID_SWT3) == n_f and _engine.launch_count(st.KID_ISWT3) == n_i
    for i, (a, b) in enumerate(zip(got_v, want_v)):
        _check(a, b, VALUE_TOL[torch.float64], ("learnable", "value", i), "swt3 learnable values float64")
    for a, b, what in zip(got_g, want_g, ("x", "dec_lo", "dec_hi", "rec_lo", "rec_hi")):
        assert a.shape == b.shape
        _check(a, b, F64_GRAD_TOL, ("learnable", "d/d" + what), "swt3 tap gradients float64")


# ---- 3. guard bands and graph capture ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_guard_bands_stay_untouched(dtype):
    """One analysis and one synthesis launch through the C ABI at 5 x 17 x 65, D = 2, 8 taps, three volumes, the output volumes embedded
    in a poisoned allocation (a guard slice above and below, two guard rows, five / six guard columns around every volume, guard
    volumes at both ends): every element outside the volumes still holds the pattern, every element inside is the reference's."""
    b, dz, h, w, flen, dilation, poison = 3, 5, 17, 65, 8, 2, -12345.5
    taps = tuple(_quantised(t, dtype) for t in random_bank(flen, 5))
    arr = st._taps6_array(taps)
    gen = torch.Generator().manual_seed(77)
    lib, did = st._swt3_entries(), _engine._DTYPE_IDS[dtype]
    dd, hh, ww = dz + 2, h + 4, w + 11
    for direction, nout in (("fwd", 8), ("inv", 1)):
        block = torch.full((nout * b + 2, dd, hh, ww), poison, dtype=dtype, device=dev())
        inside = torch.zeros_like(block, dtype=torch.bool)
        vols = [block[1 + q * b:1 + (q + 1) * b, 1:1 + dz, 2:2 + h, 5:5 + w] for q in range(nout)]
        for q in range(nout):
            inside[1 + q * b:1 + (q + 1) * b, 1:1 + dz, 2:2 + h, 5:5 + w] = True
        ins = [torch.randn(b, dz, h, w, generator=gen, dtype=torch.float64).to(dtype).to(dev()) for _ in range(9 - nout)]
        host = [t.double().cpu().numpy() for t in ins]
        guarded = (st._i64x8(*[dd * hh * ww] * 8), st._i64x8(*[hh * ww] * 8), st._i64x8(*[ww] * 8))
        dense = (st._i64x8(*[dz * h * w] * 8), st._i64x8(*[h * w] * 8), st._i64x8(*[w] * 8))
        stream = ctypes.c_void_p(_engine._stream_of(block))
        if direction == "fwd":
            rc = lib.mifwt_swt3_fwd(did, flen, b, dz, h, w, dilation, ins[0].data_ptr(), dz * h * w, h * w, w,
                                    st._vp8(*[v.data_ptr() for v in vols]), *guarded, arr, 1.0, stream)
            want = list(R3.level_fwd(host[0], taps, dilation, 1.0))
        else:
            rc = lib.mifwt_swt3_inv(did, flen, b, dz, h, w, dilation, st._vp8(*[t.data_ptr() for t in ins]), *dense,
                                    vols[0].data_ptr(), dd * hh * ww, hh * ww, ww, arr, 0.125, stream)
            want = [R3.level_inv(host, taps, dilation, 0.125)]
        assert rc == 0
        torch.cuda.synchronize()
        assert bool((block[~inside] == poison).all()), (direction, "a guard element was overwritten")
        for q in range(nout):
            _check(vols[q], want[q], VALUE_TOL[dtype], ("guarded", direction, _name(dtype), q))


def test_capture_replays_bit_identically():
    x = torch.randn(2, 8, 24, 80, generator=torch.Generator().manual_seed(8)).to(dev())
    fwd = ptwt_amd.capture(lambda t: ptwt_amd.swt3(t, "db4", level=2), x)
    x2 = torch.randn(2, 8, 24, 80, generator=torch.Generator().manual_seed(9)).to(dev())
    eager = _flat(ptwt_amd.swt3(x2, "db4", level=2))
    n_f = _engine.launch_count(st.KID_SWT3)
    replay = _flat(fwd(x2))
    torch.cuda.synchronize()
    assert _engine.launch_count(st.KID_SWT3) == n_f  # a replay enqueues nothing through the C ABI
    assert all(torch.equal(a, b) for a, b in zip(replay, eager)) and len(replay) == len(eager) == 15
    stacked = torch.stack(eager)
    inv = ptwt_amd.capture(lambda t: ptwt_amd.iswt3(_nest(list(t.unbind(0))), "db4"), stacked)
    other = torch.stack(_flat(ptwt_amd.swt3(x, "db4", level=2)))
    eager_y = ptwt_amd.iswt3(_nest(list(other.unbind(0))), "db4")
    assert torch.equal(inv(other), eager_y)
    _check(eager_y, x, VALUE_TOL[torch.float32], "captured round trip")


def test_no_cell_was_skipped():
    """Runs last (file order): the share of skipped cells is zero."""
    assert COUNTS["cells"] >= 2 * len(CELLS) + 2 * len(API_CASES), "run the whole module"
    assert COUNTS["skipped"] == 0, COUNTS
    print("\nworst norm-wise errors vs the float64 references:", {k: "%.2e" % v for k, v in sorted(WORST.items())})


if __name__ == "__main__":
    measure_reference_f32()
