"""GPU tests (``-m gpu``) of the kernels on batches whose buffers cross 2^31 elements and 2^32 bytes, against the float64 references of
the families' own modules.  Every kernel forms its addresses by hand — a batch index times an item stride, a row times a pitch, in
the buffer-resource kernels a 32-bit byte offset — and the rest of the suite stops at 2^30 float32 elements (exactly 2^32 bytes: no
offset reaches 2^32).  A wrapped offset does not crash: buffer loads return 0 and stores are dropped; the result is silently wrong.

The table (``CELLS``).  One cell = one call on a batch of SMALL items (planes of at most 128 x 128, rows of at most 4096, volumes of
32^3; the wave strips need 256 x 1030, the streaming kernels 1024 x 1024) chosen so
that the input buffer and every buffer the call writes hold just over 2^31 elements in float32 (2^29 in float64 = 2^32 bytes, 2^32 in
float16, 2^30 complex64 elements), ``tests/_large_ref.batch_over``.  Analysis and synthesis are cells of their own; a synthesis is fed
random coefficients (planes of ONE buffer [B, 4, M, M], as an analysis leaves them), not the image of an analysis.  Per cell:

1. the kernel ids of the call (``_engine.level_events``; ``_engine.launch_count`` for the stationary levels, which are enqueued
   outside the level launch path) are the ones the cell is about, on the whole batch and on every slice;
2. SAMPLED ITEMS against float64: items 0, 1, B - 2, B - 1, the item holding each of byte offsets 2^31 / 2^32 and element offsets
   2^31 / 2^32 of the input and of every output buffer with its two neighbours, eight items drawn with a fixed seed
   (``_large_ref.sample_items``, pinned on the CPU by tests/test_large_ref_host.py), copied back and compared item by item with the
   family's reference on the same (quantised) inputs;
3. EVERY ITEM against the same call on consecutive batch slices of at most 2^28 elements — the size the other modules pin —, per-item
   norm-wise error (``_large_ref.item_relerr``), slice by slice, freed as it goes: an item between the samples that was skipped or
   written to the wrong place shows here.

Bounds.  An item's result does not depend on the batch around it, so both checks use the family's EXISTING bound, imported from its
module, per item: ``TOL32`` / ``TOL64`` of tests/test_gpu_parity.py (norm-wise per sub-band) for the padded transforms, 5e-4 for
float16 storage (``F16_BOUNDS`` of tests/test_gpu_independent_banks.py), ``VALUE_TOL`` of tests/test_gpu_swt2.py and
tests/test_gpu_swt_kernels.py, ``F32_BOUNDS`` of tests/test_gpu_data_gradients.py, ``_value_tol`` / ``_tol`` of tests/test_gpu_per.py,
tests/test_gpu_ext.py and tests/test_gpu_cplx.py with the reference's own float32 error ``e_ref32`` of THAT item (check 3, which has
no reference: the rule's floor, 1e-6, the least it can give), and the element-wise bound and exact decisions of
tests/test_gpu_thresh.py (``check``; check 3: an element's result depends on that element and its threshold alone, so the whole batch
equals its slices bit for bit, ``torch.equal``); ``LEVEL_TOL`` / ``LEVEL_TOL32`` of tests/test_gpu_boundary_kernels.py and
tests/test_gpu_boundary3.py, ``tol`` of tests/test_gpu_boundary_packets.py, ``VALUE_TOL`` of tests/test_gpu_swt3.py.  Threshold gradients: the rule of ``test_gradients`` there — d/dx element-wise, d/dv within
``(15 + R + 1) eps32 sum |term|`` of the float64 sum over slices.  No bound is new and none is fitted to a kernel's output.

The audit (read before the first run: every product that forms an offset or a grid size; "i64" = the product is formed in int64_t):
  7    csrc/mifwt_dwt2_tile.h: image base ``(int64_t)img * xs_b`` (tile_image_offset), band base ``(int64_t)img * os_b[s]``; in-image
       offsets int / uint32 bytes behind ``span < 2^29`` and ``coef_extent[0] * stride < 2^31`` (dwt2_fwd_tile_supported,
       mifwt_compose.hip); grid ``ntiles <= INT32_MAX / 8`` (launch_tile).
  8    csrc/mifwt_idwt2_tile.h: ``(int64_t)img * is_b[s]``, ``(int64_t)img * ys_b + (int64_t)yr * ys_h``; spans < 2^29
       (dwt2_inv_tile_supported); ``ntiles <= INT32_MAX / 8``.
  20   csrc/mifwt_dwt2_fwd_small.hip: ``int64_t img`` loop, ``img * xs_b``, ``img * ds_b[l]``, ``img * as_b``; in-image uint32 behind
       ``sig_extent[0] * sig_stride[1] < 2^30`` and ``coef_extent[0] * stride < 2^29`` (small_plan); batch <= 2^30.
  21   csrc/mifwt_dwt2_inv_small.hip: ``int64_t img``, ``img * det_b[l]``, ``img * aa_b``, ``img * ys_b``; planes <= 4096^2, batch <= 2^30.
  14   csrc/mifwt_dwt1_tail.hip: ``const int64_t row = blockIdx.x``, ``row * x_rs`` / ``det_rs`` / ``approx_rs``; rows <= 2^30 = the grid.
  15   same file: ``row * approx_rs`` / ``y_rs`` / ``det_rs``.
  17   csrc/mifwt_dwt1_long.hip: ``(int64_t)row * x_rs`` etc.; rows <= 2^24, ``rows * (nchunks + 1) <= 2^30`` (long_plan).
  18   same file: ``(int64_t)row * approx_rs`` / ``y_rs`` / ``det_rs``; ``rows * nchunks <= 2^30`` (inv_long_plan).
  38/39 csrc/mifwt_per.hip: ``(int64_t)b * sig_bs``, ``(int64_t)gr * sig_rs``; the band offsets ``(int64_t)b * a_bs + (int64_t)m * a_rs``
       in ``store_bands``, ``grid <= INT32_MAX`` in ``cut_tiles`` and ``tiles <= INT32_MAX`` in ``fused_envelope`` (csrc/mifwt_level_tile.h,
       shared by 26/27, 38/39, 42/43 and 46/47).
  42/43 csrc/mifwt_ext.hip: the same forms in the staging and in the adjoint kernels, the same shared pieces.
  46/47 csrc/mifwt_cplx.hip: the same forms in complex elements in its own kernels; ``cut_tiles`` / ``fused_envelope`` shared.
  48/49 csrc/mifwt_thresh.hip: rows through ``i0 * xs0 + i1 * xs1`` with int64 ``i0``, ``i1``; columns int64; units, rows < 2^31 and
       ``n <= 2^30`` (seg_geometry) — THE DEFECT: ``thresholding._collapse`` merged a dense tensor into one row, so any dense tensor of
       more than 2^30 elements raised ``libmifwt: valid request this build has no kernel for``.  Fixed in ``_collapse`` (the row is cut back
       into equal rows, ``_split_row``); the dense cell below runs on kernel 48.  Partial sums ``part[(size_t)k * total + u]``.
  16   csrc/mifwt_dwt2_fwd_pyr.hip: ``(int64_t)img * xs_b`` / ``ds_b[l]`` / ``as_b``; rows of the batch laid end to end in uint32
       behind ``batch * HN < 2^31`` (line 1166); in-image byte offsets behind ``lim = 2^29`` elements (line 1331).
  22   csrc/mifwt_dwt2_inv_pyr.hip: ``(int64_t)img * bs_b`` (line 333), ``(int64_t)img * ys_b`` (line 465); ``nwg <= INT32_MAX / 8``.
  1/2  csrc/mifwt_dwt2_fwd.hip / mifwt_dwt2_inv.hip: ``(int64_t)img * xs_b``, ``(int64_t)img * os_b[s] + (int64_t)j0 * os_h[s]``,
       ``(int64_t)img * ys_b + (int64_t)y0 * ys_h``; ``ntasks <= INT32_MAX / 8``; spans < 2^29.
  12/13 csrc/mifwt_dwt2_fwd_pair.hip / mifwt_idwt2_pair.hip: ``(int64_t)img *`` every batch stride; ``ntiles <= INT32_MAX / 8``.
  0    csrc/mifwt_generic.hip: ``int64_t idx`` grid-stride loop over ``g.total``, int64 coordinates times int64 strides throughout.
  3/4  csrc/mifwt_axis_stream.h: ``int64_t task``, ``(int64_t)b * in0_s[0] + j0``, ``(int64_t)src * in0_s[1]`` (outer axis); rows form:
       ``i0 * in0_s[0]`` with int64 strides, ``nrows <= INT32_MAX / 2``, ``n <= INT32_MAX / 4``, ``nblk <= INT32_MAX``.
  40/41 csrc/mifwt_per.hip, per_axis_kernel: ``int64_t idx`` grid-stride loop over ``outer * len * inner`` (int64), ``o * sig_s[0]``,
       ``(int64_t)pos * lo_s[1]``, ``in * sig_s[2]`` with int64 strides; ``n <= INT32_MAX / 4`` (per_axis), at most 65536 blocks.
  44/45 csrc/mifwt_ext.hip, ext_axis_kernel: the same loop and products; ``n <= INT32_MAX / 4`` (``fill_axis_args``, mifwt_level_tile.h,
       for 28/29, 40/41 and 44/45).
  26/27 csrc/mifwt_bwt.hip: ``(int64_t)b * sig_bs``, ``(int64_t)gr * sig_rs``, ``(int64_t)b * a_bs + (int64_t)m * a_rs``;
       ``coef_extent <= 2^29``, ``tiles <= INT32_MAX`` (``fused_envelope``), ``grid <= INT32_MAX`` (``cut_tiles``).
  28/29 same file, bwt_axis_generic: ``int64_t idx`` over ``outer * len * inner``, ``(int64_t)j * sig_s[1]``, table rows
       ``(int64_t)r * L + k``; ``n <= INT32_MAX / 4`` (``fill_axis_args``), at most 8192 blocks.
  30/31 csrc/mifwt_bwt3.hip: ``(int64_t)b * sig_bs``, ``(int64_t)md * a_ds + (int64_t)mr * a_rs`` (lines 152, 232-233, 269-270, 329);
       ``coef_extent <= 2^29``, ``tiles <= INT32_MAX``, ``grid <= INT32_MAX`` (lines 365-367, 414).
  32/33 csrc/mifwt_bwt_tree.hip: ``const int64_t row = blockIdx.x``, ``row * in_rs``, ``row * n`` (lines 74-79, 124-129);
       ``rows <= INT32_MAX`` = the grid (line 256).
  34/35 csrc/mifwt_swt2.hip: ``int64_t task``, ``int64_t img = task / nres``, ``(int64_t)row * in_rs[q]``; ``nblk <= INT32_MAX``;
       csrc/mifwt_swt.hip (1-D, no id): ``int64_t task``, ``(int64_t)row * in0_rs`` / ``out0_rs``.
  36/37 csrc/mifwt_swt3.hip: ``int64_t task = blockIdx.x`` split into strip / tile / segment / residues, ``int64_t vol``,
       ``vol * in_vs[q]`` (lines 97-141), ``(int64_t)slice * in_ss[q] + (int64_t)row * in_rs[q]`` (line 176); every extent and
       ``dilation * L`` at most INT32_MAX / 8 (swt3_extents_ok), ``nblk <= INT32_MAX`` (line 396).
  taps csrc/mifwt_tapgrad.hip: ``int64_t idx`` over ``rows * m_len`` in the generic kernel; the wave kernels walk ``uint32_t task`` behind
       ``rows * chunks < 2^31`` (line 237), ``ntasks < 2^31`` (lines 292, 320); operands ``(int64_t)bat * a_bs + (int64_t)rin * a_rs``;
       extents at most INT32_MAX / 4 (lines 233, 315); sums in double.
  9/10 csrc/mifwt_dwt3_fwd_tile.hip / mifwt_dwt3_inv_tile.hip: ``(int64_t)img * xs_b`` / ``os_b[b]`` / ``is_b[s]`` / ``ys_b``, in-volume
       ``(int64_t)z * os_d + (int64_t)y * os_h``; volume bytes formed in int64 behind the span guards; ``ntiles``, ``nblk <= INT32_MAX / 8``.
  24/25 csrc/mifwt_dwt3_fwd_walk.hip / mifwt_dwt3_inv_walk.hip: ``(int64_t)img * xs_b`` / ``os_b`` / ``is_b[k]`` / ``ys_b``; ``nblk <= INT32_MAX / 8``.
  5/6  csrc/mifwt_compose.hip: the depth slices of all volumes as ONE 2-D batch (``batch * depth`` images through the tiles'
       ``tile_image_offset``, int64) plus the streaming axis pass along the depth (3 / 4); int64 host arithmetic throughout.
  border csrc/mifwt_adjoint_border.hip: ``const int64_t img = a.img0 + blockIdx.y`` (launches of 32768 images: grid.y is 16 bits),
       ``img * as[0] + k0 * as[1]`` and ``img * xs[0] + (int64_t)c * xs[1 + o]`` in int64.
No 32-bit product that a cell overflows was found in these kernels: the one defect is the threshold refusal above.

Cells whose coarser or smaller buffers cannot pass the mark below 64 GiB list them as ``minor`` (the second level of 12 / 13, the
deeper levels of 16 / 22, the input of a stationary level, which writes four times as much): they are sampled all the same.  16 / 22
run 2051 x 1024 x 1024 at level 3 without the eight random items.  The backward legs (own tests below): ``wavedec2`` in "symmetric"
(synthesis tiles 8 + the adjoint-border kernel), ``waverec2`` (analysis tiles 7), ``threshold`` soft with a learnable one-element
threshold (49 + the reduction launch), against float64 autograd on the sampled leaf and cotangent slices with the bounds of
tests/test_gpu_data_gradients.py / tests/test_gpu_thresh.py; and the tap gradients of a learnable db2 bank in 1-D and 2-D
(csrc/mifwt_tapgrad.hip) against the float64 sum of per-slice tap gradients under the rule of tests/test_gpu_learnable_lengths.py.

Regime HUGE (``HUGE``, ``test_huge_item``, ``test_huge_threshold``, ``test_huge_rows_of_the_longest_extent``): ONE item at the in-item
guards, level 1, where row x pitch inside the item leaves an ``int``.  Two sizes per family, analysis and synthesis each: 23170 x 23170
(the last square whose span is below the tiles' 2^29 elements, csrc/mifwt_compose.hip:110) and 46341 x 46349 (46342 x 46350 for the
circular levels), more than 2^31 elements.  The tiles 7 / 8 run inside (``MIFWT_OPT_TILE_MODE`` 1; by default a synthesis of 2^20
samples and more goes to the wave strips, which have cells of their own there) and hand over to the axis / generic passes 3 / 4 / 0
past the span.  Periodization 38 / 39, "smooth" 42 / 43, complex64 46 / 47, the boundary wavelets 26 / 27 and swt2 34 / 35 have NO
span guard — their launchers refuse ``coef_extent > 2^29`` per axis and more than INT32_MAX tiles, which no item behind ``validate``'s
INT32_MAX / 4 samples per axis reaches — so the fused id is asserted on both sides and the second size is where its 64-bit row offsets
are proved; their fallbacks 40 / 41, 44 / 45, 28 / 29 are reached by switch in regime MANY only.  ``threshold``: 2^30 elements (the
longest row) and 46341 x 46349 (three rows).  1-D: five rows of INT32_MAX / 4 samples at level 2 on 17 / 18 (the chunked kernels fuse
two levels and more; a single level of such rows takes the axis passes); one sample more is the refusal pinned below.
The window reference (``_large_ref.window_starts`` / ``window_reference``, pinned on the CPU for every family against the family's
reference on whole planes): windows of 96 x 96 at the four corners, the four edge midpoints, the centre and the rows where row x pitch
of the input or the output crosses 2^29, 2^30 and 2^31 elements; for each the crop of the input the window depends on (filter support
plus a guard) is copied back and the family's float64 single-level reference applied to it — a crop clipped at a true end keeps the
whole item's border handling there (index-map modes, the value-map mode, the boundary filters alike), a circular level's crop
continues on the other side, and only the window, which lies a guard inside every artificial end, is compared, at the family's bound.

Memory: a forward cell holds input + output (11 - 36 GiB) plus one slice; the backward legs 40 - 59 GiB in a run of the whole module.  A cell skips only when
``torch.cuda.mem_get_info`` shows less than it needs; the recorded run on the MI355X shows no skip.  Data: ``normal_()`` on the device
from a seeded generator.  ``WORST_ON_MI355X`` is a record of that run (printed when the module's last test has run), not a bound.
"""
import contextlib
from collections import namedtuple

import numpy as np
import pytest
import torch

import ptwt_amd
from oracle import fwt_oracle as O
from oracle import torch_autograd_ref as A
from ptwt_amd import _bwt, _cplx, _engine, _ext, _per
from ptwt_amd import stationary_transform as st
from ptwt_amd._wavelets import host_taps
from tests import _boundary_ref as BR
from tests import _boundary_tree_ref as BT
from tests import _cplx_ref as RC
from tests import _ext_ref as RE
from tests import _large_ref as L
from tests import _oracle_engine as OE
from tests import _per_ref as RP
from tests import _swt2_ref as R2
from tests import _swt3_ref as R3
from tests import _thresh_ref as RT
from tests import test_gpu_boundary3 as TB3
from tests import test_gpu_boundary_kernels as TBK
from tests import test_gpu_boundary_packets as TBP
from tests import test_gpu_cplx as TC
from tests import test_gpu_data_gradients as TG
from tests import test_gpu_ext as TE
from tests import test_gpu_independent_banks as TB
from tests import test_gpu_learnable_lengths as TLL
from tests import test_gpu_parity as TP
from tests import test_gpu_per as TPER
from tests import test_gpu_swt2 as TS2
from tests import test_gpu_swt3 as TS3
from tests import test_gpu_swt_kernels as TSK
from tests import test_gpu_thresh as TH

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f16, f32, f64, c64 = torch.float16, torch.float32, torch.float64, torch.complex64
#: elements a cell's buffers must exceed, per dtype (module docstring)
MARK = {f32: 1 << 31, f64: 1 << 29, f16: 1 << 32, c64: 1 << 30}
PADDED_TOL = {f32: TP.TOL32, f64: TP.TOL64, f16: TB.F16_BOUNDS["norm"]}
NO_SMALL = ((_engine.OPT_PYRAMID_MODE, 2),)  # (neither the small-plane kernels 20 / 21 nor the one-level form of 16 / 22: the tiles)
NO_TILES = ((_engine.OPT_TILE_MODE, 2), (_engine.OPT_PYRAMID_MODE, 2))  # (the option set of tests/test_gpu_independent_banks.py: the strips)
FORCE_GENERIC = ((_engine.OPT_FORCE_GENERIC, 1),)
WALK4 = ((_engine.OPT_TILE_MODE, 4),)  # (the 3-D walking kernels 24 / 25 whatever the volume)
# worst errors of this module on an MI355X relative to the bound in force (printed by its last test); a record, not a bound
WORST_ON_MI355X = {
    "7/8 tiles f32": (0.100, 0.084), "7/8 tiles f64": (1.8e-4, 1.6e-4), "7/8 tiles f16": (0.434, 0.421), "20/21 small planes": (0.100, 0.080),
    "16/22 streaming": (0.184, 0.097), "1/2 wave strips": (0.098, 0.083), "12/13 pair": (0.142, 0.095), "0 generic passes": (0.101, 0.084),
    "3/4 axis passes f64 18 taps": (3.1e-4, 2.8e-4), "3/4 rows": (0.075, 0.063), "14/15 one workgroup per row": (0.095, 0.076),
    "17/18 chunked rows": (0.105, 0.074), "38/39 periodization float32": (0.083, 0.077), "38/39 periodization float64": (2.2e-4, 2.0e-4),
    "42/43 smooth": (0.167, 0.238), "46/47 complex64": (0.096, 0.084), "34/35 swt2": (0.073, 0.094), "swt": (0.060, 0.075),
    "9/10 bricks": (0.091, 0.083), "24/25 walk": (0.090, 0.081), "5/6 composed": (0.141, 0.118),
    "40/41 periodization axis passes": (0.037, 0.036), "44/45 smooth axis passes": (0.035, 0.045), "26/27 boundary planes": (0.076, 0.075),
    "28/29 boundary axis passes": (0.037, 0.037), "30/31 boundary volumes": (0.096, 0.086), "32/33 packet subtree": (0.034, 0.035),
    "36/37 swt3": (0.096, 0.121),
    "backward wavedec2": 0.021, "backward waverec2": 0.015,
    "49 threshold gradient": 3.3e-8,  # (error 2.8e-5 of a gradient of 1.9e4, over the bound 8.7e2)
    "tap gradients 1-D": 0.152, "tap gradients 2-D": 0.544,  # (worst of the four filters: 9.1e-7 and 3.3e-6 norm-wise, of 6e-6)
    "every cell, whole batch against its slices": 0.0,  # (bit-identical)
}  # (analysis, synthesis) of the sampled items
WORST = {}

Cell = namedtuple("Cell", "name kids dtype strides make call sample every opts scope seed minor counted nrandom")


def _up(t):
    return t.to(torch.complex128 if t.is_complex() else torch.float64)


def _fill(shape, dtype, gen, scale=1.0):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    if dtype.is_complex:
        torch.view_as_real(t).normal_(generator=gen)
    else:
        t.normal_(generator=gen)
    return t.mul_(scale) if scale != 1.0 else t


def _record(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))


# ---- the two checks, norm-wise form -----------------------------------------------------------------------------------------------
def normwise_sample(ref, tol, relerr=None):
    """Check 2 of the module docstring for a family with a norm-wise bound: ``ref(list of float64 item inputs [n, ...])`` -> list of
    float64 outputs; ``tol(item inputs [1, ...])`` -> the bound of that item's outputs; ``relerr(got, want, scale)``."""
    def run(cell, items, xs, gots):
        want = ref([_up(x) for x in xs])
        assert len(want) == len(gots), (cell.name, len(want), len(gots))
        for j, item in enumerate(items):
            mine = [_up(x[j:j + 1]) for x in xs]
            bound = tol(mine)
            scale = float(torch.cat([m.reshape(-1) for m in mine]).norm())
            for k, (g, w) in enumerate(zip(gots, want)):
                assert tuple(g.shape) == tuple(w.shape), (cell.name, k, g.shape, w.shape)
                err = relerr(_up(g[j]), w[j], scale) if relerr else TP.G.relerr(_up(g[j]).numpy(), w[j].numpy())
                _record(cell.name, err / bound)
                assert err < bound, f"{cell.name}: item {item} output {k}: {err:.3e} >= {bound:.3e}"
    return run


def normwise_every(tol):
    """Check 3 for a family with a norm-wise bound ``tol`` (a number)."""
    def run(cell, k, whole, part, inputs, start):
        err = L.item_relerr(whole, part)
        worst = float(err.max())
        _record(cell.name + " slices", worst / tol)
        assert worst < tol, f"{cell.name}: output {k}, item {start + int(err.argmax())} whole batch against its slice: {worst:.3e} >= {tol:.3e}"
    return run


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def _traced(cell, inputs):
    """The call, with the route asserted: the kernel ids of its launches (``_engine.level_events``), and for entries outside the
    level launch path (``cell.counted``: kernel id -> launches per call) the library's launch counters."""
    before = {k: _engine.launch_count(k) for k, _ in cell.counted}
    _engine.level_events = []
    try:
        outs = cell.call(inputs)
        kids = {e[1] for e in _engine.level_events}
    finally:
        _engine.level_events = None
    assert kids == set(cell.kids), (cell.name, "kernel ids", sorted(kids), "expected", sorted(cell.kids))
    ran = {k: _engine.launch_count(k) - n for k, n in before.items()}
    assert ran == dict(cell.counted), (cell.name, "launches", ran, "expected", dict(cell.counted))
    return outs


def run_cell(cell):
    batch = L.batch_over(MARK[cell.dtype], cell.strides)
    esz = torch.empty((), dtype=cell.dtype).element_size()
    need = (sum(cell.strides + cell.minor) * batch * esz) * (1 + 2 * L.SLICE_ELEMENTS / MARK[cell.dtype]) + (4 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{cell.name}: {need / 2 ** 30:.1f} GiB needed, {free / 2 ** 30:.1f} GiB free")
    torch.cuda.reset_peak_memory_stats()
    for key, value in cell.opts:
        _engine.set_option(key, value)
    try:
        with cell.scope():
            _drive(cell, batch)
    finally:
        for key, _ in cell.opts:
            _engine.set_option(key, 0)
        torch.cuda.empty_cache()
    print(f"{cell.name}: batch {batch}, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB, worst / bound "
          f"{WORST.get(cell.name, 0.0):.3f} (samples) {WORST.get(cell.name + ' slices', 0.0):.3f} (slices)")


def _drive(cell, batch):
    gen = torch.Generator(device=DEV).manual_seed(cell.seed)
    inputs = cell.make(batch, gen)
    outs = _traced(cell, inputs)
    assert all(t.shape[0] == batch for t in inputs + outs)
    buffers = sorted({(t.stride(0), t.element_size()) for t in inputs + outs if t.stride(0) > 1})
    for stride, _ in buffers:  # every buffer is past the mark, as the table says (but those it lists as minor)
        assert stride in cell.strides + cell.minor and (stride in cell.minor or stride * batch > MARK[cell.dtype]), (cell.name, stride)
    items = L.sample_items(batch, buffers, cell.seed, cell.nrandom)
    assert len(items) <= 64
    idx = torch.tensor(items, device=DEV)
    cell.sample(cell, items, [t.index_select(0, idx).cpu() for t in inputs], [t.index_select(0, idx).cpu() for t in outs])
    for start, stop in L.batch_slices(batch, max(cell.strides + cell.minor)):
        part_in = [t[start:stop] for t in inputs]
        part = _traced(cell, part_in)
        for k, (w, p) in enumerate(zip(outs, part)):
            cell.every(cell, k, w[start:stop], p, part_in, start)
        del part
    del outs, inputs


# ---- the families ----------------------------------------------------------------------------------------------------------------
CELLS = []


def cell(name, kids, dtype, strides, make, call, sample, every, opts=(), scope=contextlib.nullcontext, seed=None, minor=(), counted=(),
         nrandom=8):
    """``strides``: the item strides of the buffers that must pass the mark; ``minor``: those of buffers that cannot at a batch that
    keeps the cell below 64 GiB (the coarser level of a two-level call, the input of a stationary level that writes four times as
    much) — they still cross 2^31 or 2^32 bytes where the figures in EXPERIMENTS.md say so."""
    CELLS.append(Cell(name, kids, dtype, tuple(strides), make, call, sample, every, tuple(opts), scope, 9000 + len(CELLS) if seed is None else seed,
                      tuple(minor), tuple(counted), nrandom))


def _flat2(coeffs):
    return [coeffs[0], *coeffs[1]]


def padded2d(name, kid_fwd, kid_inv, dtype, wavelet, mode, shape, opts=(), scope=contextlib.nullcontext):
    """``wavedec2`` / ``waverec2`` at level 1 on planes of ``shape``: the analysis of a random batch; the synthesis of random bands that
    are the planes of one buffer [B, 4, Mh, Mw]."""
    flen = len(host_taps(wavelet)[0])
    h, w = shape
    mh, mw = (h + flen - 1) // 2, (w + flen - 1) // 2
    ho, wo = 2 * mh - flen + 2, 2 * mw - flen + 2
    tol = PADDED_TOL[dtype]

    def ref_fwd(xs):
        return [torch.from_numpy(np.ascontiguousarray(t)) for t in _flat2(O.wavedec2(xs[0].numpy(), wavelet, mode=mode, level=1))]

    def ref_inv(xs):
        a, h, v, d = (t.numpy() for t in xs)
        return [torch.from_numpy(np.ascontiguousarray(O.waverec2([a, (h, v, d)], wavelet)))]

    cell(f"{name} wavedec2", {kid_fwd}, dtype, (h * w, 4 * mh * mw), lambda b, gen: [_fill((b, h, w), dtype, gen)],
         lambda xs: _flat2(ptwt_amd.wavedec2(xs[0], wavelet, mode=mode, level=1)),
         normwise_sample(ref_fwd, lambda mine: tol), normwise_every(tol), opts, scope)
    cell(f"{name} waverec2", {kid_inv}, dtype, (4 * mh * mw, ho * wo), lambda b, gen: list(_fill((b, 4, mh, mw), dtype, gen).unbind(1)),
         lambda xs: [ptwt_amd.waverec2([xs[0], tuple(xs[1:])], wavelet)],
         normwise_sample(ref_inv, lambda mine: tol), normwise_every(tol), opts, scope)


def padded2d_pair(name, wavelet, mode, n, opts):
    """Two levels per launch (12 / 13): ``wavedec2`` / ``waverec2`` at level 2 without a graph, float32.  The first level's buffer holds
    its three detail planes [B, 3, M1, M1]; the second level's [B, 4, M2, M2] is a quarter of it (minor)."""
    flen = len(host_taps(wavelet)[0])
    m1 = (n + flen - 1) // 2
    m2 = (m1 + flen - 1) // 2
    n_out = 2 * m1 - flen + 2
    tol = PADDED_TOL[f32]

    def flat(c):
        return [c[0], *c[1], *c[2]]

    def ref_fwd(xs):
        return [torch.from_numpy(np.ascontiguousarray(t)) for t in flat(O.wavedec2(xs[0].numpy(), wavelet, mode=mode, level=2))]

    def ref_inv(xs):
        t = [x.numpy() for x in xs]
        return [torch.from_numpy(np.ascontiguousarray(O.waverec2([t[0], tuple(t[1:4]), tuple(t[4:7])], wavelet)))]

    def make_inv(b, gen):
        return [*_fill((b, 4, m2, m2), f32, gen).unbind(1), *_fill((b, 3, m1, m1), f32, gen).unbind(1)]

    cell(f"{name} wavedec2", {12}, f32, (n * n, 3 * m1 * m1), lambda b, gen: [_fill((b, n, n), f32, gen)],
         lambda xs: flat(ptwt_amd.wavedec2(xs[0], wavelet, mode=mode, level=2)),
         normwise_sample(ref_fwd, lambda mine: tol), normwise_every(tol), opts, minor=(4 * m2 * m2,))
    cell(f"{name} waverec2", {13}, f32, (3 * m1 * m1, n_out * n_out), make_inv,
         lambda xs: [ptwt_amd.waverec2([xs[0], tuple(xs[1:4]), tuple(xs[4:7])], wavelet)],
         normwise_sample(ref_inv, lambda mine: tol), normwise_every(tol), opts, minor=(4 * m2 * m2,))


def padded1d_level(name, kid_fwd, kid_inv, wavelet, mode, n):
    """ONE 1-D level (the streaming axis passes 3 / 4 on rows): [B, n] -> the planes of [B, 2, M], float32."""
    flen = len(host_taps(wavelet)[0])
    m = (n + flen - 1) // 2
    tol = PADDED_TOL[f32]
    cell(f"{name} wavedec", {kid_fwd}, f32, (n, 2 * m), lambda b, gen: [_fill((b, n), f32, gen)],
         lambda xs: list(ptwt_amd.wavedec(xs[0], wavelet, mode=mode, level=1)),
         normwise_sample(lambda xs: [torch.from_numpy(np.ascontiguousarray(t)) for t in O.wavedec(xs[0].numpy(), wavelet, mode=mode, level=1)],
                         lambda mine: tol), normwise_every(tol))
    cell(f"{name} waverec", {kid_inv}, f32, (2 * m, 2 * m - flen + 2), lambda b, gen: list(_fill((b, 2, m), f32, gen).unbind(1)),
         lambda xs: [ptwt_amd.waverec(list(xs), wavelet)],
         normwise_sample(lambda xs: [torch.from_numpy(np.ascontiguousarray(O.waverec([t.numpy() for t in xs], wavelet)))], lambda mine: tol),
         normwise_every(tol))


def streaming2d(wavelet="db4", mode="symmetric", n=1024, level=3):
    """Three levels per launch through the streaming kernels 16 / 22, which need planes at least 896 wide: 2051 x 1024 x 1024, sized by
    the plane batch (the level buffers [B, 3, 515, 515], [B, 3, 261, 261] and [B, 4, 134, 134] are minor: the first crosses 2^32 bytes);
    no random items (each costs a three-level float64 reference of a 1024 x 1024 plane)."""
    flen = len(host_taps(wavelet)[0])
    ms = [n]
    for _ in range(level):
        ms.append((ms[-1] + flen - 1) // 2)
    minor = tuple((4 if l == level else 3) * ms[l] * ms[l] for l in range(1, level + 1))
    tol = PADDED_TOL[f32]

    def flat(c):
        return [c[0], *[t for lv in c[1:] for t in lv]]

    def nest(ts):
        return [ts[0], *[tuple(ts[1 + 3 * i:4 + 3 * i]) for i in range(level)]]

    def make_inv(b, gen):
        coarse = _fill((b, 4, ms[level], ms[level]), f32, gen)
        return [*coarse.unbind(1), *[t for l in range(level - 1, 0, -1) for t in _fill((b, 3, ms[l], ms[l]), f32, gen).unbind(1)]]

    cell("16/22 streaming wavedec2", {16}, f32, (n * n,), lambda b, gen: [_fill((b, n, n), f32, gen)],
         lambda xs: flat(ptwt_amd.wavedec2(xs[0], wavelet, mode=mode, level=level)),
         normwise_sample(lambda xs: [torch.from_numpy(np.ascontiguousarray(t)) for t in flat(O.wavedec2(xs[0].numpy(), wavelet, mode=mode, level=level))],
                         lambda mine: tol), normwise_every(tol), minor=minor, nrandom=0)
    cell("16/22 streaming waverec2", {22}, f32, (n * n,), make_inv, lambda xs: [ptwt_amd.waverec2(nest(list(xs)), wavelet)],
         normwise_sample(lambda xs: [torch.from_numpy(np.ascontiguousarray(O.waverec2(nest([t.numpy() for t in xs]), wavelet)))], lambda mine: tol),
         normwise_every(tol), minor=minor, nrandom=0)


KEYS3 = tuple(O.wavedec3(np.zeros((1, 8, 8, 8)), "db2", mode="zero", level=1)[1].keys())  # the seven detail keys, in the oracle's order


def padded3d(name, kid_fwd, kid_inv, wavelet, mode, n, opts=()):
    """``wavedec3`` / ``waverec3`` at level 1 on volumes of n^3 (float32): the analysis of a random batch, the synthesis of random bands
    that are the planes of one buffer [B, 8, M, M, M]."""
    flen = len(host_taps(wavelet)[0])
    m = (n + flen - 1) // 2
    n_out = 2 * m - flen + 2
    tol = PADDED_TOL[f32]

    def flat(c):
        return [c[0], *[c[1][k] for k in KEYS3]]

    def nest(ts):
        return [ts[0], dict(zip(KEYS3, ts[1:]))]

    cell(f"{name} wavedec3", {kid_fwd}, f32, (n ** 3, 8 * m ** 3), lambda b, gen: [_fill((b, n, n, n), f32, gen)],
         lambda xs: flat(ptwt_amd.wavedec3(xs[0], wavelet, mode=mode, level=1)),
         normwise_sample(lambda xs: [torch.from_numpy(np.ascontiguousarray(t)) for t in flat(O.wavedec3(xs[0].numpy(), wavelet, mode=mode, level=1))],
                         lambda mine: tol), normwise_every(tol), opts)
    cell(f"{name} waverec3", {kid_inv}, f32, (8 * m ** 3, n_out ** 3), lambda b, gen: list(_fill((b, 8, m, m, m), f32, gen).unbind(1)),
         lambda xs: [ptwt_amd.waverec3(nest(list(xs)), wavelet)],
         normwise_sample(lambda xs: [torch.from_numpy(np.ascontiguousarray(O.waverec3(nest([t.numpy() for t in xs]), wavelet)))], lambda mine: tol),
         normwise_every(tol), opts)


def stationary2d(n, flen=8, dilation=2, scale=0.25):
    """One stationary 2-D level through ``stationary_transform._level2_fwd`` / ``_level2_inv`` (ids 34 / 35, counted by the library's
    launch counters: these entries are outside the level launch path), four independent random filters; sized by the level buffer
    [B, 4, n, n], four times the plane batch (minor)."""
    taps = tuple(TS2._quantised(t, f32) for t in TS2.random_bank(flen, 7 * flen + 2 * n))
    tol = TS2.VALUE_TOL[f32]
    cell("34/35 swt2 fwd", set(), f32, (4 * n * n,), lambda b, gen: [_fill((b, n, n), f32, gen)],
         lambda xs: list(st._level2_fwd(xs[0], taps, dilation, scale).unbind(1)),
         normwise_sample(lambda xs: [torch.from_numpy(np.ascontiguousarray(t)) for t in R2.level_fwd(xs[0].numpy(), taps, dilation, scale)],
                         lambda mine: tol), normwise_every(tol), minor=(n * n,), counted=((st.KID_SWT2, 1), (st.KID_ISWT2, 0)))
    cell("34/35 swt2 inv", set(), f32, (4 * n * n,), lambda b, gen: list(_fill((b, 4, n, n), f32, gen).unbind(1)),
         lambda xs: [st._level2_inv(list(xs), taps, dilation, scale)],
         normwise_sample(lambda xs: [torch.from_numpy(np.ascontiguousarray(R2.level_inv([t.numpy() for t in xs], taps, dilation, scale)))],
                         lambda mine: tol), normwise_every(tol), minor=(n * n,), counted=((st.KID_SWT2, 0), (st.KID_ISWT2, 1)))


def stationary1d(n, flen=8, dilation=4, scale=0.25):
    """One stationary 1-D level (``_level_fwd`` / ``_level_inv``), sized by the level buffer [B, 2, n].  The kernel of
    csrc/mifwt_swt.hip has no id of its own and no counter, and the entry has one route; what can be asserted is that nothing ELSE ran:
    no event of the level launch path and no counted kernel."""
    bank = TSK.random_bank(flen, flen + n)
    lo, hi, rlo, rhi = (TSK._quantised(t, f32) for t in bank)
    tol = TSK.VALUE_TOL[f32]
    nothing_else = tuple((k, 0) for k in range(64))
    cell("swt fwd", set(), f32, (2 * n,), lambda b, gen: [_fill((b, n), f32, gen)],
         lambda xs: list(st._level_fwd(xs[0], lo, hi, dilation, scale).unbind(1)),
         normwise_sample(lambda xs: list(OE.swt_level_fwd(xs[0], lo, hi, dilation, scale).unbind(1)), lambda mine: tol),
         normwise_every(tol), minor=(n,), counted=nothing_else)
    cell("swt inv", set(), f32, (2 * n,), lambda b, gen: list(_fill((b, 2, n), f32, gen).unbind(1)),
         lambda xs: [st._level_inv(xs[0], xs[1], rlo, rhi, dilation, scale)],
         normwise_sample(lambda xs: [OE.swt_level_inv(xs[0], xs[1], rlo, rhi, dilation, scale)], lambda mine: tol),
         normwise_every(tol), minor=(n,), counted=nothing_else)


def padded1d(name, kid_fwd, kid_inv, wavelet, mode, n):
    """``wavedec`` / ``waverec`` at level 2 on rows of n samples (float32): [B, 1, M1] details, [B, 2, M2] approximation + details."""
    flen = len(host_taps(wavelet)[0])
    m1 = (n + flen - 1) // 2
    m2 = (m1 + flen - 1) // 2
    tol = PADDED_TOL[f32]

    def ref_fwd(xs):
        return [torch.from_numpy(np.ascontiguousarray(t)) for t in O.wavedec(xs[0].numpy(), wavelet, mode=mode, level=2)]

    def ref_inv(xs):
        return [torch.from_numpy(np.ascontiguousarray(O.waverec([t.numpy() for t in xs], wavelet)))]

    def make_inv(b, gen):
        coarse = _fill((b, 2, m2), f32, gen)
        return [coarse[:, 0], coarse[:, 1], _fill((b, m1), f32, gen)]

    n_out = 2 * m1 - flen + 2
    cell(f"{name} wavedec", {kid_fwd}, f32, (n, m1, 2 * m2), lambda b, gen: [_fill((b, n), f32, gen)],
         lambda xs: list(ptwt_amd.wavedec(xs[0], wavelet, mode=mode, level=2)), normwise_sample(ref_fwd, lambda mine: tol), normwise_every(tol))
    cell(f"{name} waverec", {kid_inv}, f32, (2 * m2, m1, n_out), make_inv,
         lambda xs: [ptwt_amd.waverec(list(xs), wavelet)], normwise_sample(ref_inv, lambda mine: tol), normwise_every(tol))


def _per_bank(dtype, flen=8):
    return TPER.random_bank(flen, 31, f32 if dtype == f32 else f64)


def _forced(module, attr, value):
    """A scope factory: ``module.attr = value`` for the duration of a cell (the routing switches the families' own modules use)."""
    @contextlib.contextmanager
    def scope():
        keep = getattr(module, attr)
        setattr(module, attr, value)
        try:
            yield
        finally:
            setattr(module, attr, keep)
    return scope


def periodized(dtype, h, w, axis=False):
    """One periodized level through ``_per.level_fwd`` / ``level_inv``, four independent random filters of eight taps: the fused kernels
    38 / 39, or with ``_per.FORCE_AXIS`` the axis passes 40 / 41 (three launches a level)."""
    bank = _per_bank(dtype)
    mh, mw = (h + 1) // 2, (w + 1) // 2
    name = f"40/41 periodization axis passes {TPER._name(dtype)}" if axis else f"38/39 periodization {TPER._name(dtype)}"
    kid_fwd, kid_inv = (40, 41) if axis else (38, 39)
    scope = _forced(_per, "FORCE_AXIS", True) if axis else contextlib.nullcontext

    def tol_of(fn):
        return lambda mine: TPER._value_tol(dtype, RP.e_ref32(fn, *mine, scale=float(mine[0].norm())) if dtype == f32 else 0.0)

    fwd = lambda t: RP.level_fwd(t, bank, 2)  # noqa: E731
    inv = lambda *b: RP.level_inv(list(b), bank, 2, [h, w])  # noqa: E731
    floor = TPER._value_tol(dtype, 0.0)
    cell(f"{name} fwd", {kid_fwd}, dtype, (h * w, 4 * mh * mw), lambda b, gen: [_fill((b, h, w), dtype, gen)],
         lambda xs: list(_per.level_fwd(xs[0], bank[0], bank[1]).unbind(1)),
         normwise_sample(lambda xs: fwd(xs[0]), tol_of(fwd), RP.relerr), normwise_every(floor), scope=scope)
    cell(f"{name} inv", {kid_inv}, dtype, (4 * mh * mw, h * w), lambda b, gen: list(_fill((b, 4, mh, mw), dtype, gen).unbind(1)),
         lambda xs: [_per.level_inv(list(xs), bank[2], bank[3], [h, w])],
         normwise_sample(lambda xs: [inv(*xs)], tol_of(inv), RP.relerr), normwise_every(floor), scope=scope)


def value_map(mode, h, w, wavelet="db4", axis=False):
    """One level of a value-map extension mode through ``_ext.level_fwd`` and its adjoint ``_ext.level_adj``, float32: the fused kernels
    42 / 43, or with ``_ext.FORCE_AXIS`` the axis passes 44 / 45."""
    bank = host_taps(wavelet)
    flen = len(bank[0])
    mh, mw = (h + flen - 1) // 2, (w + flen - 1) // 2
    fwd = lambda t: RE.level_fwd(t, bank, mode, 2)  # noqa: E731
    adj = lambda *g: RE.level_adj(list(g), bank, mode, 2, [h, w])  # noqa: E731
    name = f"44/45 {mode} axis passes" if axis else f"42/43 {mode}"
    kid_fwd, kid_adj = (44, 45) if axis else (42, 43)
    scope = _forced(_ext, "FORCE_AXIS", True) if axis else contextlib.nullcontext

    def tol_of(fn):
        return lambda mine: TE._tol(f32, RE.e_ref32(fn, *mine, scale=float(torch.cat([m.reshape(-1) for m in mine]).norm())))

    floor = TE._tol(f32, 0.0)
    cell(f"{name} fwd", {kid_fwd}, f32, (h * w, 4 * mh * mw), lambda b, gen: [_fill((b, h, w), f32, gen)],
         lambda xs: list(_ext.level_fwd(xs[0], bank[0], bank[1], mode).unbind(1)),
         normwise_sample(lambda xs: fwd(xs[0]), tol_of(fwd), RE.relerr), normwise_every(floor), scope=scope)
    cell(f"{name} adj", {kid_adj}, f32, (4 * mh * mw, h * w), lambda b, gen: [_fill((b, 4, mh, mw), f32, gen)],
         lambda xs: [_ext.level_adj(xs[0], bank[0], bank[1], mode, [h, w])],
         normwise_sample(lambda xs: [adj(*xs[0].unbind(1))], lambda mine: tol_of(adj)(list(mine[0].unbind(1))), RE.relerr), normwise_every(floor),
         scope=scope)


def boundary_level(name, kid_fwd, kid_inv, taps, sig, mode, tol, fused, scope=contextlib.nullcontext):
    """One boundary-wavelet level through ``_bwt.rows_level`` / ``_bwt.transposed_level`` on items of extents ``sig`` (odd ones get the
    mode's virtual sample), float32, four independent random filters: the fused kernels (26 / 27 planes, 30 / 31 volumes; the float64
    operator then holds the entries rounded to float32, as these kernels do — ``round32``) or the axis passes 28 / 29."""
    nd = len(sig)
    coef = [(n + 1) // 2 for n in sig]
    n_sig, n_coef = int(np.prod(sig)), int(np.prod(coef))
    kw = {"round32": fused}

    def bk(which):
        return _bwt.bank(taps, "gramschmidt", which)

    cell(f"{name} fwd", {kid_fwd}, f32, (n_sig, (1 << nd) * n_coef), lambda b, gen: [_fill((b, *sig), f32, gen)],
         lambda xs: list(_bwt.rows_level(xs[0], bk("analysis"), _engine.MODE_IDS[mode]).unbind(1)),
         normwise_sample(lambda xs: list(BR.rows_level(xs[0], taps, "analysis", mode, **kw).unbind(1)), lambda mine: tol),
         normwise_every(tol), scope=scope)
    cell(f"{name} inv", {kid_inv}, f32, ((1 << nd) * n_coef, n_sig), lambda b, gen: list(_fill((b, 1 << nd, *coef), f32, gen).unbind(1)),
         lambda xs: [_bwt.transposed_level(list(xs), bk("synthesis"), sig)],
         normwise_sample(lambda xs: [BR.transposed_level(list(xs), taps, "synthesis", sig, **kw)], lambda mine: tol),
         normwise_every(tol), scope=scope)


def boundary_tree(n, k, wavelet="db4"):
    """``k`` levels of a boundary-wavelet packet tree below every row in ONE launch (``_bwt.rows_tree`` / ``transposed_tree``, ids
    32 / 33): rows of n samples, k level buffers [B, n] each; the float64 host chain of tests/_boundary_tree_ref.py."""
    taps = host_taps(wavelet)
    cell("32/33 packet subtree fwd", {32}, f32, (n,), lambda b, gen: [_fill((b, n), f32, gen)],
         lambda xs: _bwt.rows_tree(xs[0], _bwt.bank(taps, "qr", "analysis"), k),
         normwise_sample(lambda xs: BT.tree_fwd(xs[0], taps, k), lambda mine: TBP.tol(f32, "fwd")), normwise_every(TBP.tol(f32, "fwd")))
    cell("32/33 packet subtree inv", {33}, f32, (n,), lambda b, gen: [_fill((b, 1 << k, n >> k), f32, gen)],
         lambda xs: _bwt.transposed_tree(xs[0], _bwt.bank(taps, "qr", "synthesis"), k),
         normwise_sample(lambda xs: BT.tree_inv(xs[0], taps, k), lambda mine: TBP.tol(f32, "inv")), normwise_every(TBP.tol(f32, "inv")))


def stationary3d(n, flen=8, dilation=2, scale=0.25):
    """One stationary 3-D level through ``stationary_transform._level3_fwd`` / ``_level3_inv`` (ids 36 / 37, counted by the library's
    launch counters), six independent random filters; sized by the level buffer [B, 8, n, n, n], eight times the volume batch (minor)."""
    taps = tuple(TS3._quantised(t, f32) for t in TS3.random_bank(flen, 7 * flen + 3 * n))
    tol = TS3.VALUE_TOL[f32]
    cell("36/37 swt3 fwd", set(), f32, (8 * n ** 3,), lambda b, gen: [_fill((b, n, n, n), f32, gen)],
         lambda xs: list(st._level3_fwd(xs[0], taps, dilation, scale, composed=False).unbind(1)),
         normwise_sample(lambda xs: [torch.from_numpy(np.ascontiguousarray(t)) for t in R3.level_fwd(xs[0].numpy(), taps, dilation, scale)],
                         lambda mine: tol), normwise_every(tol), minor=(n ** 3,), counted=((st.KID_SWT3, 1), (st.KID_ISWT3, 0)))
    cell("36/37 swt3 inv", set(), f32, (8 * n ** 3,), lambda b, gen: list(_fill((b, 8, n, n, n), f32, gen).unbind(1)),
         lambda xs: [st._level3_inv(list(xs), taps, dilation, scale, composed=False)],
         normwise_sample(lambda xs: [torch.from_numpy(np.ascontiguousarray(R3.level_inv([t.numpy() for t in xs], taps, dilation, scale)))],
                         lambda mine: tol), normwise_every(tol), minor=(n ** 3,), counted=((st.KID_SWT3, 0), (st.KID_ISWT3, 1)))


@contextlib.contextmanager
def _fused_complex():
    """Every complex cell of the fused envelope on the fused kernels 46 / 47, whatever the measured routing says."""
    keep = _cplx.COMPOSED_CELLS
    _cplx.COMPOSED_CELLS = set()
    _cplx._plans.clear()
    try:
        yield
    finally:
        _cplx.COMPOSED_CELLS = keep
        _cplx._plans.clear()


def complex2d(h, w, mode="symmetric", wavelet="db4"):
    """One complex64 level through ``_cplx.level_fwd`` / ``level_inv`` (ids 46 / 47)."""
    bank = host_taps(wavelet)
    flen = len(bank[0])
    mh, mw = (h + flen - 1) // 2, (w + flen - 1) // 2
    ho, wo = 2 * mh - flen + 2, 2 * mw - flen + 2
    fwd = lambda t: RC.level_fwd(t, bank, mode, 2)  # noqa: E731
    inv = lambda *b: RC.level_inv(list(b), bank, 2, None, [ho, wo])  # noqa: E731

    def tol_of(fn):
        return lambda mine: TC._tol(c64, RC.e_ref32(fn, *mine, scale=float(torch.cat([m.reshape(-1) for m in mine]).norm())))

    floor = TC._tol(c64, 0.0)
    cell("46/47 complex64 fwd", {46}, c64, (h * w, 4 * mh * mw), lambda b, gen: [_fill((b, h, w), c64, gen)],
         lambda xs: list(_cplx.level_fwd(xs[0], bank[0], bank[1], _engine.MODE_IDS[mode]).unbind(1)),
         normwise_sample(lambda xs: fwd(xs[0]), tol_of(fwd), RC.relerr), normwise_every(floor), scope=_fused_complex)
    cell("46/47 complex64 inv", {47}, c64, (4 * mh * mw, ho * wo), lambda b, gen: list(_fill((b, 4, mh, mw), c64, gen).unbind(1)),
         lambda xs: [_cplx.level_inv(list(xs), bank[2], bank[3], [ho, wo])],
         normwise_sample(lambda xs: [inv(*xs)], tol_of(inv), RC.relerr), normwise_every(floor), scope=_fused_complex)


# ---- thresholding (48): the element-wise bound and the exact decisions of tests/test_gpu_thresh.py -------------------------------------
def _thresh_every(cell, k, whole, part, inputs, start):
    """Check 3: an element's result depends on that element and its threshold alone, so the whole batch and its slice agree bit for bit."""
    same = torch.equal(whole, part)
    _record(cell.name + " slices", 0.0 if same else float("inf"))
    if not same:
        bad = (whole != part).reshape(whole.shape[0], -1).any(1).nonzero()
        raise AssertionError(f"{cell.name}: tensor {k}, item {start + int(bad[0])} whole batch against its slice")


def thresholds():
    n, m = 128, 67
    # a dense tensor, one number: collapsed into ONE row of 2^31 + 3 x 2^14 elements, cut back into four (thresholding._split_row)
    cell("48 threshold dense", {48}, f32, (n * n,), lambda b, gen: [_fill((b, n, n), f32, gen, 2.0)],
         lambda xs: [ptwt_amd.threshold(xs[0], 0.5, "soft")],
         lambda c, items, xs, gots: TH.check(gots[0], xs[0], RT.threshold(_up(xs[0]), 0.5, "soft"), 0.5, 0.0, c.name),
         _thresh_every)

    # a container of strided bands (the planes of one level buffer) with one threshold PER IMAGE for the approximation and another for
    # the details; the outputs mirror the buffer.  (Thresholds are multiples of 1/8: the decisions must agree exactly.)
    def make(b, gen):
        buf = _fill((b, 4, m, m), f32, gen, 2.0)
        va = torch.randint(1, 9, (b,), device=DEV, generator=gen).to(f32) / 8
        vd = torch.randint(4, 17, (b,), device=DEV, generator=gen).to(f32) / 8
        return [*buf.unbind(1), va, vd]

    def call(xs):
        out = ptwt_amd.threshold([xs[0], tuple(xs[1:4])], [xs[4], xs[5]], "garrote")
        return [out[0], *out[1]]

    def sample(c, items, xs, gots):
        want = RT.threshold([_up(xs[0]), tuple(_up(t) for t in xs[1:4])], [_up(xs[4]), _up(xs[5])], "garrote")
        for k, (g, w) in enumerate(zip(gots, [want[0], *want[1]])):
            TH.check(g, xs[k], w, _up(xs[4 if k == 0 else 5]).reshape(-1, 1, 1), 0.0, f"{c.name} band {k}")

    cell("48 threshold bands per image", {48}, f32, (4 * m * m,), make, call, sample, _thresh_every)


padded2d("7/8 tiles f32", 7, 8, f32, "db4", "symmetric", (128, 128), NO_SMALL)
padded2d("7/8 tiles f64", 7, 8, f64, "db2", "reflect", (128, 128), NO_SMALL)
padded2d("7/8 tiles f16", 7, 8, f16, "db4", "zero", (128, 128), NO_SMALL, ptwt_amd.half_storage)
padded2d("20/21 small planes", 20, 21, f32, "db4", "reflect", (128, 128))
streaming2d()
padded2d("1/2 wave strips", 1, 2, f32, "db4", "symmetric", (256, 1030), NO_TILES)
padded2d_pair("12/13 pair", "db4", "reflect", 128, NO_SMALL)
padded2d("0 generic passes", 0, 0, f32, "db4", "symmetric", (128, 128), FORCE_GENERIC)
padded2d("3/4 axis passes f64 18 taps", 3, 4, f64, "db9", "symmetric", (128, 128))
padded1d_level("3/4 rows", 3, 4, "db4", "symmetric", 999)
padded1d("14/15 one workgroup per row", 14, 15, "db4", "symmetric", 1000)
padded1d("17/18 chunked rows", 17, 18, "db4", "reflect", 4096)
padded3d("9/10 bricks", 9, 10, "db2", "symmetric", 32)
padded3d("24/25 walk", 24, 25, "db2", "reflect", 32, WALK4)
padded3d("5/6 composed", 5, 6, "db5", "symmetric", 32)
periodized(f32, 126, 124)
periodized(f64, 126, 124)
periodized(f32, 126, 124, axis=True)
value_map("smooth", 126, 124)
value_map("smooth", 126, 124, axis=True)
complex2d(126, 124)
boundary_level("26/27 boundary planes", 26, 27, TBK.random_bank(8), (125, 123), "symmetric", TBK.LEVEL_TOL[f32], True)
boundary_level("28/29 boundary axis passes", 28, 29, TBK.random_bank(22), (125, 123), "reflect", TBK.LEVEL_TOL[f32], False)
boundary_level("30/31 boundary volumes", 30, 31, TB3.random_bank(8), (31, 32, 29), "periodic", TB3.LEVEL_TOL32[8], True,
               _forced(_bwt, "COMPOSED3_CELLS", set()))
boundary_tree(4096, 2)
stationary2d(128)
stationary3d(32)
stationary1d(4096)
thresholds()


@pytest.mark.parametrize("c", CELLS, ids=lambda c: c.name.replace(" ", "-"))
def test_cell(c):
    run_cell(c)


def test_threshold_backward_with_a_learnable_threshold():
    """``threshold(x, v, "soft")`` of a dense tensor of 2^31 + 3 x 2^14 float32 elements with a learnable one-element threshold: kernel 49
    plus the reduction launch.  d/dx of the sampled items against float64 autograd of the reference on the sampled cotangent slices
    (element-wise, the rule of tests/test_gpu_thresh.py); d/dv against the float64 sum over batch slices of ``-sign(x) g [|x| > v]``,
    within ``(15 + 0 + 1) eps32 sum |g| [|x| > v]`` (same module: TERMS_PER_PARTIAL, TERM_ROUNDINGS["soft"], one rounding to float32)."""
    n, v0 = 128, 1.25
    batch = L.batch_over(MARK[f32], (n * n,))
    need = 4 * batch * n * n * 4 + (10 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{need / 2 ** 30:.1f} GiB needed, {free / 2 ** 30:.1f} GiB free")
    torch.cuda.reset_peak_memory_stats()
    gen = torch.Generator(device=DEV).manual_seed(77)
    try:
        x = _fill((batch, n, n), f32, gen, 2.0)
        # (no element within 2e-3 of the threshold: no tie can flip between the float32 kernel and the float64 reference — TH.pushed)
        for s, e in L.batch_slices(batch, n * n):
            xs = x[s:e]
            near = (xs.abs() - v0).abs() < 2e-3
            xs.copy_(torch.where(near, torch.where(xs < 0, -(v0 + 4e-3), v0 + 4e-3).to(f32), xs))
            del near
        g = _fill((batch, n, n), f32, gen)
        x.requires_grad_(True)
        v = torch.tensor([v0], dtype=f32, device=DEV, requires_grad=True)
        _engine.level_events = []
        try:
            y = ptwt_amd.threshold(x, v, "soft")
            gx, gv = torch.autograd.grad(y, (x, v), g)
            tags = [(e[0], e[1]) for e in _engine.level_events]
        finally:
            _engine.level_events = None
        assert tags == [("thresh_fwd", 48), ("thresh_bwd", 49)], tags
        del y
        assert gx.dtype == f32 and gv.dtype == f32 and gv.shape == v.shape
        items = L.sample_items(batch, [(n * n, 4)], 77)
        idx = torch.tensor(items, device=DEV)
        xi = x.detach().index_select(0, idx).double().requires_grad_(True)
        gi = g.index_select(0, idx).double()
        vi = torch.tensor([v0], dtype=f64, device=DEV, requires_grad=True)
        want_gx, = torch.autograd.grad(RT.threshold(xi, vi, "soft"), (xi,), gi)
        bound = 8 * 2 * TH.EPS[f32] * torch.clamp(xi.detach().abs(), min=v0) * gi.abs()
        err = (gx.index_select(0, idx).double() - want_gx).abs()
        assert bool((err <= bound).all()), "d/dx of the sampled items"
        want_v = torch.zeros((), dtype=f64, device=DEV)
        terms = torch.zeros((), dtype=f64, device=DEV)
        for s, e in L.batch_slices(batch, n * n):
            xs, gs = x.detach()[s:e], g[s:e]
            keep = xs.abs() > v0
            # every item: d/dx is g where the element is kept and 0 elsewhere, exactly
            assert torch.equal(gx[s:e], torch.where(keep, gs, torch.zeros_like(gs))), f"d/dx, items {s} .. {e}"
            want_v -= (torch.sign(xs) * gs * keep).sum(dtype=f64)
            terms += (gs.abs() * keep).sum(dtype=f64)
            del keep
        bound_v = (TH.TERMS_PER_PARTIAL - 1 + TH.TERM_ROUNDINGS["soft"] + 1) * TH.EPS[f32] * float(terms)
        err_v = abs(float(gv.double()) - float(want_v))
        _record("49 threshold gradient", err_v / bound_v)
        print(f"threshold gradient: kernel {float(gv):.6e} float64 sum over slices {float(want_v):.6e} error {err_v:.3e} bound {bound_v:.3e}, "
              f"peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
        assert err_v <= bound_v
    finally:
        x = g = gx = gv = None
        torch.cuda.empty_cache()


def test_threshold_of_a_row_with_no_cut_is_composed():
    """A single axis of 2^31 - 1 elements (a prime: no equal rows of at most 2^30 elements exist) is outside the kernels' envelope and
    takes the composed route: no launch of kernel 48, and the values of windows at both ends and around elements 2^30 and
    2^31 - 2^20 within the element-wise bound of tests/test_gpu_thresh.py."""
    n = (1 << 31) - 1
    need = 6 * n * 4 + (2 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{need / 2 ** 30:.1f} GiB needed, {free / 2 ** 30:.1f} GiB free")
    x = y = None
    try:
        x = _fill((n,), f32, torch.Generator(device=DEV).manual_seed(5), 2.0)
        before = _engine.launch_count(48)
        y = ptwt_amd.threshold(x, 0.5, "soft")
        assert _engine.launch_count(48) == before and y.shape == x.shape and y.dtype == f32
        for start in (0, (1 << 30) - 2048, n - (1 << 20), n - 4096):
            xs, ys = x[start:start + 4096].cpu(), y[start:start + 4096].cpu()
            TH.check(ys, xs, RT.threshold(_up(xs), 0.5, "soft"), 0.5, 0.0, f"composed, elements from {start}")
    finally:
        x = y = None
        torch.cuda.empty_cache()


def _backward_cell(name, strides, make, call, ref_call, grads_of, kids, masks, opts=()):
    """A backward leg on a batch past the marks: ``call(leaves)`` -> outputs, cotangents ``grads_of`` them drawn on the device, the
    gradients of the leaves (1) item by item against float64 autograd of the reference ``ref_call`` on the sampled leaf and cotangent
    slices — the measures and the bounds of tests/test_gpu_data_gradients.py (norm-wise, max-abs and, for a signal, the border strip) —
    and (2) every item against the same backward on consecutive batch slices."""
    batch = L.batch_over(MARK[f32], strides)
    need = 2 * sum(strides) * batch * 4 * 1.3 + (6 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{name}: {need / 2 ** 30:.1f} GiB needed, {free / 2 ** 30:.1f} GiB free")
    torch.cuda.reset_peak_memory_stats()
    bounds = TG.F32_BOUNDS
    gen = torch.Generator(device=DEV).manual_seed(4242)
    for key, value in opts:
        _engine.set_option(key, value)
    try:
        leaves = make(batch, gen)
        cots = grads_of(batch, gen)

        def backward(lv, ct):
            lv = [t.detach().requires_grad_(True) for t in lv]
            _engine.level_events = []
            try:
                outs = call(lv)
                got = torch.autograd.grad(outs, lv, ct)
                ran = {e[1] for e in _engine.level_events}
            finally:
                _engine.level_events = None
            assert ran == kids, (name, "kernel ids", sorted(ran), "expected", sorted(kids))
            return got

        got = backward(leaves, cots)
        buffers = sorted({(t.stride(0), t.element_size()) for t in list(leaves) + list(cots) + list(got)})
        assert all(st_ in strides and st_ * batch > MARK[f32] for st_, _ in buffers), (name, buffers)
        items = L.sample_items(batch, buffers, 4242)
        idx = torch.tensor(items, device=DEV)
        lv64 = [t.index_select(0, idx).cpu().double().requires_grad_(True) for t in leaves]
        want = torch.autograd.grad(ref_call(lv64), lv64, [t.index_select(0, idx).cpu().double() for t in cots])
        for k, (g, w, mask) in enumerate(zip(got, want, masks)):
            gi = g.index_select(0, idx).cpu().double().numpy()
            for j, item in enumerate(items):
                m = TG.D.measures(gi[j], w[j].numpy(), mask)
                for key, v in m.items():
                    _record(name, v / bounds[key])
                    assert v < bounds[key], f"{name}: gradient {k}, item {item}, {key}: {v:.3e} >= {bounds[key]:.3e}"
        for start, stop in L.batch_slices(batch, max(strides)):
            part = backward([t[start:stop] for t in leaves], [t[start:stop] for t in cots])
            for k, (g, p) in enumerate(zip(got, part)):
                err = L.item_relerr(g[start:stop], p)
                _record(name + " slices", float(err.max()) / bounds["norm"])
                assert float(err.max()) < bounds["norm"], f"{name}: gradient {k}, item {start + int(err.argmax())} whole batch against its slice"
            del part
        print(f"{name}: batch {batch}, peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB, worst / bound {WORST[name]:.3f} (samples) "
              f"{WORST[name + ' slices']:.3f} (slices)")
    finally:
        for key, _ in opts:
            _engine.set_option(key, 0)
        leaves = cots = got = None
        torch.cuda.empty_cache()


def test_backward_of_wavedec2_symmetric():
    """d/dx of ``wavedec2(x, "db4", mode="symmetric", level=1)`` on 131075 planes of 128 x 128: the synthesis tiles with the reversed
    analysis taps (8) plus the adjoint-border kernel, launched in chunks of 32768 images (``img0 + blockIdx.y``, int64 in
    csrc/mifwt_adjoint_border.hip); the forward on the tiles (7)."""
    n, m = 128, 67
    _backward_cell("backward wavedec2", (n * n, 4 * m * m), lambda b, gen: [_fill((b, n, n), f32, gen)],
                   lambda lv: _flat2(ptwt_amd.wavedec2(lv[0], "db4", mode="symmetric", level=1)),
                   lambda lv: _flat2(A.wavedec2(lv[0], "db4", mode="symmetric", level=1)),
                   lambda b, gen: list(_fill((b, 4, m, m), f32, gen).unbind(1)), {7, 8}, [TG.D.border_mask((n, n), (0, 1), 8)], NO_SMALL)


def test_backward_of_waverec2():
    """d/dcoefficients of ``waverec2`` of random bands (the planes of one leaf [B, 4, 67, 67]): the analysis tiles with the reversed
    synthesis taps (7) write the gradient buffer [B, 4, 67, 67]; the forward on the synthesis tiles (8)."""
    n, m = 128, 67

    def rec(fn):
        return lambda lv: [fn([lv[0][:, 0], (lv[0][:, 1], lv[0][:, 2], lv[0][:, 3])], "db4")]

    _backward_cell("backward waverec2", (4 * m * m, n * n), lambda b, gen: [_fill((b, 4, m, m), f32, gen)], rec(ptwt_amd.waverec2), rec(A.waverec2),
                   lambda b, gen: [_fill((b, n, n), f32, gen)], {7, 8}, [None], NO_SMALL)


TAPCORR = (_engine.VARIANT_TAPCORR_ROWS, _engine.VARIANT_TAPCORR_COLS, _engine.VARIANT_TAPCORR_TERM)


@contextlib.contextmanager
def _tap_correlations(batch, what):
    """The route of the tap-gradient correlations of csrc/mifwt_tapgrad.hip, which have no kernel id and no event: the calls of
    ``ENGINE.tap_correlate`` / ``tap_correlate_planes`` are recorded, and on leaving the scope (1) every call saw the WHOLE batch and
    (2) the library's launch counters of the three kernels moved by what the launchers' guards say for those calls: the wave kernel along
    rows while ``rows x ceil(M / 64) < 2^31`` (else the one-thread-per-term kernel, once per 32 taps), the wave kernel along columns
    for the planes entry with ``along = 0``."""
    eng, calls = _engine.ENGINE, []
    keep = {name: getattr(eng, name) for name in ("tap_correlate", "tap_correlate_planes")}

    def spy(name):
        def run(*args, **kw):
            along, a = (1, args[0]) if name == "tap_correlate" else (args[0], args[1])
            calls.append((name, along, tuple(a.shape), args[2] if name == "tap_correlate" else args[3]))
            return keep[name](*args, **kw)
        return run

    before = [_engine.launch_count(k) for k in TAPCORR]
    for name in keep:
        setattr(eng, name, spy(name))
    try:
        yield calls
    finally:
        for name in keep:  # (the entries are methods of the engine's class: dropping the instance attributes puts them back)
            delattr(eng, name)
            assert getattr(eng, name) == keep[name]
    want = [0, 0, 0]
    for name, along, shape, flen in calls:
        rows = int(np.prod(shape[:-1]))
        if along == 0:
            want[1] += 1
        elif rows * -(-shape[-1] // 64) < 1 << 31:
            want[0] += 1
        else:
            want[2] += -(-flen // 32)
    ran = [_engine.launch_count(k) - n for k, n in zip(TAPCORR, before)]
    assert calls and all(int(np.prod(shape[:-1])) >= batch for _, _, shape, _ in calls), (what, calls)
    assert ran == want, (what, "launches of the row / column / per-term correlation kernels", ran, "expected", want, calls)
    print(f"{what}: correlation launches (rows, columns, per term) {ran}")


def _sum_of_slice_gradients(taps64, slices, term):
    """The float64 sum over batch slices of d ``term(start, stop)`` / d taps (``term``: a float64 scalar on the device)."""
    total = [torch.zeros_like(t) for t in taps64]
    for start, stop in slices:
        for acc, g in zip(total, torch.autograd.grad(term(start, stop), taps64)):
            acc += g
    return total


@pytest.mark.parametrize("sig", [(4096,), (128, 128)], ids=["1d", "2d"])
def test_tap_gradients_of_a_learnable_db2_bank(sig):
    """The four tap gradients of a learnable db2 bank, level 1 in "symmetric", on a batch of more than 2^31 float32 elements: the
    correlations of csrc/mifwt_tapgrad.hip reduce over the WHOLE batch in one call each (asserted: every call saw all the rows), the
    place where a 32-bit count or offset would wrap.  d/d(dec_lo, dec_hi) of ``<cotangents, wavedec(x)>`` and d/d(rec_lo, rec_hi) of
    ``<cotangent, waverec(random coefficients)>`` against the float64 SUM over batch slices of 2^26 elements of the same gradients of
    the level written as plain tensor arithmetic (``_large_ref.analysis_level`` / ``synthesis_level_adjoint``, pinned to
    oracle/torch_autograd_ref.py on the CPU), under the rule of tests/test_gpu_learnable_lengths.py: norm-wise below ``F32_TOL`` and
    max-abs below ten times that of the largest entry (``_check`` there)."""
    nd, flen, mode = len(sig), 4, "symmetric"
    coef = tuple((n + flen - 1) // 2 for n in sig)
    out = tuple(2 * m - flen + 2 for m in coef)
    n_sig, n_coef, n_out = int(np.prod(sig)), (1 << nd) * int(np.prod(coef)), int(np.prod(out))
    batch = L.batch_over(MARK[f32], (n_sig, n_coef, n_out))
    need = 6 * max(n_sig, n_coef) * batch * 4 + (8 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{need / 2 ** 30:.1f} GiB needed, {free / 2 ** 30:.1f} GiB free")
    torch.cuda.reset_peak_memory_stats()
    dec, rec = (ptwt_amd.wavedec, ptwt_amd.waverec) if nd == 1 else (ptwt_amd.wavedec2, ptwt_amd.waverec2)
    nest = (lambda ts: list(ts)) if nd == 1 else (lambda ts: [ts[0], tuple(ts[1:])])
    flat = (lambda c: list(c)) if nd == 1 else _flat2
    gen = torch.Generator(device=DEV).manual_seed(31 + nd)
    values = [torch.tensor(t, dtype=f32) for t in host_taps("db2")]  # (float32 taps: both sides see the same rounded values)
    taps = [t.to(DEV).requires_grad_(True) for t in values]
    taps64 = [t.double().to(DEV).requires_grad_(True) for t in values]
    slices = L.batch_slices(batch, max(n_sig, n_coef), 1 << 26)
    name = f"tap gradients {nd}-D"
    x = g = y = None
    try:
        # analysis: d/d(dec_lo, dec_hi)
        x = _fill((batch, *sig), f32, gen)
        g = _fill((batch, 1 << nd, *coef), f32, gen)
        with _tap_correlations(batch, name + " analysis"):
            got = torch.autograd.grad(flat(dec(x, tuple(taps), mode=mode, level=1)), taps[:2], list(g.unbind(1)))
        want = _sum_of_slice_gradients(taps64[:2], slices, lambda s, e: sum(
            (c.double() * t).sum() for c, t in zip(g[s:e].unbind(1), L.analysis_level(x[s:e].double(), taps64[0], taps64[1], mode))))
        errs = [TLL._check(a, b.cpu(), TLL.F32_TOL, (name, which)) for a, b, which in zip(got, want, TLL.TAPS[:2])]
        x = g = None
        # synthesis: d/d(rec_lo, rec_hi), random coefficients
        x = _fill((batch, 1 << nd, *coef), f32, gen)
        g = _fill((batch, *out), f32, gen)
        with _tap_correlations(batch, name + " synthesis"):
            y = rec(nest(list(x.unbind(1))), tuple(taps))
            assert tuple(y.shape) == (batch, *out)
            got = torch.autograd.grad(y, taps[2:], g)
        y = None
        want = _sum_of_slice_gradients(taps64[2:], slices, lambda s, e: sum(
            (c.double() * t).sum() for c, t in zip(x[s:e].unbind(1), L.synthesis_level_adjoint(g[s:e].double(), taps64[2], taps64[3]))))
        errs += [TLL._check(a, b.cpu(), TLL.F32_TOL, (name, which)) for a, b, which in zip(got, want, TLL.TAPS[2:])]
        _record(name, max(errs) / TLL.F32_TOL)
        print(f"{name}: batch {batch}, norm-wise errors {['%.2e' % e for e in errs]} (bound {TLL.F32_TOL:.0e}), "
              f"peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    finally:
        x = g = y = got = None
        torch.cuda.empty_cache()


# ---- regime HUGE: ONE item at the in-item guards, windows of 96 x 96 against float64 ---------------------------------------------------
Huge = namedtuple("Huge", "name fam analysis dtype make call kids counted tol relerr opts scope gib seed")
HUGE = []
INSIDE = (23170, 23170)   # span 23169 x 23170 + 23170 = 536 848 900 < 2^29 elements, 23171^2 is not: the last square inside
                          # dwt2_fwd_tile_supported (csrc/mifwt_compose.hip:110); rows of 2 mod 4 samples, so no row but the first is 16-byte aligned
PAST = (46341, 46349)     # 2 147 859 009 elements > 2^31: row x pitch leaves an int from row 46333 on
PAST_EVEN = (46342, 46350)  # (circular levels: even extents)
FALLBACK = {0, 3, 4}      # what a padded 2-D level runs on past the tiles' span: the streaming axis passes or the generic passes


def huge(name, fam, analysis, dtype, make, call, kids, tol, relerr=None, opts=(), scope=contextlib.nullcontext, counted=(), gib=24):
    HUGE.append(Huge(name, fam, analysis, dtype, make, call, kids, tuple(counted), tol, relerr, tuple(opts), scope, gib, 7000 + len(HUGE)))


def run_huge(h):
    """One call on ONE item; the route; every window of ``_large_ref.window_starts`` of every output against the family's float64
    single-level reference on the crop of the input the window depends on (``_large_ref.window_reference``), at the family's bound."""
    free = torch.cuda.mem_get_info()[0]
    if free < h.gib << 30:
        pytest.skip(f"{h.name}: {h.gib} GiB needed, {free / 2 ** 30:.1f} GiB free")
    torch.cuda.reset_peak_memory_stats()
    for key, value in h.opts:
        _engine.set_option(key, value)
    inputs = outs = None
    try:
        with h.scope():
            inputs = h.make(torch.Generator(device=DEV).manual_seed(h.seed))
            before = {k: _engine.launch_count(k) for k, _ in h.counted}
            _engine.level_events = []
            try:
                outs = h.call(inputs)
                kids = {e[1] for e in _engine.level_events}
            finally:
                _engine.level_events = None
            assert (kids and kids <= h.kids) if h.kids is FALLBACK else kids == h.kids, (h.name, "kernel ids", sorted(kids), "expected", sorted(h.kids))
            ran = {k: _engine.launch_count(k) - n for k, n in before.items()}
            assert ran == dict(h.counted), (h.name, "launches", ran, "expected", dict(h.counted))
        nd = h.fam.ndim
        in_ext, out_ext = tuple(inputs[0].shape[-nd:]), tuple(outs[0].shape[-nd:])
        assert all(tuple(t.shape[-nd:]) == in_ext for t in inputs) and all(tuple(t.shape[-nd:]) == out_ext for t in outs)
        per_row = float(h.fam.factor) if h.analysis else 1.0 / h.fam.factor
        pitches = {(t.stride(-2), 1.0) for t in outs} | {(t.stride(-2), per_row) for t in inputs}
        starts = L.window_starts(out_ext, sorted(pitches))
        crops = []

        def gather(idx):
            crops[:] = [_up(L.take(t, idx).cpu()) for t in inputs]
            return crops

        for start in starts:
            want = L.window_reference(h.fam, h.analysis, gather, in_ext, out_ext, start)
            bound = h.tol(crops)
            scale = float(torch.cat([torch.view_as_real(c).reshape(-1) if c.is_complex() else c.reshape(-1) for c in crops]).norm())
            assert len(want) == len(outs)
            for k, (o, w) in enumerate(zip(outs, want)):
                got = _up(o[(Ellipsis, *[slice(s, s + w.shape[-nd + a]) for a, s in enumerate(start)])].cpu())
                assert got.shape == w.shape, (h.name, start, k, got.shape, w.shape)
                err = h.relerr(got, w, scale) if h.relerr else TP.G.relerr(got.numpy(), w.numpy())
                _record(h.name, err / bound)
                assert err < bound, f"{h.name}: window at {start}, output {k}: {err:.3e} >= {bound:.3e}"
        print(f"{h.name}: {'x'.join(map(str, in_ext))} -> {'x'.join(map(str, out_ext))}, {len(starts)} windows, peak "
              f"{torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB, worst / bound {WORST.get(h.name, 0.0):.3f}")
    finally:
        for key, _ in h.opts:
            _engine.set_option(key, 0)
        inputs = outs = None
        torch.cuda.empty_cache()


def _huge_families():
    db4 = host_taps("db4")
    flen = len(db4[0])

    def planes(shape, dtype, count):
        return lambda gen: list(_fill((1, count, *shape), dtype, gen).unbind(1))

    def image(shape, dtype):
        return lambda gen: [_fill((1, *shape), dtype, gen)]

    def coef(shape, n):
        return tuple((e + n - 1) // 2 for e in shape)

    fixed = lambda v: (lambda crops: v)  # noqa: E731
    # (the tiles whatever the measured routing says: from 2^20 samples on the synthesis of a plane goes to the wave strips by default,
    # csrc/mifwt_compose.hip:223; past the span no fused kernel takes the plane and the option changes nothing)
    always_tiles = ((_engine.OPT_TILE_MODE, 1), (_engine.OPT_PYRAMID_MODE, 2))
    fam = L.padded_family("db4", "symmetric", 2)
    for name, shape, fwd, inv, opts in (("7/8 tiles inside", INSIDE, {7}, {8}, always_tiles), ("7/8 tiles past", PAST, FALLBACK, FALLBACK, NO_SMALL),
                                        ("1/2 wave strips inside", INSIDE, {1}, {2}, NO_TILES)):
        huge(f"{name} wavedec2", fam, True, f32, image(shape, f32),
             lambda xs: _flat2(ptwt_amd.wavedec2(xs[0], "db4", mode="symmetric", level=1)), fwd, fixed(PADDED_TOL[f32]), opts=opts)
        huge(f"{name} waverec2", fam, False, f32, planes(coef(shape, flen), f32, 4),
             lambda xs: [ptwt_amd.waverec2([xs[0], tuple(xs[1:])], "db4")], inv, fixed(PADDED_TOL[f32]), opts=opts)
    # The families below have no span guard: their fused kernels form row x pitch in int64 (the audit above) and their launchers refuse
    # only ``coef_extent > 2^29`` per axis and more than INT32_MAX tiles, which no item that fits the device reaches behind ``validate``'s
    # INT32_MAX / 4 samples per axis.  So the fused id runs on both sides of 2^31 elements, and the second cell is where it must be right.
    bank = _per_bank(f32)
    for where, shape in (("inside", INSIDE), ("past", PAST_EVEN)):
        fam = L.per_family(bank)
        tol = lambda crops, fam=fam: TPER._value_tol(f32, RP.e_ref32(lambda *t: fam.fwd(list(t)) if len(t) == 1 else fam.inv(list(t), [None, None]),  # noqa: E731
                                                                     *crops, scale=float(torch.cat([c.reshape(-1) for c in crops]).norm())))
        huge(f"38/39 periodization {where} fwd", fam, True, f32, image(shape, f32),
             lambda xs: list(_per.level_fwd(xs[0], bank[0], bank[1]).unbind(1)), {38}, tol, RP.relerr)
        huge(f"38/39 periodization {where} inv", fam, False, f32, planes(coef(shape, 2), f32, 4),
             lambda xs, shape=shape: [_per.level_inv(list(xs), bank[2], bank[3], list(shape))], {39}, tol, RP.relerr)
    for where, shape in (("inside", INSIDE), ("past", PAST)):
        fam = L.ext_family(db4, "smooth")
        tol = lambda crops, fam=fam: TE._tol(f32, RE.e_ref32(lambda t: fam.fwd([t]) if t.dim() == 3 else fam.inv([t], [None, None]), *crops,  # noqa: E731
                                                             scale=float(crops[0].norm())))
        huge(f"42/43 smooth {where} fwd", fam, True, f32, image(shape, f32),
             lambda xs: list(_ext.level_fwd(xs[0], db4[0], db4[1], "smooth").unbind(1)), {42}, tol, RE.relerr)
        huge(f"42/43 smooth {where} adj", fam, False, f32, lambda gen, shape=shape: [_fill((1, 4, *coef(shape, flen)), f32, gen)],
             lambda xs, shape=shape: [_ext.level_adj(xs[0], db4[0], db4[1], "smooth", list(shape))], {43}, tol, RE.relerr)
        fam = L.cplx_family(db4, "symmetric")
        tol = lambda crops, fam=fam: TC._tol(c64, RC.e_ref32(lambda *t: fam.fwd(list(t)) if len(t) == 1 else fam.inv(list(t), [None, None]),  # noqa: E731
                                                             *crops, scale=float(torch.cat([c.reshape(-1) for c in crops]).norm())))
        out = tuple(2 * m - flen + 2 for m in coef(shape, flen))
        huge(f"46/47 complex64 {where} fwd", fam, True, c64, image(shape, c64),
             lambda xs: list(_cplx.level_fwd(xs[0], db4[0], db4[1], _engine.MODE_IDS["symmetric"]).unbind(1)), {46}, tol, RC.relerr,
             scope=_fused_complex, gib=44)
        huge(f"46/47 complex64 {where} inv", fam, False, c64, planes(coef(shape, flen), c64, 4),
             lambda xs, out=out: [_cplx.level_inv(list(xs), db4[2], db4[3], list(out))], {47}, tol, RC.relerr, scope=_fused_complex, gib=44)
        taps = TBK.random_bank(8)
        fam = L.boundary_family(taps, "symmetric", True)
        huge(f"26/27 boundary planes {where} fwd", fam, True, f32, image(shape, f32),
             lambda xs, taps=taps: list(_bwt.rows_level(xs[0], _bwt.bank(taps, "gramschmidt", "analysis"), _engine.MODE_IDS["symmetric"]).unbind(1)),
             {26}, fixed(TBK.LEVEL_TOL[f32]))
        huge(f"26/27 boundary planes {where} inv", fam, False, f32, planes(coef(shape, 2), f32, 4),
             lambda xs, taps=taps, shape=shape: [_bwt.transposed_level(list(xs), _bwt.bank(taps, "gramschmidt", "synthesis"), list(shape))],
             {27}, fixed(TBK.LEVEL_TOL[f32]))
    staps = tuple(TS2._quantised(t, f32) for t in TS2.random_bank(8, 99))
    for where, shape in (("inside", INSIDE), ("past", PAST_EVEN)):
        fam = L.swt2_family(staps, 0.25)
        huge(f"34/35 swt2 {where} fwd", fam, True, f32, image(shape, f32), lambda xs: list(st._level2_fwd(xs[0], staps, 1, 0.25).unbind(1)),
             set(), fixed(TS2.VALUE_TOL[f32]), counted=((st.KID_SWT2, 1), (st.KID_ISWT2, 0)), gib=50)
        huge(f"34/35 swt2 {where} inv", fam, False, f32, planes(shape, f32, 4), lambda xs: [st._level2_inv(list(xs), staps, 1, 0.25)],
             set(), fixed(TS2.VALUE_TOL[f32]), counted=((st.KID_SWT2, 0), (st.KID_ISWT2, 1)), gib=50)


_huge_families()


@pytest.mark.parametrize("h", HUGE, ids=lambda h: h.name.replace(" ", "-"))
def test_huge_item(h):
    run_huge(h)


def test_the_huge_table_covers_what_it_claims():
    """No GPU work: every family of the regime has a cell on either side of 2^31 elements (the tiles: of their span guard), analysis and
    synthesis; the item sizes are what the names say."""
    names = {h.name for h in HUGE}
    assert len(names) == len(HUGE)
    for family in ("7/8 tiles", "38/39 periodization", "42/43 smooth", "46/47 complex64", "26/27 boundary planes", "34/35 swt2"):
        assert len([n for n in names if n.startswith(family + " inside")]) == 2 and len([n for n in names if n.startswith(family + " past")]) == 2
    assert (INSIDE[0] - 1) * INSIDE[1] + INSIDE[1] < 1 << 29 <= (INSIDE[0] + 1) * (INSIDE[1] + 1) and INSIDE[0] % 2 == 0
    assert PAST[0] * PAST[1] > 1 << 31 and PAST_EVEN[0] * PAST_EVEN[1] > 1 << 31 and PAST[0] % 2 and PAST[1] % 2
    assert {h.analysis for h in HUGE} == {True, False} and all(h.gib <= 64 for h in HUGE)


@pytest.mark.parametrize("shape", [(1 << 30,), PAST], ids=["inside", "past"])
def test_huge_threshold(shape):
    """``threshold`` of ONE dense tensor on kernel 48: 2^30 elements, the longest row ``seg_geometry`` takes (csrc/mifwt_thresh.hip:357),
    as it is; and 46341 x 46349, which the host layer cuts into three rows of 715 953 003 elements.  Windows of 96 x 96 consecutive
    elements at both ends, in the middle, around elements 2^29 / 2^30 / 2^31 and around the two row cuts, element-wise (``check`` of
    tests/test_gpu_thresh.py)."""
    n = int(np.prod(shape))
    free = torch.cuda.mem_get_info()[0]
    if free < 3 * n * 4 + (4 << 30):
        pytest.skip(f"{3 * n * 4 / 2 ** 30:.1f} GiB needed, {free / 2 ** 30:.1f} GiB free")
    x = y = None
    try:
        x = _fill(shape, f32, torch.Generator(device=DEV).manual_seed(48), 2.0)
        _engine.level_events = []
        try:
            y = ptwt_amd.threshold(x, 0.5, "soft")
            tags = [(e[0], e[1]) for e in _engine.level_events]
        finally:
            _engine.level_events = None
        assert tags == [("thresh_fwd", 48)] and y.shape == x.shape and y.dtype == f32, tags
        size = L.WINDOW * L.WINDOW
        marks = [0, n // 2, n] + [m for m in L.OFFSET_MARKS if m < n] + ([n // 3, 2 * (n // 3)] if len(shape) == 2 else [])
        xf, yf = x.reshape(-1), y.reshape(-1)
        for mark in marks:
            start = min(max(mark - size // 2, 0), n - size)
            xs, ys = xf[start:start + size].cpu(), yf[start:start + size].cpu()
            TH.check(ys, xs, RT.threshold(_up(xs), 0.5, "soft"), 0.5, 0.0, f"threshold of {shape}, elements from {start}")
    finally:
        x = y = xf = yf = None
        torch.cuda.empty_cache()


ROW_SAMPLES = (2 ** 31 - 1) // 4  # the longest axis ``validate`` takes (csrc/mifwt_api.hip:25)


def _row_windows(rows, extent, buffers):
    """(row, start) of the windows of a 1-D output [rows, extent]: both ends and the middle of the first and the last row, and for every
    buffer ``(pitch, samples of it per output sample)`` the window around the element at which row x pitch + position crosses a mark."""
    size = min(L.WINDOW, extent)
    out = {(r, s) for r in (0, rows - 1) for s in L.axis_starts(extent)}
    for pitch, per in buffers:
        for mark in L.OFFSET_MARKS:
            row, pos = mark // pitch, int(mark % pitch / per)
            if row < rows:
                out.add((row, min(max(pos - size // 2, 0), extent - size)))
    return sorted(out)


def test_huge_rows_of_the_longest_extent():
    """Five rows of INT32_MAX / 4 = 536 870 911 samples (2 684 354 555 elements: rows 4 starts 4 elements below 2^31), ``wavedec`` and
    ``waverec`` at level 2 in "symmetric" on the chunked kernels 17 / 18 (which fuse two levels and more; a single level of such rows
    takes the axis passes): windows of 96 coefficients / samples of every output at both ends and in the middle of the first and last
    row and where row x pitch + position crosses 2^29, 2^30 and 2^31 elements of any buffer, against the oracle's single level applied
    twice on the crops the window depends on.  One sample more per row is the refusal pinned below."""
    rows, n, flen = 5, ROW_SAMPLES, 8
    m1 = (n + flen - 1) // 2
    m2 = (m1 + flen - 1) // 2
    n_out = 2 * m1 - flen + 2
    free = torch.cuda.mem_get_info()[0]
    if free < 40 << 30:
        pytest.skip(f"40 GiB needed, {free / 2 ** 30:.1f} GiB free")
    fam = L.padded_family("db4", "symmetric", 1)
    tol = PADDED_TOL[f32]
    gen = torch.Generator(device=DEV).manual_seed(1718)
    x = c = y = None

    def traced(fn, kid):
        _engine.level_events = []
        try:
            out = fn()
            kids = {e[1] for e in _engine.level_events}
        finally:
            _engine.level_events = None
        assert kids == {kid}, (kids, kid)
        return out

    def row_of(t, row):
        return lambda idx: [_up(L.take(t[row:row + 1], idx).cpu())]

    def close(got, want, what):
        err = TP.G.relerr(_up(got.cpu()).numpy(), want.numpy())
        _record("17/18 rows of INT32_MAX / 4 samples", err / tol)
        assert got.shape == want.shape and err < tol, f"{what}: {err:.3e} >= {tol:.3e}"

    try:
        x = _fill((rows, n), f32, gen)
        a2, d2, d1 = traced(lambda: ptwt_amd.wavedec(x, "db4", mode="symmetric", level=2), 17)
        assert a2.shape == (rows, m2) and d1.shape == (rows, m1)
        for row, w0 in _row_windows(rows, m1, [(d1.stride(0), 1), (n, 2)]):
            want = L.window_reference(fam, True, row_of(x, row), (n,), (m1,), (w0,))[1]
            close(d1[row:row + 1, w0:w0 + L.WINDOW], want, f"d1 row {row} from {w0}")
        for row, w0 in _row_windows(rows, m2, [(a2.stride(0), 1), (n, 4)]):
            idx, off, _, _ = L.axis_crop(w0, L.WINDOW, m1, 2, fam.guard, False, True)
            lo, hi = int(idx[0]), int(idx[-1]) + 1
            a1 = L.window_reference(fam, True, row_of(x, row), (n,), (m1,), (lo,), size=hi - lo)[0]
            for got, want, what in zip((a2, d2), fam.fwd([a1]), ("a2", "d2")):
                close(got[row:row + 1, w0:w0 + L.WINDOW], want[..., off:off + L.WINDOW], f"{what} row {row} from {w0}")
        x = a2 = d2 = d1 = None
        c = [_fill((rows, 2, m2), f32, gen), _fill((rows, m1), f32, gen)]
        a2, d2, d1 = c[0][:, 0], c[0][:, 1], c[1]
        y = traced(lambda: ptwt_amd.waverec([a2, d2, d1], "db4"), 18)
        assert y.shape == (rows, n_out)
        for row, w0 in _row_windows(rows, n_out, [(n_out, 1), (m1, 0.5), (a2.stride(0), 0.25)]):
            idx, off, _, _ = L.axis_crop(w0, L.WINDOW, m1, 2, fam.guard, False, False)
            lo, hi = int(idx[0]), int(idx[-1]) + 1
            a1 = L.window_reference(fam, False, lambda i: [row_of(a2, row)(i)[0], row_of(d2, row)(i)[0]], (m2,), (m1,), (lo,), size=hi - lo)[0]
            want = fam.inv([a1, _up(d1[row:row + 1, lo:hi].cpu())], [None])[0]
            close(y[row:row + 1, w0:w0 + L.WINDOW], want[..., off:off + L.WINDOW], f"y row {row} from {w0}")
        print(f"rows of {n} samples: peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB, worst / bound "
              f"{WORST['17/18 rows of INT32_MAX / 4 samples']:.3f}")
    finally:
        x = c = y = a2 = d2 = d1 = None
        torch.cuda.empty_cache()


def test_a_row_of_2_to_the_29_samples_is_refused_without_a_launch():
    """A documented limit (limits at large sizes): an extent above INT32_MAX / 4 = 2^29 - 1 samples is refused by the level
    descriptor's check (``validate``, csrc/mifwt_api.hip) with a RuntimeError that names the library; nothing is launched."""
    x = torch.zeros((1, 1 << 29), dtype=f32, device=DEV)
    before = [_engine.launch_count(k) for k in range(64)]
    with pytest.raises(RuntimeError, match="libmifwt: bad argument"):
        ptwt_amd.wavedec(x, "db2", mode="zero", level=1)
    torch.cuda.synchronize()
    assert [_engine.launch_count(k) for k in range(64)] == before
    del x
    torch.cuda.empty_cache()


def test_the_table_covers_what_it_claims():
    """No GPU work: every cell names its buffers' strides, analysis and synthesis both occur per family, names are unique, and every
    batch puts every buffer past its mark with a sample set of a few dozen items."""
    assert len({c.name for c in CELLS}) == len(CELLS)
    reached = set().union(*[c.kids for c in CELLS])
    # every id of the table (34 - 37 through the launch counters, next line): not the matrix-core kernels 11 / 23 — test_full_size_config5_*
    # of tests/test_gpu_parity.py runs them at 2^33 elements — and not 49, which the threshold's backward leg below asserts
    assert reached == set(range(0, 11)) | {12, 13, 14, 15, 16, 17, 18, 20, 21, 22} | set(range(24, 34)) | set(range(38, 49)), sorted(reached)
    assert {k for c in CELLS for k, n in c.counted if n} == {34, 35, 36, 37}
    assert {c.dtype for c in CELLS} == {f16, f32, f64, c64}
    for c in CELLS:
        batch = L.batch_over(MARK[c.dtype], c.strides)
        assert all(s * batch > MARK[c.dtype] for s in c.strides) and (batch - 3) * min(c.strides) <= MARK[c.dtype], c.name
        esz = torch.empty((), dtype=c.dtype).element_size()
        assert len(L.sample_items(batch, [(s, esz) for s in c.strides + c.minor], c.seed, c.nrandom)) <= 64, c.name
        assert sum(c.strides + c.minor) * batch * esz < 40 << 30, c.name


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    """After the module's last test, whichever tests were selected: the worst error of every cell that ran, relative to its bound."""
    yield
    print("\nworst error / bound:", {k: float(f"{v:.3g}") for k, v in sorted(WORST.items())})
