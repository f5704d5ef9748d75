"""GPU tests (``-m gpu``) of the order-statistic, sparse and packing kernels (ids 50 .. 60) on buffers that cross 2^31 elements and 2^32
bytes: the sibling of tests/test_gpu_large_offsets.py, whose audit and tables end at ids 48 / 49, under the same regime and rules.  The
driver (``Cell``, ``run_cell``, the route assertions, the sampled items, the batch slices) is imported from that module, the helpers
from tests/_large_ref.py.  A wrapped offset does not crash: loads return 0 and stores are dropped; the result is silently wrong.

Regime MANY (``POST``, ``test_cell``; ``PACK``, ``test_pack_cell``).  One cell = one call on a batch of small items with every buffer it
lists past the mark of its dtype (``MARK``: 2^31 float32 elements, 2^29 float64 = 2^32 bytes, 2^32 float16, 2^28 complex128 = 2^32
bytes).  Per cell, as there: 1. the kernel ids of the call on the whole batch and on every slice; 2. sampled items
(``_large_ref.sample_items``) against the family's numpy reference; 3. every item against the same call on slices of at most 2^28
elements.
  50 / 51  ``estimate_sigma``: images of 63 x 65 (LDS-resident) and 1023 x 1025 (streaming, ``FORCE_STREAM``; 32 KiB of counters per
           image: 64 MiB), float32 and float64; the two order statistics bit for bit against tests/_estimator_ref.py and sigma within
           an ulp, as tests/test_gpu_estimators.py compares; slices ``torch.equal``.  One cell reads the diagonal band of a level-1
           ``wavedec2`` container (a plane of the level buffer: its image stride is four planes), one cell data of 8 magnitudes.
  52 / 53  band moments, BayesShrink and VisuShrink thresholds of the strided planes of one level buffer with one sigma per image:
           ``check_thresholds`` / the moments bound ``n 2^-53`` / the VisuShrink bound ``4 eps`` of tests/test_gpu_estimators.py per
           sampled image; slices under the floor of those rules (4 eps, n 2^-53; the sums are added in a fixed order per image).
  54 / 55  ``keep_threshold`` with an int and with one k per image from a device tensor (``dk_stride`` 1), then ``sparsify`` "hard",
           which runs kernel 48 with the per-image values: the value bit for bit against tests/_sparsify_ref.py, the output with the
           exact decisions of tests/test_gpu_thresh.py (``check``); slices ``torch.equal``.  One cell pools the three strided detail
           planes of a level buffer, with 8 magnitudes and "soft".
  56 / 57 / 58  ``sparse_encode`` / ``sparse_decode``, per route ``keep = n - 3`` (the compacted buffers pass the mark: ``g * cap``)
           and ``keep = n / 64`` (they are ``minor``): values, int32 indices and counts bit for bit against tests/_sparse_ref.py; the
           decoded batch ``torch.equal`` to ``sparsify(..., "hard")`` slice by slice on tie-free data; one streaming cell with 8
           magnitudes (the tie quota decided in items past the mark).
  59 / 60  ``coeffs_to_array`` / ``ravel_coeffs`` and the ``copy=True`` inverses, EVERY element: ``torch.equal`` to the torch composition
           (``torch.full`` plus slice assignment, ``torch.cat``) built slice by slice, padding -7.5, with ``COMPOSED_CELLS`` emptied as
           tools/pack_bench.py does for its kernel legs.  Containers with the shapes and strides of ``wavedec2`` db4 level 3 of 33 x 33
           images (gaps, bands of 10 / 13 / 20 elements a row: narrower than a vector row) in float32, float16 and complex128, and of
           ``wavedec3`` db2 level 2 of 17^3 volumes in float32, built from random level buffers.

Regime HUGE: one item at the in-item guards, checked by COUNTS, not by a sort: v is the k-th largest magnitude iff it occurs and
``count(|x| > v) < k <= count(|x| >= v)`` (``_large_ref.is_kth_largest``, integer comparisons in chunks, pinned on the CPU against
``numpy.sort`` by tests/test_large_ref_host.py); the median of ``estimate_sigma`` is the mean of the order statistics of
``_large_ref.median_ranks``.
  ``test_huge_image_inside``  46340 x 46340 float32 (2 147 395 600 elements, the last square below 2^31), dense and as a view with a
           row pitch of 46344 (row x pitch crosses 2^31 inside the item): 51, 55 for k in {1, 1000, n // 2, n - 1}, 57 with k = 1000
           (indices ascending and unique, ``values == x.flatten()[indices]``, every kept magnitude ``>=`` the value).
  ``test_huge_image_past``  46341 x 46341 (2 147 488 281): no kernel of 50 .. 58 launches and every call raises a ``ValueError`` that
           names the limit (THE DEFECT below).
  ``test_huge_row``  a dense [1, 2^30 + 4096] tensor: ``thresholding._geometry`` cuts the row in two; 51 / 55 by counts.
  ``test_huge_pack``  the haar level-1 container of a 46342 x 46350 image from random bands: 59 / 60, ``torch.equal`` to slice
           assignment.  ``test_pack_rows_past_the_guard_are_composed``: a 1-D float16 container of 2^31 + 8 rows of 2 samples makes
           ``mifwt_pack_plan`` answer negative: no 59 launch, bit-equal to the composition.

The audit (read before the first run: every product that forms an offset, a unit count or a grid size; "i64" = formed in 64 bits):
  bands  csrc/mifwt_bands.h ``visit_slot``: ``row`` is uint32 (``g * rp + r``, below the band's rows < 2^31, line 125), split into int64
       ``i0``, ``i1`` (line 77) and multiplied with the int64 strides: ``i0 * b.s0 + i1 * b.s1`` i64 (line 78); columns int64 (80 - 90).
       ``band_geometry``: ``n <= 2^30``, ``e1 <= 2^30``, ``e0 e1 < 2^31`` (line 125), ``rp n < 2^31`` (line 129); slots per row at most n
       (line 134), so slots per image < 2^31.  ``pool_of``: images < 2^31 (line 150), pooled count < 2^31 (line 158).  ``unit_plan``
       (165 - 173) in uint64.
  50   csrc/mifwt_estim.hip ``select_lds_kernel``: ``g * b.rp + r`` uint32 below the rows (line 76), LDS index ``r * b.n + c`` below the
       capacity; grid = images < 2^31 (line 328).
  51   ``select_stream_kernel``: counters ``(size_t)g * 2 * kStreamBins`` i64 (170, 190), states ``(size_t)(pass & 1) * images + g`` i64
       (168, 171), chunk ``t0 = w * spw < slots < 2^31`` (179); grid ``wgs * images`` behind ``< 2^31`` (334; ``wgs <= max(1, 4096 /
       images)``, so the guard cannot fire behind ``band_geometry``); host sizes in size_t (317 - 320, 335).
  52   ``moments_kernel``: ``uint32 u`` grid-stride below ``total < 2^31`` (238; ``build_moments`` line 428), ``part[u]``;
       ``thresholds_kernel``: ``uint64 i`` over ``nseg * images`` (281 - 283), ``part + ustart + (size_t)g * ppi`` i64 (289).
  53   the same ``thresholds_kernel``; grid ``nseg * images / 256`` in uint64 (473 - 474).
  54   csrc/mifwt_select.hip ``kth_lds_kernel``: as 50, ``keys[kbase + r * n + c]`` below the capacity (102); ``dk[(int64_t)g * stride]``
       (mifwt_bands.h:104).
  55   ``kth_stream_kernel``: counters ``(size_t)g * kStreamBins`` (176, 192), states ``(size_t)(pass & 1) * images + g`` (174, 177),
       ``t0 = w * spw`` (183); the 32-bit unit prefix ``ustart`` behind ``total >= 2^31`` of ``fill_units`` (239 - 241), checked for
       every launch before anything is enqueued (271 - 272); ``zero_counters_kernel`` in size_t (200 - 202).
  56   csrc/mifwt_compact.hip ``compact_lds_kernel``: outputs ``(size_t)g * a.cap`` i64 (116 - 117, ``fill_padding`` 81 - 82).
  57   ``compact_count_kernel`` / ``compact_write_kernel``: table ``2 * ((size_t)g * upi + ubase + w)`` i64 (161, 200), outputs
       ``(size_t)g * cap`` (203 - 204), the int32 index ``fbase + r * n + c`` below the pooled count < 2^31 (224); ``ustart`` behind
       ``launch * images >= 2^31`` of ``units_per_image`` (279), ``upi < 2^31`` (318); ``compact_scan_kernel`` ``2 * (size_t)g * upi`` (172).
  58   ``compact_move_kernel``: ``uint64 id`` over ``images * cap`` (248 - 251), element ``g * (uint64)(size) + (i - start)`` i64 (260);
       pooled sizes < 2^31 (425), grid behind ``< 2^31`` (432).
  59 / 60  csrc/mifwt_pack.hip ``pack_kernel``: ``uint32 u`` grid-stride below ``total < 2^31`` (89; ``build_args`` line 179), ``r0 = lu *
       rb < rows < 2^31`` (110; rows line 137, row and inner extents line 135), ``rows * upr`` units in uint64 (146); box bases
       ``i0 * ds[0] + i1 * ds[1] + (int64_t)i2 * ds[2]`` i64 (105 - 106, 117 - 118), columns ``(c0 + j) * st`` int64 (70, 80).
       coeff_array.py falls back to the composition where ``mifwt_pack_plan`` answers negative (``_within``, lines 395 - 406, read at
       438, 464, 498).
  Python  estimators.py ``_band`` (122 - 133) answers None from ``_COUNT_LIMIT`` = 2^31 elements per image on, ``_check_count`` (156 -
       162) refuses such an image before that; sparsify.py ``_value`` (line 171) refuses the pool at the same limit; sparse.py
       ``_arguments`` (line 332) at ``_INDEX_LIMIT`` = 2^31 (int32 indices).  ``_band`` goes through ``thresholding._geometry``: a dense
       image of more than 2^30 elements is cut into equal rows (``_split_row``).
No 32-bit product that a legal call overflows was found in these kernels.  THE DEFECT is on the far side of ``_COUNT_LIMIT``: the
composition that ``estimate_sigma`` / ``keep_threshold`` / ``sparsify`` took there is a ``torch.sort`` of the image, which refuses a
sorted axis of more than 2^31 - 1 elements with a ``RuntimeError`` from inside torch — every pool the kernels hand over for its size
was one the composition could not serve.  Fixed in estimators.py / sparsify.py: a pool of 2^31 elements per image and more raises a
``ValueError`` that names the limit before anything is launched, as ``sparse_encode`` always did (``test_huge_image_past``).

Which test sits on which side of a guard (inside: the kernel answers right; past: refused or composed; host: the return codes of the C
entries without a device, tests/test_*_host.py):
  n <= 2^30 per row        inside ``test_huge_row`` (a row of 2^30 + 4096 is cut in two) and ``test_huge_image_inside`` (two rows of
                           1 073 697 800); past: host (``n = 2^30 + 1`` refused), and Python never hands over such a row.
  rp n, pooled count < 2^31  inside ``test_huge_image_inside``; past ``test_huge_image_past``; host rows 2^31 - 1 / 2^31.
  rows, images < 2^31      host only (2^31 rows need 8 GiB of one-element rows and 32 TiB of counters).
  units < 2^31             host (moments plan, compaction workspace, pack plan); the selection's unit guards sit behind the data
                           pointers and need 89 million images of more than 12288 elements: not reachable on one device.
  int32 indices            inside ``test_huge_image_inside`` (57, indices up to 2 147 395 599); past ``test_huge_image_past``.
  pack rows / row length   inside ``test_huge_pack``; past ``test_pack_rows_past_the_guard_are_composed``; host pack rows and units.

Memory: a MANY cell holds 8 - 36 GiB (inputs, outputs and one slice; stated per cell as ``run_cell`` computes it, per pack cell and
per HUGE test in GiB); a test skips only when ``torch.cuda.mem_get_info`` shows less.  Data: seeded ``normal_()`` on the device;
tie-free where the check needs it (``_tie_free``); quantised to 8 magnitudes in one cell per selection family (``_quantise``).  No bound
is new: selection, compaction and packing are bit-exact, moments and thresholds use the bounds of tests/test_gpu_estimators.py.
``WORST_ON_MI355X`` is a record (printed by the module's last test), not a bound.
"""
import contextlib
import importlib
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, estimators as E
from ptwt_amd.constants import WaveletDetailTuple2d
from tests import _estimator_ref as RE
from tests import _large_ref as L
from tests import _pack_ref as RP
from tests import _sparse_ref as RSP
from tests import _sparsify_ref as RS
from tests import _thresh_ref as RT
from tests import test_gpu_estimators as TGE
from tests import test_gpu_large_offsets as M
from tests import test_gpu_thresh as TH
from tests.test_gpu_large_offsets import DEV, WORST, Cell, _fill, _forced, _record, _thresh_every, _up, run_cell

pytestmark = pytest.mark.gpu

S = importlib.import_module("ptwt_amd.sparse")
SP = importlib.import_module("ptwt_amd.sparsify")
C = importlib.import_module("ptwt_amd.coeff_array")

f16, f32, f64, c128 = torch.float16, torch.float32, torch.float64, torch.complex128
#: elements a cell's buffers must exceed, per dtype: the marks of tests/test_gpu_large_offsets.py, and 2^32 bytes of complex128
MARK = {**M.MARK, c128: 1 << 28}
PAD = -7.5
# worst error over the bound in force of this module on an MI355X (printed by its last test); a record, not a bound
WORST_ON_MI355X = {
    "every bit-exact cell (50 / 51, 54 - 60, the HUGE items), samples and slices": 0.0,
    "52/53 thresholds float32": 0.106, "52/53 thresholds float64": 4e-4,  # (the BayesShrink thresholds; moments and VisuShrink below them)
    "52/53 thresholds, whole batch against its slices": 0.0,  # (bit-identical)
}  # no skip; the slowest test 1.9 s, the module 22 s
POST = []


def cell(name, kids, dtype, strides, make, call, sample, every, scope=contextlib.nullcontext, minor=(), nrandom=8):
    POST.append(Cell(name, set(kids), dtype, tuple(strides), make, call, sample, every, (), scope, 9500 + len(POST), tuple(minor), (), nrandom))


# ---- data ------------------------------------------------------------------------------------------------------------------------
def _in_slices(t, fn):
    """``fn(view)`` in place on consecutive parts of ``t`` of at most 2^28 elements along its first axis."""
    per = max(1, L.SLICE_ELEMENTS // max(1, t[0].numel()))
    for s in range(0, t.shape[0], per):
        fn(t[s:s + per])


def _quantise(t):
    """``t`` in place with 8 distinct magnitudes, 0.25 .. 2.0, signs kept: every order statistic is decided among heavy ties."""
    def fn(v):
        q = v.abs().mul_(3).floor_().clamp_(max=7).add_(1).mul_(0.25)
        v.copy_(torch.where(v < 0, -q, q))
    _in_slices(t, fn)
    return t


def _tie_free(t):
    """``t`` [B, n] in place with distinct magnitudes per image: ``|x|`` rounded down to a multiple of ``2^(low - 22)`` below 4 plus
    ``(j + 1) 2^-22`` at position j, ``low = ceil(log2(n + 1))`` — exact in float32 (24 bits below 4), signs kept."""
    n = t.shape[1]
    low = math.ceil(math.log2(n + 1))
    assert low <= 20
    step = 2.0 ** (low - 22)
    pos = torch.arange(1, n + 1, device=t.device, dtype=t.dtype) * 2.0 ** -22

    def fn(v):
        m = v.abs().clamp_(max=3.9).div_(step).floor_().mul_(step).add_(pos)
        v.copy_(torch.where(v < 0, -m, m))
    _in_slices(t, fn)
    return t


def _same(got, want, what):
    assert TGE.same_bits(got, want), what


def _equal_every(c, k, whole, part, inputs, start):
    _thresh_every(c, k, whole, part, inputs, start)  # (``torch.equal``, the first item that differs named)


# ---- 50 / 51: estimate_sigma -----------------------------------------------------------------------------------------------------
def _sigma_sample(c, items, xs, gots):
    xn = xs[0].numpy()
    _same(gots[0].numpy(), RE.order_stats(xn, 1), f"{c.name}: order statistics")
    TGE.within_ulp(gots[1].numpy(), RE.estimate_sigma(xn, 1), f"{c.name}: sigma")
    _record(c.name, 0.0)


def _sigma_call(xs):
    return [E._order_stats(xs[0], 1), ptwt_amd.estimate_sigma(xs[0], lead=1)]


def sigmas():
    for dtype, route, shape in ((f32, "lds", (63, 65)), (f64, "lds", (63, 65)), (f32, "stream", (1023, 1025)), (f64, "stream", (1023, 1025))):
        kid = 51 if route == "stream" else 50
        cell(f"{kid} estimate_sigma {str(dtype)[6:]}", {kid}, dtype, (shape[0] * shape[1],),
             lambda b, gen, dtype=dtype, shape=shape: [_fill((b, *shape), dtype, gen, 3.0)], _sigma_call, _sigma_sample, _equal_every,
             _forced(E, "FORCE_STREAM", route == "stream"), minor=(2,))
    cell("50 estimate_sigma 8 magnitudes", {50}, f32, (63 * 65,), lambda b, gen: [_quantise(_fill((b, 63, 65), f32, gen))], _sigma_call,
         _sigma_sample, _equal_every, minor=(2,))
    # the diagonal band of a level-1 wavedec2 container: a plane of the level buffer [B, 4, 66, 65], not contiguous
    h, w, m0, m1 = 126, 124, 66, 65

    def band(b, gen):
        d = ptwt_amd.wavedec2(_fill((b, h, w), f32, gen), "db4", mode="symmetric", level=1)[1].diagonal
        assert tuple(d.shape) == (b, m0, m1) and d.stride() == (4 * m0 * m1, m1, 1) and not d.is_contiguous()
        return [d]

    cell("50 estimate_sigma strided band", {50}, f32, (4 * m0 * m1,), band, _sigma_call, _sigma_sample, _equal_every, minor=(2,))


# ---- 52 / 53: band moments, BayesShrink and VisuShrink thresholds --------------------------------------------------------------------
def thresholds(dtype, m=67):
    eps = float(torch.finfo(dtype).eps)
    n = m * m

    def make(b, gen):
        buf = _fill((b, 4, m, m), dtype, gen)
        buf[:, 1].mul_(2.0)    # well conditioned: mean(d^2) = 4 against sigma^2 <= 0.5625
        buf[:, 2].mul_(0.25)   # mean(d^2) < sigma^2: the clamp
        sigma = (torch.randint(4, 7, (b,), device=DEV, generator=gen).to(dtype) / 8)
        return [*buf.unbind(1), sigma]

    def call(xs):
        coeffs = [xs[0], WaveletDetailTuple2d(*xs[1:4])]
        bayes = ptwt_amd.estimate_thresholds(coeffs, "bayes", xs[4])
        visu = ptwt_amd.estimate_thresholds(coeffs, "visu", xs[4])
        return [*bayes[1], *visu[1], *E._band_moments(coeffs)[1]]

    def sample(c, items, xs, gots):
        coeffs = [xs[0], WaveletDetailTuple2d(*xs[1:4])]
        sig = xs[4].double().numpy()
        clamped = TGE.check_thresholds([None, WaveletDetailTuple2d(*gots[0:3])], coeffs, sig, dtype, c.name)
        assert clamped == len(items)  # the 0.25 sigma band of every image
        cn = TGE.to_np(coeffs)
        ref = RE.leaves(RE.estimate_thresholds(cn, "bayes", sigma=sig)[1:])
        for got, want, t in zip(gots[0:3], ref, cn[1]):
            _, tol = TGE.threshold_tolerance(t, 1, sig, eps)
            _record(c.name, float((np.abs(got.double().numpy() - want) / want / tol).max()))
        visu = RE.leaves(RE.estimate_thresholds(cn, "visu", sigma=sig)[1:])
        for got, want in zip(gots[3:6], visu):
            err = np.abs(got.double().numpy() - want)
            _record(c.name, float((err / (4 * eps * want)).max()))
            assert bool((err <= 4 * eps * want).all()), f"{c.name}: visu"
        for got, t in zip(gots[6:9], cn[1]):
            want = RE.moments(t, 1)
            rel = np.abs(got.numpy() - want) / want
            _record(c.name, float(rel.max() / (n * TGE.U)))
            assert got.dtype == f64 and bool((rel <= n * TGE.U).all()), f"{c.name}: moments"

    def every(c, k, whole, part, inputs, start):
        floor = n * TGE.U if k >= 6 else 4 * eps
        rel = ((whole.double() - part.double()).abs() / part.double().abs())
        worst = float(rel.max())
        _record(c.name + " slices", worst / floor)
        assert worst <= floor, f"{c.name}: output {k}, item {start + int(rel.argmax())} whole batch against its slice: {worst:.3e} > {floor:.3e}"

    cell(f"52/53 thresholds {str(dtype)[6:]}", {52, 53}, dtype, (4 * n,), make, call, sample, every)


# ---- 54 / 55: keep_threshold, sparsify -----------------------------------------------------------------------------------------------
def _check_kept(c, xs_pool, k, got_v, what):
    """The value bit for bit against the reference; returns it as float64 [images, 1]."""
    want = RS.kth([t.numpy() for t in xs_pool], 1, k)
    _same(got_v.numpy(), want, f"{c.name}: {what}")
    return torch.from_numpy(want.astype(np.float64)).reshape(-1, 1)


def kept(dtype, route, n):
    kid = 55 if route == "stream" else 54
    k0 = n // 3

    def make(b, gen):
        d = _fill((b, n), dtype, gen, 2.0)
        return [d, torch.zeros((b, 1), dtype=dtype, device=DEV), torch.randint(0, n + 1, (b,), device=DEV, generator=gen)]

    def call(xs):
        coeffs = [xs[1], xs[0]]
        return [ptwt_amd.keep_threshold(coeffs, k0), ptwt_amd.keep_threshold(coeffs, xs[2]), ptwt_amd.sparsify(coeffs, xs[2], "hard")[1]]

    def sample(c, items, xs, gots):
        _check_kept(c, xs[:1], k0, gots[0], f"k = {k0}")
        v = _check_kept(c, xs[:1], xs[2].numpy(), gots[1], "k per image")
        TH.check(gots[2], xs[0], RT.threshold(_up(xs[0]), v, "hard"), v, 0.0, f"{c.name}: sparsify")
        _record(c.name, 0.0)

    cell(f"{kid}+48 keep_threshold sparsify {str(dtype)[6:]}", {kid, 48}, dtype, (n,), make, call, sample, _equal_every,
         _forced(SP, "FORCE_STREAM", route == "stream"))


def kept_bands(m=63):
    """The three strided detail planes of one level buffer pooled (3 m^2 = 11907 elements, inside the LDS route), 8 magnitudes, "soft"."""
    k0 = m * m

    def make(b, gen):
        return list(_quantise(_fill((b, 4, m, m), f32, gen)).unbind(1))

    def call(xs):
        coeffs = [xs[0], WaveletDetailTuple2d(*xs[1:4])]
        return [ptwt_amd.keep_threshold(coeffs, k0), *ptwt_amd.sparsify(coeffs, k0, "soft")[1]]

    def sample(c, items, xs, gots):
        v = _check_kept(c, xs[1:4], k0, gots[0], f"k = {k0}").reshape(-1, 1, 1)
        for k in range(3):
            TH.check(gots[1 + k], xs[1 + k], RT.threshold(_up(xs[1 + k]), v, "soft"), v, 0.0, f"{c.name}: band {k}")
        _record(c.name, 0.0)

    cell("54+48 keep_threshold sparsify bands 8 magnitudes", {54, 48}, f32, (4 * m * m,), make, call, sample, _equal_every, minor=(m * m,))


# ---- 56 / 57 / 58: sparse_encode, sparse_decode ------------------------------------------------------------------------------------------
def sparse(route, n, keep, ties=False):
    kids = {55, 57, 58} if route == "stream" else {54, 56, 58}
    past = keep > n // 2

    def make(b, gen):
        d = _fill((b, n), f32, gen)
        return [_quantise(d) if ties else _tie_free(d), torch.zeros((b, 1), dtype=f32, device=DEV)]

    def call(xs):
        s = ptwt_amd.sparse_encode([xs[1], xs[0]], keep)
        return [s.values, s.indices, s.counts, ptwt_amd.sparse_decode(s)[1]]

    def sample(c, items, xs, gots):
        want = RSP.encode([xs[0].numpy()], 1, keep, keep)
        for k, what in enumerate(("values", "indices", "counts")):
            _same(gots[k].numpy(), want[k], f"{c.name}: {what}")
        _same(gots[3].numpy(), RSP.decode(*want, [tuple(xs[0].shape)], 1)[0], f"{c.name}: decoded")
        _record(c.name, 0.0)

    def every(c, k, whole, part, inputs, start):
        _equal_every(c, k, whole, part, inputs, start)
        if k == 3 and not ties:  # the rule of tests/test_gpu_sparse.py: decode equals sparsify "hard" where the k-th magnitude is not tied
            dense = ptwt_amd.sparsify([inputs[1], inputs[0]], keep, "hard")[1]
            assert torch.equal(whole, dense), f"{c.name}: decoded against sparsify, items from {start}"

    name = f"{'55+57+58' if route == 'stream' else '54+56+58'} sparse keep {'n - 3' if past else 'n / 64'}{' 8 magnitudes' if ties else ''}"
    cell(name, kids, f32, (n, keep) if past else (n,), make, call, sample, every, _forced(S, "FORCE_STREAM", route == "stream"),
         minor=() if past else (keep,))


sigmas()
thresholds(f32)
thresholds(f64)
kept(f32, "lds", 4095)
kept(f64, "lds", 4095)
kept(f32, "stream", (1 << 20) - 1)
kept_bands()
for _route, _n in (("lds", 4095), ("stream", (1 << 20) - 1)):
    sparse(_route, _n, _n - 3)
    sparse(_route, _n, _n // 64)
sparse("stream", (1 << 20) - 1, ((1 << 20) - 1) // 64, ties=True)


@pytest.mark.parametrize("c", POST, ids=lambda c: c.name.replace(" ", "-"))
def test_cell(c):
    run_cell(c)


# ---- 59 / 60: packing, every element -------------------------------------------------------------------------------------------------
PackCell = namedtuple("PackCell", "name dtype fmt buffers gib")
PACK = [
    PackCell("59/60 wavedec2 db4 L3 33x33 f32", f32, "wavedec2", ((4, 10, 10), (3, 13, 13), (3, 20, 20)), 36),
    PackCell("59/60 wavedec2 db4 L3 33x33 f16", f16, "wavedec2", ((4, 10, 10), (3, 13, 13), (3, 20, 20)), 36),
    PackCell("59/60 wavedec2 db4 L3 33x33 c128", c128, "wavedec2", ((4, 10, 10), (3, 13, 13), (3, 20, 20)), 36),
    PackCell("59/60 wavedec3 db2 L2 17^3 f32", f32, "wavedecn", ((8, 6, 6, 6), (8, 10, 10, 10)), 36),
]
KEYS = {2: ("da", "ad", "dd"), 3: M.KEYS3}


def _levels(bufs):
    """(approximation, per level {key: plane}) over the planes of the level buffers ``bufs``, the strided views a transform returns:
    plane 0 of the coarsest buffer and the last 2^d - 1 planes of every buffer (2-D: [B, 4, ...] then [B, 3, ...]; 3-D: [B, 8, ...]
    throughout, the first plane of a finer level unused)."""
    keys = KEYS[bufs[0].dim() - 2]
    return bufs[0][:, 0], [dict(zip(keys, buf[:, buf.shape[1] - len(keys):].unbind(1))) for buf in bufs]


def _container(fmt, approx, levels):
    if fmt == "wavedec2":
        return (approx, *[WaveletDetailTuple2d(lv["da"], lv["ad"], lv["dd"]) for lv in levels])
    return (approx, *[dict(lv) for lv in levels])


def _entry(e):
    return dict(zip(KEYS[2], e)) if isinstance(e, tuple) else e


def _pack_events(fn):
    _engine.level_events = []
    try:
        out = fn()
        return out, [e[1] for e in _engine.level_events]
    finally:
        _engine.level_events = None


def _equal_in_slices(got, want, item, what):
    for s, e in L.batch_slices(got.shape[0], item):
        assert torch.equal(got[s:e], want[s:e]), f"{what}: items {s} .. {e}"


def run_pack(p):
    free = torch.cuda.mem_get_info()[0]
    if free < p.gib << 30:
        pytest.skip(f"{p.name}: {p.gib} GiB needed, {free / 2 ** 30:.1f} GiB free")
    d = len(p.buffers[0]) - 1
    ext = [sum(b[1 + a] for b in p.buffers) + p.buffers[0][1 + a] for a in range(d)]  # a + sum of the levels' extents, per axis
    per_arr = math.prod(ext)
    per_flat = math.prod(p.buffers[0][1:]) + sum((2 ** d - 1) * math.prod(b[1:]) for b in p.buffers)
    batch = L.batch_over(MARK[p.dtype], (per_arr, per_flat))
    torch.cuda.reset_peak_memory_stats()
    gen = torch.Generator(device=DEV).manual_seed(9700 + PACK.index(p))
    bufs = arr = flat = back = None
    try:
        with _forced(C, "COMPOSED_CELLS", set())():
            bufs = [_fill((batch, *b), p.dtype, gen) for b in p.buffers]
            approx, levels = _levels(bufs)
            coeffs = _container(p.fmt, approx, levels)
            assert not approx.is_contiguous()
            # ---- coeffs_to_array: kernel 59, gaps filled with the padding
            (arr, slices), ids = _pack_events(lambda: ptwt_amd.coeffs_to_array(coeffs, PAD))
            assert ids == [59] and tuple(arr.shape) == (batch, *ext) and arr.numel() > MARK[p.dtype]
            two = _container(p.fmt, *_levels([b[:2] for b in bufs]))
            want2, wslices = RP.to_array(RP.cpu(two), PAD)
            assert slices == wslices and RP.same_bits(arr[:2], want2)  # (the layout itself, against tests/_pack_ref.py)
            tensors = [approx] + [lv[k] for lv, sl in zip(levels, slices[1:]) for k in sl]
            index = [slices[0]] + [sl[k] for sl in slices[1:] for k in sl]
            gaps = per_arr - per_flat
            assert gaps > 0
            for s, e in L.batch_slices(batch, per_arr):
                ref = torch.full((e - s, *ext), PAD, dtype=p.dtype, device=DEV)
                for t, sl in zip(tensors, index):
                    ref[sl] = t[s:e]
                assert torch.equal(arr[s:e], ref), f"{p.name}: coeffs_to_array, items {s} .. {e}"
                del ref
            # ---- array_to_coeffs(copy=True): kernel 60
            back, ids = _pack_events(lambda: ptwt_amd.array_to_coeffs(arr, slices, p.fmt, copy=True))
            assert ids == [60]
            got = [back[0]] + [_entry(e)[k] for e, sl in zip(back[1:], slices[1:]) for k in sl]
            for g, t, sl in zip(got, tensors, index):
                assert g.is_contiguous() and g.shape == t.shape
                _equal_in_slices(g, arr[sl], per_arr, f"{p.name}: array_to_coeffs against the slice of arr")
                _equal_in_slices(g, t, per_arr, f"{p.name}: array_to_coeffs against the band")
            arr = back = got = None
            torch.cuda.empty_cache()
            # ---- ravel_coeffs: kernel 59, the bands in sorted key order
            (flat, rsl, shapes), ids = _pack_events(lambda: ptwt_amd.ravel_coeffs(coeffs))
            assert ids == [59] and tuple(flat.shape) == (batch, per_flat) and flat.numel() > MARK[p.dtype]
            assert all(list(sl) == sorted(sl) for sl in rsl[1:])
            ordered = [approx] + [lv[k] for lv, sl in zip(levels, rsl[1:]) for k in sl]
            for s, e in L.batch_slices(batch, per_flat):
                ref = torch.cat([t[s:e].reshape(e - s, -1) for t in ordered], 1)
                assert torch.equal(flat[s:e], ref), f"{p.name}: ravel_coeffs, items {s} .. {e}"
                del ref
            # ---- unravel_coeffs(copy=True): kernel 60
            back, ids = _pack_events(lambda: ptwt_amd.unravel_coeffs(flat, rsl, shapes, p.fmt, copy=True))
            assert ids == [60]
            got = [back[0]] + [_entry(e)[k] for e, sl in zip(back[1:], rsl[1:]) for k in sl]
            for g, t in zip(got, ordered):
                assert g.is_contiguous() and g.shape == t.shape
                _equal_in_slices(g, t, per_flat, f"{p.name}: unravel_coeffs")
        _record(p.name, 0.0)
        print(f"{p.name}: batch {batch}, arr {per_arr} and flat {per_flat} elements an item ({gaps} of padding), peak "
              f"{torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    finally:
        bufs = arr = flat = back = got = coeffs = approx = levels = tensors = ordered = None
        torch.cuda.empty_cache()


@pytest.mark.parametrize("p", PACK, ids=lambda p: p.name.replace(" ", "-"))
def test_pack_cell(p):
    run_pack(p)


# ---- regime HUGE -------------------------------------------------------------------------------------------------------------------
INSIDE = 46340  # 46340^2 = 2 147 395 600 < 2^31 <= 46341^2 = 2 147 488 281
PITCH = 46344
#: test -> (the families it covers, the kernel ids it asserts)
HUGE = {
    "test_huge_image_inside": (("estimate_sigma", "keep_threshold", "sparse_encode"), {51, 55, 57}),
    "test_huge_image_past": (("estimate_sigma", "keep_threshold", "sparsify", "sparse_encode"), set()),
    "test_huge_row": (("estimate_sigma", "keep_threshold"), {51, 55}),
    "test_huge_pack": (("coeffs_to_array", "array_to_coeffs"), {59, 60}),
    "test_pack_rows_past_the_guard_are_composed": (("coeffs_to_array",), set()),
}


def _need(gib, what):
    free = torch.cuda.mem_get_info()[0]
    if free < gib << 30:
        pytest.skip(f"{what}: {gib} GiB needed, {free / 2 ** 30:.1f} GiB free")
    torch.cuda.reset_peak_memory_stats()


def _ids(fn):
    """(result, the set of kernel ids of the call)."""
    _engine.level_events = []
    try:
        out = fn()
        return out, {e[1] for e in _engine.level_events}
    finally:
        _engine.level_events = None


def _check_counts(x, v, k, what):
    ok, greater, equal = L.is_kth_largest([x], v, k)
    assert ok, f"{what}: {float(v)!r} is not the {k}-th largest magnitude: {greater} greater, {equal} equal"
    return greater, equal


def _check_sigma_by_counts(x, lead, kid, what):
    """``estimate_sigma`` of ONE image ``x``: its two order statistics by counts, sigma within an ulp of their float64 mean / 0.6745."""
    count = x.numel()
    stats, ids = _ids(lambda: E._order_stats(x, lead))
    sigma, ids2 = _ids(lambda: ptwt_amd.estimate_sigma(x, lead=lead))
    assert ids == ids2 == {kid}, (what, ids, ids2)
    lo, hi = stats.reshape(2).cpu()
    k_lo, k_hi = L.median_ranks(count)
    _check_counts(x, lo, k_lo, f"{what}: the order statistic of rank (c - 1) // 2")
    _check_counts(x, hi, k_hi, f"{what}: the order statistic of rank c // 2")
    want = np.array([(float(lo) + float(hi)) * 0.5 / RE.MAD_SCALE])
    TGE.within_ulp(sigma.reshape(1).cpu().numpy(), want, f"{what}: sigma")
    return sigma


@pytest.mark.parametrize("layout", ["dense", "pitched"])
def test_huge_image_inside(layout):
    """One image of 46340 x 46340 float32, the last square below 2^31 elements (module docstring).  9 GiB and the counting chunks."""
    _need(24, "46340 x 46340")
    n, count = INSIDE, INSIDE * INSIDE
    x = s = None
    try:
        gen = torch.Generator(device=DEV).manual_seed(31)
        x = _fill((n, n), f32, gen) if layout == "dense" else _fill((n, PITCH), f32, gen)[:, :n]
        assert x.is_contiguous() == (layout == "dense") and (layout == "dense" or (n - 1) * x.stride(0) + n > 1 << 31)
        _check_sigma_by_counts(x, 0, 51, layout)
        values = {}
        for k in (1, 1000, count // 2, count - 1):
            v, ids = _ids(lambda: ptwt_amd.keep_threshold(x, k))
            assert ids == {55} and v.shape == () and v.dtype == f32
            values[k] = (v.cpu(), *_check_counts(x, v.cpu(), k, f"{layout}: keep_threshold k = {k}"))
        s, ids = _ids(lambda: ptwt_amd.sparse_encode(x, 1000))
        assert ids == {55, 57} and tuple(s.values.shape) == (1000,) and s.indices.dtype == torch.int32 and int(s.counts) == 1000
        idx = s.indices.long()
        assert bool((idx[1:] > idx[:-1]).all()) and int(idx[0]) >= 0 and int(idx[-1]) < count  # ascending, unique, inside
        picked = x[idx // n, idx % n]  # (``x.flatten()[indices]`` without a dense copy of a pitched image)
        assert torch.equal(s.values, picked)
        v, greater, equal = values[1000]
        mags = s.values.abs().cpu()
        assert bool((mags >= v).all()) and int((mags > v).sum()) == greater and int((mags == v).sum()) == 1000 - greater
        _record(f"HUGE 46340^2 {layout}", 0.0)
        print(f"46340 x 46340 {layout}: peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    finally:
        x = s = None
        torch.cuda.empty_cache()


def test_huge_image_past():
    """One image of 46341 x 46341 float32, 2 147 488 281 elements, past the limit: no kernel of ids 50 .. 58 launches; every call
    raises a ``ValueError`` that names the limit (the composition the selection took here was a ``torch.sort``, which takes at most
    2^31 - 1 elements: module docstring).  9 GiB, 43 GiB while the composed moments run."""
    _need(56, "46341 x 46341")
    n = INSIDE + 1
    x = None
    try:
        x = _fill((n, n), f32, torch.Generator(device=DEV).manual_seed(32))
        assert x.numel() >= 1 << 31
        calls = {"estimate_sigma": lambda: ptwt_amd.estimate_sigma(x), "keep_threshold": lambda: ptwt_amd.keep_threshold(x, 1000),
                 "sparsify": lambda: ptwt_amd.sparsify(x, 1000), "sparse_encode": lambda: ptwt_amd.sparse_encode(x, 1000)}
        for name, fn in calls.items():
            _engine.level_events = []
            try:
                with pytest.raises(ValueError, match=r"fewer than 2\^31 .* got 2147488281"):
                    fn()
                assert _engine.level_events == [], (name, _engine.level_events)
            finally:
                _engine.level_events = None
        # its moments need no sort: the composition serves them
        coeffs = [torch.zeros((1, 1), dtype=f32, device=DEV), x.reshape(1, n * n)]
        thr, ids = _ids(lambda: ptwt_amd.estimate_thresholds(coeffs, "bayes", sigma=0.5))
        assert ids == set() and thr[1].shape == (1,)
        m2 = float(x.double().pow_(2).sum()) / (n * n)
        want = 0.25 / math.sqrt(m2 - 0.25)
        tol = 4 * float(torch.finfo(f32).eps) + 2 * (m2 / abs(m2 - 0.25)) * n * n * TGE.U  # (``threshold_tolerance`` of tests/test_gpu_estimators.py)
        assert abs(float(thr[1]) - want) <= tol * want
    finally:
        x = None
        torch.cuda.empty_cache()


def test_huge_row():
    """One dense row of 2^30 + 4096 float32 elements, [1, n]: ``band_geometry`` refuses ``n > 2^30``, ``thresholding._geometry`` cuts
    the row into two of 2^29 + 2048.  Kernels 51 / 55, by counts.  4 GiB."""
    _need(8, "a row of 2^30 + 4096")
    n = (1 << 30) + 4096
    x = None
    try:
        x = _fill((1, n), f32, torch.Generator(device=DEV).manual_seed(33))
        sigma = _check_sigma_by_counts(x, 1, 51, "row")
        assert tuple(sigma.shape) == (1,)
        for k in (1, n // 2, n - 1):
            v, ids = _ids(lambda: ptwt_amd.keep_threshold(x, k, lead=1))
            assert ids == {55} and tuple(v.shape) == (1,)
            _check_counts(x, v.cpu(), k, f"row: keep_threshold k = {k}")
        _record("HUGE row of 2^30 + 4096", 0.0)
    finally:
        x = None
        torch.cuda.empty_cache()


def test_huge_pack():
    """The haar level-1 ``wavedec2`` container of a 46342 x 46350 float32 image (four random bands of 23171 x 23175): ``coeffs_to_array``
    (59) and ``array_to_coeffs(copy=True)`` (60), both ``torch.equal`` to slice assignment; row x pitch of ``arr`` crosses 2^31.  26 GiB."""
    _need(30, "46342 x 46350")
    h, w = 23171, 23175
    bands = arr = back = None
    try:
        gen = torch.Generator(device=DEV).manual_seed(34)
        bands = [_fill((h, w), f32, gen) for _ in range(4)]
        coeffs = (bands[0], WaveletDetailTuple2d(*bands[1:]))
        (arr, slices), ids = _ids(lambda: ptwt_amd.coeffs_to_array(coeffs, PAD))
        assert ids == {59} and tuple(arr.shape) == (2 * h, 2 * w) and arr.numel() > 1 << 31
        where = {"a": (slice(0, h), slice(0, w)), "da": (slice(h, 2 * h), slice(0, w)), "ad": (slice(0, h), slice(w, 2 * w)),
                 "dd": (slice(h, 2 * h), slice(w, 2 * w))}
        assert slices == [where["a"], {k: where[k] for k in ("da", "ad", "dd")}]
        for key, t in zip(("a", "da", "ad", "dd"), bands):
            assert torch.equal(arr[where[key]], t), f"coeffs_to_array: block {key}"
        back, ids = _ids(lambda: ptwt_amd.array_to_coeffs(arr, slices, "wavedec2", copy=True))
        assert ids == {60}
        for key, g, t in zip(("a", "da", "ad", "dd"), [back[0], *back[1]], bands):
            assert g.is_contiguous() and torch.equal(g, t), f"array_to_coeffs: band {key}"
        _record("HUGE pack 46342 x 46350", 0.0)
        print(f"46342 x 46350 packed: peak {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")
    finally:
        bands = arr = back = coeffs = None
        torch.cuda.empty_cache()


def test_pack_rows_past_the_guard_are_composed():
    """The far side of the row guard: a 1-D float16 container whose leading extents 8 x (2^28 + 1) give 2^31 + 8 rows of 2 samples.
    ``mifwt_pack_plan`` answers negative: the call takes the composition, no 59 launch, bit-equal to slice assignment.  34 GiB."""
    _need(40, "2^31 + 8 rows of 2")
    lead = (8, (1 << 28) + 1)
    a = d = arr = None
    try:
        gen = torch.Generator(device=DEV).manual_seed(35)
        a, d = _fill((*lead, 2), f16, gen), _fill((*lead, 2), f16, gen)
        assert lead[0] * lead[1] == (1 << 31) + 8
        with _forced(C, "COMPOSED_CELLS", set())():
            (arr, slices), ids = _ids(lambda: ptwt_amd.coeffs_to_array([a, d], None))
        assert ids == set() and tuple(arr.shape) == (*lead, 4) and arr.dtype == f16
        for i in range(lead[0]):
            assert torch.equal(arr[i, :, 0:2], a[i]) and torch.equal(arr[i, :, 2:4], d[i]), f"composed coeffs_to_array, leading index {i}"
    finally:
        a = d = arr = None
        torch.cuda.empty_cache()


def test_the_tables_cover_what_they_claim():
    many = set().union(*[c.kids for c in POST]) | ({59, 60} if PACK else set())
    assert set(range(50, 61)) <= many, sorted(set(range(50, 61)) - many)
    for dtype in (f32, f64):  # both selection routes in both types
        for kid in (50, 51, 54):
            assert any(kid in c.kids and c.dtype == dtype for c in POST), (kid, dtype)
    assert {p.dtype for p in PACK} == {f32, f16, c128} and {p.fmt for p in PACK} == {"wavedec2", "wavedecn"}
    assert sum("8 magnitudes" in c.name for c in POST) == 3 and any("strided band" in c.name for c in POST)
    assert sum("n - 3" in c.name for c in POST) == 2 and sum("n / 64" in c.name for c in POST) == 3
    families = {f for fams, _ in HUGE.values() for f in fams}
    assert families == {"estimate_sigma", "keep_threshold", "sparsify", "sparse_encode", "coeffs_to_array", "array_to_coeffs"}
    assert set().union(*[kids for _, kids in HUGE.values()]) == {51, 55, 57, 59, 60}
    assert all(callable(globals()[name]) for name in HUGE)
    mine = {name: WORST[name] for name in WORST if any(name.startswith(c.name) for c in POST) or name.startswith(("HUGE", "59/60"))}
    print("worst error / bound of this run:", {k: round(v, 4) for k, v in mine.items() if v})
    print("recorded on an MI355X:", WORST_ON_MI355X)
