"""CPU tests of tests/_large_ref.py: the sample set and the batch slices of tests/test_gpu_large_offsets.py."""
import numpy as np
import pytest
import torch

from oracle import torch_autograd_ref as A
from ptwt_amd._wavelets import host_taps
from tests import _large_ref as L


def test_crossing_items_by_hand():
    # float32 planes of 128 x 128: byte offset 2^31 is element 2^29 = item 32768, byte 2^32 = element 2^30 = item 65536, element 2^31
    # = item 131072; element 2^32 is not reached by 131075 items
    assert L.crossing_items(131075, 16384, 4) == [32768, 65536, 131072]
    # float64: byte marks at elements 2^28 and 2^29; a batch that ends behind 2^29 elements reaches no element mark
    assert L.crossing_items(32771, 16384, 8) == [16384, 32768]
    # float16, 2^32 elements: byte marks at elements 2^30 and 2^31 — the second coincides with the element mark 2^31 (once)
    assert L.crossing_items(262147, 16384, 2) == [65536, 131072, 262144]
    # a mark inside an item, not at its first element
    assert L.crossing_items(10 ** 9, 1000, 4) == [(1 << 29) // 1000, (1 << 30) // 1000, (1 << 31) // 1000, (1 << 32) // 1000]
    assert L.crossing_items(5, 16, 4) == []


def test_sample_items():
    b = L.batch_over(1 << 31, [16384, 4 * 67 * 67])
    assert b * 16384 > 1 << 31 and (b - 3) * 16384 <= 1 << 31
    buffers = [(16384, 4), (4 * 67 * 67, 4)]
    items = L.sample_items(b, buffers, seed=3)
    assert items == sorted(set(items)) and items[0] == 0 and items[-1] == b - 1 and {1, b - 2} <= set(items)
    assert all(0 <= i < b for i in items) and len(items) <= 4 + 3 * 3 * len(buffers) + 8
    for stride, esz in buffers:
        for mark in (1 << 31, 1 << 32):
            for first in (mark // esz, mark):
                item = first // stride
                if item < b:  # the item that holds the mark, and a neighbour on either side
                    assert item * stride <= first < (item + 1) * stride
                    assert {item - 1, item, item + 1} <= set(items), (stride, first)
    assert (1 << 31) // 16384 in items and (1 << 31) // (4 * 67 * 67) in items
    assert L.sample_items(b, buffers, seed=3) == items  # a fixed seed
    assert len(set(L.sample_items(b, buffers, seed=4)) - set(items)) > 0
    fixed = L.sample_items(b, buffers, nrandom=0)
    assert set(fixed) < set(items) and len(items) - len(fixed) <= 8
    assert L.sample_items(3, [(10, 4)]) == [0, 1, 2]  # a tiny batch: every item once


def test_batch_slices_cover_the_batch_once():
    for batch, item in ((131075, 16384), (7, 1 << 28), (5, (1 << 28) + 1), (1000, 3)):
        sl = L.batch_slices(batch, item)
        assert sl[0][0] == 0 and sl[-1][1] == batch and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        assert all(0 < e - s and ((e - s) * item <= L.SLICE_ELEMENTS or e - s == 1) for s, e in sl)
        sizes = [e - s for s, e in sl]
        assert max(sizes) - min(sizes) <= 1 and len(sl) == -(-batch // max(1, L.SLICE_ELEMENTS // item))  # equal slices, as few as fit


@pytest.mark.parametrize("mode", ["zero", "constant", "reflect", "periodic", "symmetric"])
@pytest.mark.parametrize("shape", [(3, 37), (2, 40), (2, 13, 18), (3, 16, 11)])
def test_level_maps_match_the_autograd_reference_in_values_and_tap_gradients(shape, mode):
    """``analysis_level`` and ``synthesis_level_adjoint`` against oracle/torch_autograd_ref.py: the bands, and the gradients of
    ``<cotangents, level>`` w.r.t. all four filters of a random bank of six taps (four independent filters)."""
    g = torch.Generator().manual_seed(sum(shape))
    nd, flen = len(shape) - 1, 6
    dec, rec = (A.wavedec, A.waverec) if nd == 1 else (A.wavedec2, A.waverec2)
    x = torch.randn(*shape, generator=g, dtype=torch.float64)
    taps = [(torch.randn(flen, generator=g, dtype=torch.float64) / flen ** 0.5).requires_grad_(True) for _ in range(4)]
    want = dec(x, tuple(taps), mode=mode, level=1)
    want = [want[0], want[1]] if nd == 1 else [want[0], *want[1]]
    got = L.analysis_level(x, taps[0], taps[1], mode)
    cots = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in want]
    for a, b in zip(got, want):
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-12, atol=1e-13)
    want_g = torch.autograd.grad(want, taps[:2], cots)
    got_g = torch.autograd.grad(sum((c * t).sum() for c, t in zip(cots, got)), taps[:2])
    for a, b in zip(got_g, want_g):
        assert torch.allclose(a, b, rtol=1e-11, atol=1e-12)
    bands = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in want]
    y = rec([bands[0], bands[1]] if nd == 1 else [bands[0], tuple(bands[1:])], tuple(taps))
    g_y = torch.randn(y.shape, generator=g, dtype=torch.float64)
    adj = L.synthesis_level_adjoint(g_y, taps[2], taps[3])
    assert [t.shape for t in adj] == [t.shape for t in bands]
    pairing = sum((c * t).sum() for c, t in zip(bands, adj))
    assert torch.allclose(pairing, (g_y * y).sum(), rtol=1e-11)
    for a, b in zip(torch.autograd.grad(pairing, taps[2:]), torch.autograd.grad(y, taps[2:], g_y)):
        assert torch.allclose(a, b, rtol=1e-11, atol=1e-12)


def test_window_starts_by_hand():
    # an output of 23171 x 23175 coefficients whose rows are 23175 elements apart, computed from an input of 46341 x 46349 samples
    # (pitch 46349, two input rows per output row): corners, edge midpoints, centre, and the rows at which row x pitch crosses a mark
    got = L.window_starts((23171, 23175), [(23175, 1), (46349, 2)])
    rows, cols = sorted({r for r, _ in got}), sorted({c for _, c in got})
    assert cols == [0, (23175 - 96) // 2, 23175 - 96] and {0, (23171 - 96) // 2, 23171 - 96} <= set(rows)
    assert {(r, c) for r in (0, (23171 - 96) // 2, 23171 - 96) for c in cols} <= set(got)
    crossing = [(1 << 29) // 23175, (1 << 29) // 46349 // 2, (1 << 30) // 46349 // 2, (1 << 31) // 46349 // 2]
    assert (1 << 30) // 23175 >= 23171  # (the output buffer itself ends before 2^30 elements)
    for row in crossing:
        assert any(r <= row < r + 96 and c == cols[1] for r, c in got), row
    assert len(got) == 9 + 2  # (rows 23165 and 23166 lie in the bottom edge's middle window, which is there already)
    assert L.window_starts((5, 40), [(40, 1)]) == [(0, 0)]  # an output smaller than a window: the whole of it, once
    assert L.axis_starts(1000) == [0, 452, 904]


def _families():
    g = np.random.default_rng(5)
    bank8 = tuple(tuple(float(v) for v in g.standard_normal(8) / 8 ** 0.5) for _ in range(4))
    taps4 = tuple(tuple(float(v) for v in g.standard_normal(4) / 2) for _ in range(4))
    return {
        "padded 2-D": (L.padded_family("db4", "symmetric", 2), 8, False), "padded 2-D reflect": (L.padded_family("db2", "reflect", 2), 4, False),
        "padded 1-D": (L.padded_family("db4", "symmetric", 1), 8, False), "periodized": (L.per_family(bank8), 8, "per"),
        "smooth": (L.ext_family(host_taps("db4"), "smooth"), 8, "ext"), "complex": (L.cplx_family(host_taps("db4"), "symmetric"), 8, "cplx"),
        "boundary": (L.boundary_family(bank8, "symmetric", False), 8, "bwt"), "stationary": (L.swt2_family(taps4, 0.25), 4, "swt"),
    }


@pytest.mark.parametrize("name", ["padded 2-D", "padded 2-D reflect", "padded 1-D", "periodized", "smooth", "complex", "boundary", "stationary"])
def test_window_reference_equals_the_window_of_the_whole_reference(name):
    """Every window of :func:`window_starts` (and a few odd interior ones) of a plane of a few hundred samples, windows of 20: the
    family's reference on the gathered crop, cut to the window, against the same window of the family's reference on the whole plane —
    analysis and synthesis, odd extents where the family takes them (a crop at a true end keeps the plane's border handling, a crop
    inside never sees a border; circular families continue on the other side)."""
    fam, flen, kind = _families()[name]
    g = torch.Generator().manual_seed(len(name))
    even = kind in ("per", "swt")
    sig = ((151,), (150,)) if fam.ndim == 1 else ((148, 162), (130, 150)) if even else ((149, 161), (150, 131), (77, 160))
    for ext in sig:
        shape = (1, *ext)
        x = torch.randn(shape, generator=g, dtype=torch.float64)
        if kind == "cplx":
            x = torch.complex(x, torch.randn(shape, generator=g, dtype=torch.float64))
        whole = fam.fwd([x])
        coef = tuple(whole[0].shape[-fam.ndim:])
        starts = [(s,) for s in L.axis_starts(coef[0], 20)] + [(7,), (33,)] if fam.ndim == 1 else \
            L.window_starts(coef, [(coef[1], 1)], 20) + [(7, 9), (coef[0] - 31, 33)]
        for start in starts:
            got = L.window_reference(fam, True, lambda idx: [L.take(x, idx)], ext, coef, start, 20)
            for a, b in zip(got, whole):
                want = b[(Ellipsis, *[slice(s, s + 20) for s in start])]
                assert a.shape == want.shape and torch.allclose(a, want, rtol=1e-12, atol=1e-13), (name, ext, "analysis", start)
        bands = [torch.randn(t.shape, generator=g, dtype=torch.float64).to(t.dtype) for t in whole]
        if kind == "cplx":
            bands = [torch.complex(b.real, torch.randn(b.shape, generator=g, dtype=torch.float64)) for b in bands]
        if kind == "ext":
            bands = [torch.stack(bands, 1)]
        out_ext = ext if kind in ("ext", "bwt", "per", "swt") else tuple(2 * m - flen + 2 for m in coef)
        y = fam.inv(bands, list(out_ext))[0]
        assert tuple(y.shape[-fam.ndim:]) == tuple(out_ext)
        starts = [(s,) for s in L.axis_starts(out_ext[0], 20)] + [(11,)] if fam.ndim == 1 else \
            L.window_starts(out_ext, [(out_ext[1], 1)], 20) + [(11, 5), (out_ext[0] - 41, 37)]
        for start in starts:
            got = L.window_reference(fam, False, lambda idx: [L.take(b, idx) for b in bands], coef, out_ext, start, 20)[0]
            want = y[(Ellipsis, *[slice(s, s + 20) for s in start])]
            assert got.shape == want.shape and torch.allclose(got, want, rtol=1e-12, atol=1e-13), (name, ext, "synthesis", start)


def test_item_relerr():
    g = torch.Generator().manual_seed(0)
    want = torch.randn(5, 3, 4, generator=g)
    got = want.clone()
    got[2] += 1e-3 * torch.randn(3, 4, generator=g)
    got[4] = want[3]  # a misplaced item
    err = L.item_relerr(got, want)
    ref = torch.stack([(got[i].double() - want[i].double()).norm() / want[i].double().norm() for i in range(5)])
    assert err.dtype == torch.float64 and torch.allclose(err, ref, rtol=1e-6, atol=0)
    assert err[0] == 0 and err[1] == 0 and err[3] == 0 and 1e-4 < err[2] < 1e-2 and err[4] > 0.5
    c = torch.randn(2, 6, generator=g, dtype=torch.float64).to(torch.complex64).reshape(2, 6)
    assert L.item_relerr(c, c).tolist() == [0.0, 0.0]


# ---- the counting check of tests/test_gpu_large_offsets_post.py -------------------------------------------------------------------------
def _sorted_magnitudes(arrays):
    return np.sort(np.concatenate([np.abs(a).reshape(-1) for a in arrays]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_counting_check_against_a_sort_on_adversarial_pools(dtype):
    """``is_kth_largest`` says yes to ``numpy.sort(|x|)[n - k]`` and no to every other value, on the pools of tests/_sparsify_ref.py
    and tests/_estimator_ref.py (ties at the cut, -0.0, denormals, inf, bits that differ in the last digit), in chunks smaller than
    the pool, over several tensors, one of them a strided view."""
    from tests import _estimator_ref as RE
    from tests import _sparsify_ref as RS
    n = 301
    pools = {f"sparsify {k}": v[0] for k, v in RS.pools(dtype, 1, n, seed=4).items()}
    pools.update({f"estimator {k}": v for k, v in RE.adversarial(dtype, n, seed=5).items()})
    pools["tie free"] = RS.tie_free(dtype, 1, n, seed=6)[0]
    for name, values in pools.items():
        wide = torch.from_numpy(np.stack([values[100:], values[100:]], 1).copy())
        tensors = [torch.from_numpy(values[:100].copy()).reshape(4, 25), wide[:, 0]]  # (the second: stride 2)
        assert not tensors[1].is_contiguous()
        s = _sorted_magnitudes([values])
        distinct = np.unique(s)
        for k in (1, 2, 3, n // 2, (n + 1) // 2, n - 1, n):
            v = s[n - k]
            ok, greater, equal = L.is_kth_largest(tensors, v, k, chunk=64)
            assert ok and greater == int((s > v).sum()) and equal == int((s == v).sum()), (name, k)
            assert L.is_kth_largest(tensors, torch.tensor(v), k, chunk=7)[0], (name, k)  # a tensor value, another chunking
            for other in distinct[distinct != v][:: max(1, distinct.size // 5)]:  # another value of the pool is not the k-th largest
                assert not L.is_kth_largest(tensors, other, k, chunk=64)[0], (name, k, other)
            if np.isfinite(v) and v > 0:  # a value between two of the pool has the right counts and does not occur
                between = np.nextafter(v, dtype(0), dtype=dtype)
                if between not in distinct:
                    assert not L.is_kth_largest(tensors, between, k, chunk=64)[0], (name, k)
        assert L.is_kth_largest(tensors, np.inf, 0)[0]  # k = 0: +inf and nothing else
        assert s[-1] == np.inf or not L.is_kth_largest(tensors, s[-1], 0)[0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_counting_check_every_rank_of_a_small_pool(dtype):
    values = np.array([0.0, -0.0, 1.5, -1.5, 1.5, np.inf, -3.0, 2.0 ** -140 if dtype == np.float32 else 5e-324, 0.25, -0.25, 7.0], dtype=dtype)
    t = [torch.from_numpy(values)]
    s = _sorted_magnitudes([values])
    n = values.size
    for k in range(1, n + 1):
        for v in np.unique(s):
            assert L.is_kth_largest(t, v, k, chunk=3)[0] == bool(v == s[n - k]), (k, v)
    assert L.magnitude_counts(t, 0.0) == (9, 2) and L.magnitude_counts(t, -0.0) == (9, 2)  # -0.0 is 0.0
    assert L.magnitude_counts(t, 1.5) == (3, 3) and L.magnitude_counts(t, np.inf) == (0, 1)
    assert L.magnitude_keys(torch.from_numpy(values)).min() == 0


def test_median_through_the_counting_check():
    """``median_ranks``: the two order statistics whose mean is numpy's median (tests/_estimator_ref.py), odd and even counts."""
    from tests import _estimator_ref as RE
    assert L.median_ranks(1) == (1, 1) and L.median_ranks(2) == (2, 1) and L.median_ranks(5) == (3, 3) and L.median_ranks(6) == (4, 3)
    for count in (1, 2, 7, 64, 301):
        for name, x in RE.adversarial(np.float32, count, seed=count).items():
            lo, hi = RE.order_stats(x)
            k_lo, k_hi = L.median_ranks(count)
            t = [torch.from_numpy(x)]
            assert L.is_kth_largest(t, lo, k_lo, chunk=50)[0] and L.is_kth_largest(t, hi, k_hi, chunk=50)[0], (name, count)
            if np.isfinite(lo) and np.isfinite(hi):
                assert (np.float64(lo) + np.float64(hi)) * 0.5 / RE.MAD_SCALE == RE.estimate_sigma(x), (name, count)
