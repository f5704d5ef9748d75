"""threshold / threshold_firm without a GPU: the reference's closed forms against PyWavelets' documented numbers and the edge cases, every
argument error of the two functions, the C ABI's declarations, exports and refusals, and the CPU model of the kernels' map from
workgroup iterations to elements."""
import ctypes
import os
import re

import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, thresholding as T
from tests import _thresh_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X7 = torch.linspace(1, 4, 7, dtype=torch.float64)


# ---- the reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,want", [
    ("soft", [0, 0, 0, 0.5, 1, 1.5, 2]),
    ("hard", [0, 0, 2, 2.5, 3, 3.5, 4]),
    ("garrote", [0, 0, 0, 0.9, 1.66666667, 2.35714286, 3]),
    ("greater", [0, 0, 2, 2.5, 3, 3.5, 4]),
    ("less", [1, 1.5, 2, 0, 0, 0, 0]),
])
def test_reference_reproduces_the_pywavelets_documentation(mode, want):
    got = R.threshold(X7, 2, mode)
    assert torch.allclose(got, torch.tensor(want, dtype=torch.float64), atol=5e-9, rtol=0)
    # ... and so does the package's composed route, which shares no code with the reference
    got = T._composed(X7, 2.0, None, T.MODES[mode], 0.0)
    assert torch.allclose(got, torch.tensor(want, dtype=torch.float64), atol=5e-9, rtol=0)


def test_reference_firm_reproduces_the_pywavelets_documentation():
    want = torch.tensor([0, 0, 0, 1.5, 3, 3.5, 4], dtype=torch.float64)
    assert torch.allclose(R.threshold_firm(X7, 2, 3), want, atol=1e-12, rtol=0)
    assert torch.allclose(T._composed(X7, 2.0, 3.0, T.FIRM, 0.0), want, atol=1e-12, rtol=0)


@pytest.mark.parametrize("fn", [R.threshold, lambda x, v, mode="soft", substitute=0.0: T._composed(x, float(v), None, T.MODES[mode], substitute)],
                         ids=["reference", "composed"])
def test_edge_cases(fn):
    x = torch.tensor([-3.0, -1.0, 0.0, 0.5, 1.0, 2.0], dtype=torch.float64)
    for mode in ("soft", "garrote", "hard"):
        assert fn(x, 1.0, mode)[2] == 0  # x = 0 gives 0
        assert torch.equal(fn(x, 0.0, mode), x)  # v = 0 is the identity, with no NaN at x = 0
    # the substitute: where m < v (soft / garrote: ties give 0), where the element is not kept (hard / greater / less)
    assert fn(x, 1.0, "soft", 7.0).tolist() == [-2.0, 0.0, 7.0, 7.0, 0.0, 1.0]
    assert fn(x, 1.0, "garrote", 7.0).tolist() == [-3.0 * (1 - 1 / 9), 0.0, 7.0, 7.0, 0.0, 1.5]
    assert fn(x, 1.0, "hard", 7.0).tolist() == [-3.0, -1.0, 7.0, 7.0, 1.0, 2.0]
    assert fn(x, 1.0, "greater", 7.0).tolist() == [7.0, 7.0, 7.0, 7.0, 1.0, 2.0]
    assert fn(x, 1.0, "less", 7.0).tolist() == [-3.0, -1.0, 0.0, 0.5, 1.0, 7.0]


@pytest.mark.parametrize("firm", [R.threshold_firm, lambda x, lo, hi: T._composed(x, float(lo), float(hi), T.FIRM, 0.0)], ids=["reference", "composed"])
def test_firm_edge_cases(firm):
    x = torch.tensor([-3.0, -1.0, 0.0, 0.5, 1.0, 2.0], dtype=torch.float64)
    # v_hi == v_lo: hard thresholding there with substitute 0 (a tie is not kept), nothing divided
    assert firm(x, 1.0, 1.0).tolist() == [-3.0, 0.0, 0.0, 0.0, 0.0, 2.0]
    # continuity at both knees
    lo, hi, h = 1.0, 2.5, 1e-9
    near = torch.tensor([lo - h, lo, lo + h, hi - h, hi, hi + h], dtype=torch.float64)
    got = firm(near, lo, hi)
    assert torch.allclose(got[:3], torch.zeros(3, dtype=torch.float64), atol=1e-8)
    assert torch.allclose(got[3:], torch.full((3,), hi, dtype=torch.float64), atol=1e-8)
    assert torch.equal(firm(-near, lo, hi), -got)


def test_complex_data_uses_the_magnitude():
    z = torch.tensor([3 + 4j, 0.3 - 0.4j, 0j, -6 + 8j], dtype=torch.complex128)
    for fn in (R.threshold, lambda x, v, mode: T._composed(x, float(v), None, T.MODES[mode], 0.0)):
        assert torch.allclose(fn(z, 2.5, "soft"), torch.tensor([1.5 + 2j, 0j, 0j, -4.5 + 6j], dtype=torch.complex128))
        assert torch.equal(fn(z, 5.0, "hard"), torch.tensor([3 + 4j, 0j, 0j, -6 + 8j], dtype=torch.complex128))
        assert torch.allclose(fn(z, 5.0, "garrote"), torch.tensor([0j, 0j, 0j, 0.75 * (-6 + 8j)], dtype=torch.complex128))
    for fn in (R.threshold_firm, lambda x, lo, hi: T._composed(x, float(lo), float(hi), T.FIRM, 0.0)):
        assert torch.allclose(fn(z, 2.5, 7.5), torch.tensor([0.75 * (3 + 4j), 0j, 0j, -6 + 8j], dtype=torch.complex128))


def test_reference_maps_containers_and_leading_form_thresholds():
    a, b = torch.arange(6.0).reshape(2, 3), torch.arange(12.0).reshape(2, 2, 3)
    data = (a, ptwt_amd.WaveletDetailTuple2d(b, b + 1, b + 2), {"ad": b, "da": -b})
    out = R.threshold(data, [None, 2.0, torch.tensor([1.0, 100.0])], "hard")
    assert out[0] is a and type(out[1]) is ptwt_amd.WaveletDetailTuple2d and list(out[2]) == ["ad", "da"]
    assert torch.equal(out[1].vertical, torch.where(b + 1 >= 2, b + 1, torch.zeros(())))
    assert torch.equal(out[2]["ad"][0], torch.where(b[0] >= 1, b[0], torch.zeros(()))) and not out[2]["ad"][1].any()


# ---- argument errors (CPU tensors: every check but the device's comes first) -------------------------------------------------------
def test_argument_errors():
    x = torch.zeros(2, 8)
    cont = [x, x, x]
    with pytest.raises(ValueError, match="unknown mode 'semisoft'"):
        ptwt_amd.threshold(x, 1.0, "semisoft")
    with pytest.raises(ValueError, match="value must be non-negative, got -1.0"):
        ptwt_amd.threshold(x, -1.0)
    with pytest.raises(ValueError, match="value_low must be non-negative"):
        ptwt_amd.threshold_firm(x, -1.0, 2.0)
    with pytest.raises(ValueError, match="value_high must not be below value_low, got 1.0 < 2.0"):
        ptwt_amd.threshold_firm(x, 2.0, 1.0)
    with pytest.raises(ValueError, match=r"\(3,\) is no leading part of \(2, 8\)"):
        ptwt_amd.threshold(x, torch.ones(3))
    with pytest.raises(ValueError, match="is no leading part"):
        ptwt_amd.threshold(x, torch.ones(2, 8))  # (the whole shape is no LEADING form)
    with pytest.raises(ValueError, match="one entry per container entry: 2 for 3"):
        ptwt_amd.threshold(cont, [1.0, 2.0])
    with pytest.raises(ValueError, match="one entry per container entry"):
        ptwt_amd.threshold_firm(cont, [1.0, 2.0, 3.0], [1.0, 2.0])
    with pytest.raises(ValueError, match="None for the same container entries"):
        ptwt_amd.threshold_firm(cont, [None, 2.0, 3.0], [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="must be a number or a tensor"):
        ptwt_amd.threshold(x, "1")
    with pytest.raises(ValueError, match="real data only"):
        ptwt_amd.threshold(torch.zeros(4, dtype=torch.complex64), 1.0, "greater")
    with pytest.raises(ValueError, match="real data only"):
        ptwt_amd.threshold(torch.zeros(4, dtype=torch.complex128), 1.0, "less")
    for dtype in (torch.float16, torch.bfloat16, torch.int32):
        with pytest.raises(ValueError, match="Input dtype .* not supported"):
            ptwt_amd.threshold(x.to(dtype), 1.0)
    for call in (lambda: ptwt_amd.threshold(x, 1.0), lambda: ptwt_amd.threshold_firm(cont, 1.0, 2.0),
                 lambda: ptwt_amd.threshold(cont, [None, 1.0, torch.ones(2)], "garrote")):
        with pytest.raises(RuntimeError, match="expected a tensor on a ROCm device, got device 'cpu'"):
            call()
    with ptwt_amd.half_storage():  # (inside the scope the 16-bit types pass the dtype check and reach the device's)
        with pytest.raises(RuntimeError, match="ROCm device"):
            ptwt_amd.threshold(x.to(torch.bfloat16), 1.0)


def test_public_names():
    assert "threshold" in ptwt_amd.__all__ and "threshold_firm" in ptwt_amd.__all__
    assert ptwt_amd.threshold is T.threshold and ptwt_amd.threshold_firm is T.threshold_firm
    assert T._plans in _engine._routing_caches


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_header_and_library_export_the_symbols():
    with open(os.path.join(ROOT, "include", "mifwt.h")) as f:
        header = f.read()
    lib = _engine.load_library()
    for sym in ("mifwt_thresh_fwd", "mifwt_thresh_bwd", "mifwt_thresh_max_segments"):
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert getattr(lib, sym) is not None
    for name, kid in (("MIFWT_KID_THRESH_FWD", 48), ("MIFWT_KID_THRESH_BWD", 49)):
        assert re.search(r"#define %s %d\b" % (name, kid), header)
    assert re.search(r"^ \*   48 / 49  thresholding", header, flags=re.M)  # (the id table)
    assert lib.mifwt_abi_version() == 3 and "#define MIFWT_ABI_VERSION 3" in header
    assert (T.KID_FWD, T.KID_BWD) == (48, 49)
    assert T.max_segments() >= 24


def _segs(n=1, extent=(1, 1, 8), last=1):
    arr = (T.Seg * n)()
    for s in arr:
        s.x = s.y = s.g = 4096  # (never dereferenced: every call below is refused on the host)
        s.extent[:] = extent
        s.x_stride[:] = s.y_stride[:] = s.g_stride[:] = (0, 0, last)
    return arr


def test_refusals_launch_nothing():
    lib = T._lib()
    before = (_engine.launch_count(48), _engine.launch_count(49))
    cap = T.max_segments()
    bad, unsupported = -1, -2
    assert lib.mifwt_thresh_fwd(0, 0, 0, 0.0, _segs(), 0, None) == bad  # nseg out of range
    assert lib.mifwt_thresh_fwd(0, 0, 0, 0.0, _segs(cap + 1), cap + 1, None) == bad
    assert lib.mifwt_thresh_bwd(0, 0, _segs(cap + 1), cap + 1, None, 0, None) == bad
    assert lib.mifwt_thresh_fwd(0, 0, 6, 0.0, _segs(), 1, None) == bad  # unknown mode
    assert lib.mifwt_thresh_fwd(0, 0, -1, 0.0, _segs(), 1, None) == bad
    assert lib.mifwt_thresh_bwd(1, 9, _segs(), 1, None, 0, None) == bad
    assert lib.mifwt_thresh_fwd(0, 0, 0, 0.0, _segs(last=2), 1, None) == bad  # a non-unit innermost stride
    assert lib.mifwt_thresh_bwd(0, 0, _segs(last=2), 1, None, 0, None) == bad
    assert lib.mifwt_thresh_fwd(7, 0, 0, 0.0, _segs(), 1, None) == bad  # unknown dtype
    for dt in (0, 1):
        assert lib.mifwt_thresh_fwd(dt, 1, 3, 0.0, _segs(), 1, None) == unsupported  # greater / less on complex data
        assert lib.mifwt_thresh_fwd(dt, 1, 4, 0.0, _segs(), 1, None) == unsupported
    assert lib.mifwt_thresh_plan(0, 0, _segs(last=2), 1, None) == bad
    assert (_engine.launch_count(48), _engine.launch_count(49)) == before


# ---- the map from units to elements -------------------------------------------------------------------------------------------------
SIZES = [64, 0, 4099, 1, 65, 3, 63, 5, 4]  # mixed order


@pytest.mark.parametrize("dt,is_complex,vec", [(0, 0, 4), (1, 0, 2), (2, 0, 8), (0, 1, 2), (1, 1, 1)], ids=["f32", "f64", "f16", "c64", "c128"])
def test_every_element_is_visited_exactly_once(dt, is_complex, vec):
    """The prefix table of the library against the model's unit counts, then the model's walk: every element of every segment exactly
    once, whatever the rows' misalignment, every unit inside its segment and inside one threshold group."""
    shapes = [(1, 1, n) for n in SIZES] + [(3, 5, n) for n in SIZES] + [(1, 4, 2 * 4099)]
    rows_per = [0] * len(SIZES) + [5 if n else 0 for n in SIZES] + [1]
    for c0 in range(0, len(shapes), T.max_segments()):
        part, rp = shapes[c0:c0 + T.max_segments()], rows_per[c0:c0 + T.max_segments()]
        arr = _segs(len(part))
        for s, ext, r in zip(arr, part, rp):
            s.extent[:] = ext
            s.x_stride[:] = s.y_stride[:] = (ext[1] * ext[2], ext[2], 1)
            if r:
                s.dvalue[0], s.rows_per_value[0] = 4096, r
        start = (ctypes.c_int64 * (len(part) + 1))()
        total = T._lib().mifwt_thresh_plan(dt, is_complex, arr, len(part), start)
        geos = [R.seg_geometry(e[0] * e[1], e[2], vec, r) for e, r in zip(part, rp)]
        assert [start[i + 1] - start[i] for i in range(len(part))] == [g["units"] for g in geos]
        assert total == start[len(part)] == sum(g["units"] for g in geos)
        for (e0, e1, n), r, g in zip(part, rp, geos):
            for mis in (lambda row: 0, lambda row: (row * 3 + 1) % vec):
                seen = torch.zeros(e0 * e1, max(n, 1), dtype=torch.int32)
                for u in range(g["units"]):
                    elems = R.unit_elements(g, u, mis)
                    assert elems and len({grp for _, _, grp in elems}) == 1
                    assert len(elems) <= R.UNIT_SLOTS * vec
                    for row, col, grp in elems:
                        assert 0 <= row < e0 * e1 and 0 <= col < n and grp == (row // r if r else 0)
                        seen[row, col] += 1
                assert n == 0 or bool((seen == 1).all())


def test_collapsed_forms():
    """Views as the descriptors express them: at most three extents, unit innermost stride, never merged across a threshold's axes."""
    c = T._collapse
    assert c((3, 7, 13), (364, 13, 1), []) == ([1, 3, 91], [0, 364, 1], [])  # buf[:, 1] of a [3, 4, 7, 13] buffer
    assert c((3, 7, 13), (91, 13, 1), []) == ([1, 1, 273], [0, 0, 1], [])
    assert c((3, 7, 13), (91, 13, 1), [1]) == ([1, 3, 91], [0, 91, 1], [1])  # one threshold per image: rows are images
    assert c((2, 3, 4, 5), (60, 20, 5, 1), [2]) == ([1, 6, 20], [0, 20, 1], [1])
    assert c((2, 3, 4, 6), (96, 32, 8, 1), [1]) == ([2, 12, 6], [96, 8, 1], [12])  # padded rows: twelve rows per image
    assert c((2, 3, 4, 6), (96, 32, 8, 1), [1, 2]) is None  # four extents: read from a copy
    assert c((3, 1), (1, 1), [1]) == ([1, 3, 1], [0, 1, 1], [1])  # a last axis of one element stays the row
    assert c((4, 6), (1, 4), []) is None  # a transposed view has no unit innermost stride: read from a copy
    assert c((), (), []) == ([1, 1, 1], [0, 0, 1], [])


def test_rows_beyond_the_kernel_limit_are_cut_back():
    """A dense tensor of more than 2^30 elements (geometry only, no memory): the merged row is cut into the fewest equal rows the
    kernels take, the descriptor table of the cut is accepted by the library, a per-image threshold keeps its rows; a length without
    such a cut is left as it is and reported as outside the envelope (the composed route)."""
    c, lim = T._collapse, T.ROW_LIMIT
    b = 131073  # 131073 x 128 x 128 = 2^31 + 2^14 elements; 131073 = 3 x 43691
    n = b * 128 * 128
    assert T._split_row(n) == (3, 43691 * 16384) and T._split_row(lim + 2) == (2, lim // 2 + 1)
    assert T._split_row((1 << 31) - 1) is None  # a prime
    assert T._split_row(3 * 1073741827) is None  # 3 x a prime above 2^30: the first divisor from 4 on is that prime
    assert c((b, 128, 128), (16384, 128, 1), []) == ([1, 3, 43691 * 16384], [0, 43691 * 16384, 1], [])
    assert c((b, 128, 128), (16384, 128, 1), [1]) == ([1, b, 16384], [0, 16384, 1], [1])
    assert c((2, lim + 2), (lim + 2, 1), [1]) == ([2, 2, lim // 2 + 1], [lim + 2, lim // 2 + 1, 1], [2])  # two cut rows per threshold index
    assert c((lim,), (1,), []) == ([1, 1, lim], [0, 0, 1], [])  # the limit itself is a row
    assert c(((1 << 31) - 1,), (1,), []) == ([1, 1, (1 << 31) - 1], [0, 0, 1], [])
    meta = torch.empty((b, 128, 128), device="meta")
    assert T._kernel_takes(meta, (0, 0)) and T._kernel_takes(meta, (1, 0))
    assert not T._kernel_takes(torch.empty(((1 << 31) - 1,), device="meta"), (0, 0))
    assert T._kernel_takes(torch.empty((lim,), device="meta"), (0, 0))
    for ext, want in (((1, 3, 43691 * 16384), R.seg_geometry(3, 43691 * 16384, 4)["units"]), ((1, 1, n), -2)):  # (-2: unsupported)
        arr = _segs()
        arr[0].extent[:] = ext
        arr[0].x_stride[:] = arr[0].y_stride[:] = (ext[1] * ext[2], ext[2], 1)
        assert T._lib().mifwt_thresh_plan(0, 0, arr, 1, None) == want, ext


def test_flattening_a_container_leaves_no_reference_cycle_around_its_tensors():
    """``_flatten`` used to walk the container with a nested function that called itself — a reference cycle that also held the list of
    leaves, so every input tensor of a ``threshold`` call stayed alive until the cyclic collector ran (8 GiB of device memory after a
    call on a large batch).  With the collector off, dropping the last references must free the tensors at once."""
    import gc
    import weakref

    gc.collect()
    gc.disable()
    try:
        a, b = torch.zeros(3), torch.zeros(2, 2)
        refs = [weakref.ref(a), weakref.ref(b)]
        leaves, owner, n = T._flatten([a, (b, {"k": a})])
        assert [t.shape for t in leaves] == [a.shape, b.shape, a.shape] and owner == [0, 1, 1] and n == 2
        del leaves, a, b
        assert all(r() is None for r in refs)
    finally:
        gc.enable()
