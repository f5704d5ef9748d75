"""sparse_encode / sparse_decode on the GPU (kernel ids 56 / 57 / 58, csrc/mifwt_compact.hip) against the numpy reference of
tests/_sparse_ref.py: per image a stable argsort of the negated magnitudes, the first k, sorted ascending, padded with 0 / -1.

Tolerance 0 everywhere: the compaction moves bits and computes nothing, so values are compared as bytes and indices and counts as
integers.  Both routes (default and ``FORCE_STREAM``), float32 and float64.  Every allocation a kernel writes is carved out of canary
bytes (tests/test_gpu_canaries.py)."""
import importlib

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, estimators as E, thresholding as T
from tests import _sparse_ref as R
from tests import _sparsify_ref as R0
from tests.test_gpu_canaries import _GuardedTorch

S = importlib.import_module("ptwt_amd.sparse")
SP = importlib.import_module("ptwt_amd.sparsify")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NP = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
ROUTES = pytest.mark.parametrize("route", ["default", "stream"])


@pytest.fixture()
def canaries(monkeypatch):
    g = _GuardedTorch()
    for mod in (S, SP, E, T, _engine):
        monkeypatch.setattr(mod, "torch", g)
    yield g
    g.check("sparse")


@pytest.fixture()
def events():
    _engine.level_events = []
    try:
        yield _engine.level_events
    finally:
        _engine.level_events = None


def force(monkeypatch, route):
    monkeypatch.setattr(S, "FORCE_STREAM", route == "stream")


def leaves(obj):
    if isinstance(obj, torch.Tensor):
        return [obj]
    if isinstance(obj, dict):
        return [t for v in obj.values() for t in leaves(v)]
    return [t for v in obj for t in leaves(v)]


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def pooled(coeffs, approx):
    return leaves(coeffs if approx or isinstance(coeffs, torch.Tensor) else coeffs[1:])


def fill(tensors, values):
    """Write the pool ``values`` [images, n] into ``tensors`` in place of their values, in pooling order."""
    off = 0
    for t in tensors:
        m = t.numel() // values.shape[0]
        if m:
            t.copy_(torch.from_numpy(values[:, off:off + m].copy()).reshape(t.shape))
        off += m
    assert off == values.shape[1]


def check(coeffs, keep, lead, approx=False, capacity=None, what="", decode=True):
    """sparse_encode bit-equal to the reference, the container back from sparse_decode bit-equal to the reference decode."""
    ts = pooled(coeffs, approx)
    tn = [t.detach().cpu().numpy() for t in ts]
    n = R.flat_pool(tn, lead).shape[1]
    k = keep.cpu().numpy() if isinstance(keep, torch.Tensor) else R0.k_of(keep, n)
    cap = capacity if capacity is not None else k
    want = R.encode(tn, lead, k, cap)
    s = ptwt_amd.sparse_encode(coeffs, keep, approx=approx, capacity=capacity)
    assert isinstance(s, ptwt_amd.SparseCoeffs) and s.layout.n == n and s.layout.capacity == cap
    assert s.values.dtype == ts[0].dtype and s.indices.dtype == torch.int32 and s.counts.dtype == torch.int32
    got = (s.values.cpu().numpy(), s.indices.cpu().numpy(), s.counts.cpu().numpy())
    assert same_bits(got[2], want[2]), (what, keep, got[2], want[2])
    assert same_bits(got[1], want[1]), (what, keep, got[1], want[1])
    assert same_bits(got[0], want[0]), (what, keep)
    if isinstance(coeffs, torch.Tensor) or approx:
        assert s.approx is None
    else:
        assert s.approx is coeffs[0]
    if decode:
        back = ptwt_amd.sparse_decode(s)
        assert type(back) is type(coeffs)
        outs = pooled(back, approx)
        if not (isinstance(coeffs, torch.Tensor) or approx):
            assert back[0] is coeffs[0]
        dense = R.decode(*want, [t.shape for t in tn], lead)
        assert len(outs) == len(dense)
        for o, d in zip(outs, dense):
            assert o.is_contiguous() and same_bits(o.cpu().numpy(), d), (what, keep)
    return s


def segmented(values, dtype):
    """The pool ``values`` [images, n] as a container [approximation, first third, rest]: two segments (the first one empty for n < 3)."""
    images, n = values.shape
    x = torch.from_numpy(values).to(DEV)
    cut = n // 3
    return [torch.ones(images, 2, dtype=dtype, device=DEV), x[:, :cut].contiguous(), x[:, cut:].contiguous()]


def all_pools(dtype, images, n, seed):
    out = dict(R.pools(NP[dtype], images, n, seed=seed))
    out["tie_free"] = R.tie_free(NP[dtype], images, n, seed=seed)
    return out


def ks_of(n):
    return sorted({0, 1, 2, n // 2, n - 1, n} & set(range(n + 1)))


# ---- pools, sizes, k -------------------------------------------------------------------------------------------------------------------
@DTYPES
@ROUTES
def test_adversarial_pools_sizes_and_k(dtype, route, monkeypatch, canaries, events):
    force(monkeypatch, route)
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 4097):
        for name, values in all_pools(dtype, 2, n, seed=n).items():
            coeffs = segmented(values, dtype)
            for k in ks_of(n):
                check(coeffs, k, 1, what=f"{name} n={n} {route}", decode=k in (2, n // 2))
    assert {e[1] for e in events if e[0] == "compact_encode"} == ({57} if route == "stream" else {56})
    assert {e[1] for e in events if e[0] == "select_kth"} == ({55} if route == "stream" else {54})
    assert {e[1] for e in events if e[0] == "compact_scatter"} == {58}


@DTYPES
def test_several_chunks_and_the_capacity_boundary(dtype, canaries, events):
    cap = E.lds_capacity(dtype)
    for n, kid in ((40001, 57), (cap, 56), (cap + 1, 57)):  # 40001: three (float32) / five (float64) units per segment and image
        del events[:]
        for name, values in all_pools(dtype, 2, n, seed=7).items():
            x = torch.from_numpy(values).to(DEV)
            coeffs = [torch.ones(2, 2, dtype=dtype, device=DEV), x]
            for k in (1, n // 2, n):
                check(coeffs, k, 1, what=f"{name} n={n}", decode=k == n // 2)
        assert {e[1] for e in events if e[0] == "compact_encode"} == {kid}


# ---- order and quota -------------------------------------------------------------------------------------------------------------------
@DTYPES
@ROUTES
def test_equal_pool_keeps_the_first_k(dtype, route, monkeypatch, canaries):
    force(monkeypatch, route)
    for n in (257, 40001):
        values = R.pools(NP[dtype], 2, n, seed=1)["equal"]
        coeffs = segmented(values, dtype)
        k = n // 2
        s = check(coeffs, k, 1, what=f"equal n={n}")
        assert s.indices.cpu().tolist() == [list(range(k))] * 2
        assert s.counts.cpu().tolist() == [k, k]


def _units(n, dtype):
    """Elements per unit of a dense 16-byte-aligned row of ``n`` elements on the streaming route (csrc/mifwt_bands.h: unit_plan)."""
    vec = 16 // torch.empty(0, dtype=dtype).element_size()
    slots = (n + 2 * vec - 2) // vec
    wpi = -(-slots // 4096)
    spw = -(-slots // wpi)
    return spw * vec, -(-slots // spw)


@DTYPES
@ROUTES
def test_tie_cut_in_a_first_chunk_a_later_chunk_on_a_boundary_and_in_a_later_segment(dtype, route, monkeypatch, canaries):
    force(monkeypatch, route)
    n0, n1 = 40001, 9000
    per_unit, units = _units(n0, dtype)
    assert units >= 3
    i = np.arange(n0 + n1)
    row = np.where(i % 1000 == 0, 3.0, np.where(i % 10 == 7, 1e-3, 0.25)) * np.where(i % 3 == 0, -1.0, 1.0)  # "three": heavy ties
    values = np.stack([row, row[::-1] * 1.0]).astype(NP[dtype])
    x = torch.from_numpy(values).to(DEV)
    coeffs = [torch.ones(2, 2, dtype=dtype, device=DEV), x[:, :n0].contiguous(), x[:, n0:].contiguous()]
    assert coeffs[1].data_ptr() % 16 == 0
    big = int((np.abs(row) == 3.0).sum())
    ties_before = np.concatenate([[0], np.cumsum(np.abs(row) == 0.25)])  # ties before flat index j of image 0
    cuts = {"first chunk": 100, "later chunk": per_unit + per_unit // 2, "chunk boundary": per_unit, "second boundary": 2 * per_unit,
            "later segment": n0 + 500}
    for name, j in cuts.items():
        for quota in (ties_before[j] - 1, ties_before[j], ties_before[j] + 1):
            s = check(coeffs, big + int(quota), 1, what=name, decode=False)
            kept = s.indices[0].cpu().numpy()
            tie_idx = kept[np.abs(row[kept]) == 0.25]
            assert tie_idx.size == quota and j - 4 < tie_idx.max() < j + 4, name  # the cut lies where it was put


@DTYPES
@ROUTES
def test_three_pool_every_seventh_k(dtype, route, monkeypatch, canaries):
    force(monkeypatch, route)
    n = 1000
    values = R.pools(NP[dtype], 2, n, seed=4)["three"]
    coeffs = segmented(values, dtype)
    for k in range(0, n + 1, 7):
        check(coeffs, k, 1, what="three", decode=False)


# ---- containers -------------------------------------------------------------------------------------------------------------------------
def _real_containers(dtype):
    g = torch.Generator().manual_seed(1)
    r = lambda *shape: torch.randn(*shape, generator=g, dtype=dtype).to(DEV)
    return {"wavedec2": (ptwt_amd.wavedec2(r(3, 37, 41), "db2", level=3), 1),
            "wavedec": (ptwt_amd.wavedec(r(5, 1003), "db5", level=4), 1),
            "wavedec3": (ptwt_amd.wavedec3(r(2, 20, 20, 20), "haar", level=4), 1),
            "two leading axes": (ptwt_amd.wavedec2(r(2, 3, 21, 27), "db2", level=2), 2)}


@DTYPES
@ROUTES
def test_real_containers(dtype, route, monkeypatch, canaries):
    force(monkeypatch, route)
    for name, (coeffs, lead) in _real_containers(dtype).items():
        if name == "wavedec2":
            assert any(not t.is_contiguous() or t.data_ptr() % 16 for t in leaves(coeffs[1:]))  # misaligned strided views
        if name == "wavedec3":
            assert len(leaves(coeffs)) == 29 > S.max_segments()
        for approx in (False, True):
            for keep in (0.05, 0.5, 1):
                s = check(coeffs, keep, lead, approx=approx, what=f"{name} approx={approx}")
            assert tuple(s.counts.shape) == tuple(leaves(coeffs)[-1].shape[:lead]) == s.layout.lead
            ts = pooled(coeffs, approx)
            n = sum(t.numel() for t in ts) // int(np.prod(s.layout.lead))
            ties = R.pools(NP[dtype], int(np.prod(s.layout.lead)), n, seed=5)["three"]
            saved = [t.clone() for t in ts]
            fill(ts, ties)
            for keep in (0.3, 0.7):
                check(coeffs, keep, lead, approx=approx, what=f"{name} three approx={approx}")
            for t, v in zip(ts, saved):
                t.copy_(v)


@DTYPES
@ROUTES
def test_a_list_of_29_tensors_and_empty_tensors(dtype, route, monkeypatch, canaries):
    force(monkeypatch, route)
    g = torch.Generator().manual_seed(2)
    many = [torch.randn(2, 3 + 5 * (i % 7), generator=g, dtype=dtype).to(DEV) for i in range(29)]
    many[5] = torch.empty(2, 0, dtype=dtype, device=DEV)
    for keep in (1, 0.2, 1.0):
        s = check(many, keep, 1, approx=True, what="29 tensors")
        check(many, keep, 1, what="28 tensors")
    assert len(s.layout.entries) == 29 and s.layout.entries[5][0] == (2, 0)
    holes = [torch.randn(3, 4, generator=g, dtype=dtype).to(DEV), torch.empty(3, 0, dtype=dtype, device=DEV),
             torch.randn(3, 9, generator=g, dtype=dtype).to(DEV), torch.empty(3, 0, 5, dtype=dtype, device=DEV),
             torch.randn(3, 6, generator=g, dtype=dtype).to(DEV)]
    for keep in (0, 4, 15):
        check(holes, keep, 1, what="empty tensors")


@DTYPES
@ROUTES
def test_a_bare_tensor_is_one_pool(dtype, route, monkeypatch, canaries):
    force(monkeypatch, route)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 7, generator=g, dtype=dtype).to(DEV)
    s = check(x, 10, 0, what="bare")
    assert s.values.shape == (10,) and s.indices.shape == (10,) and s.counts.shape == () and s.layout.lead == ()
    assert isinstance(ptwt_amd.sparse_decode(s), torch.Tensor)
    check(x.t(), 0.5, 0, what="bare, transposed")  # no collapsed form: read from a contiguous copy, in row-major order


# ---- k on the device -------------------------------------------------------------------------------------------------------------------
@DTYPES
@ROUTES
def test_tensor_keep(dtype, route, monkeypatch, canaries):
    force(monkeypatch, route)
    coeffs, _ = _real_containers(dtype)["wavedec2"]
    n = sum(t[0].numel() for t in leaves(coeffs[1:]))
    for capacity in (40, 1000, n):
        for ks in ([5, 900, n], [-7, 0, n + 100], [capacity, capacity + 1, capacity - 1]):  # below 0 and above the capacity: clipped
            kt = torch.tensor(ks, dtype=torch.int64, device=DEV)
            s = check(coeffs, kt, 1, capacity=capacity, what=f"k = {ks}")
            want = np.clip(ks, 0, capacity)
            assert s.counts.cpu().tolist() == want.tolist()
            for g in range(3):  # the padding
                assert not bool(s.values[g, want[g]:].any()) and bool((s.indices[g, want[g]:] == -1).all())
                assert bool((s.indices[g, : want[g]] >= 0).all())
        for k1 in (17, -1, 10 ** 12):
            s = check(coeffs, torch.tensor([k1], dtype=torch.int64, device=DEV), 1, capacity=capacity, what=f"k = [{k1}]")
            assert s.counts.cpu().tolist() == [min(max(k1, 0), capacity)] * 3
    s = check(coeffs, 10, 1, capacity=25, what="an int keep below the capacity")
    assert s.values.shape == (3, 25) and s.counts.cpu().tolist() == [10] * 3


# ---- capture -----------------------------------------------------------------------------------------------------------------------------
@DTYPES
@ROUTES
def test_captured_call_replays_on_new_data_and_new_k(dtype, route, monkeypatch):
    force(monkeypatch, route)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 64, 72, generator=g, dtype=dtype).to(DEV)
    kt = torch.tensor([100, 400], dtype=torch.int64, device=DEV)
    K = 500

    def fn(t):
        s = ptwt_amd.sparse_encode(ptwt_amd.wavedec2(t, "db4", level=3), kt, capacity=K)
        return s.values, s.indices, s.counts, ptwt_amd.waverec2(ptwt_amd.sparse_decode(s), "db4")

    def reference(t, ks):
        tn = [c.cpu().numpy() for c in leaves(ptwt_amd.wavedec2(t, "db4", level=3)[1:])]
        return R.encode(tn, 1, np.array(ks), K)

    cap = ptwt_amd.capture(fn, x)
    for t, ks in ((x, [100, 400]), (torch.randn(2, 64, 72, generator=g, dtype=dtype).to(DEV) * 3, [100, 400]), (x, [7, 3000]), (x, [0, 1])):
        kt.copy_(torch.tensor(ks, dtype=torch.int64, device=DEV))
        got = [o.clone() for o in cap(t)]
        for a, b in zip(got[:3], reference(t, ks)):
            assert same_bits(a.cpu().numpy(), b), ks
        assert all(torch.equal(a, b) for a, b in zip(got, fn(t)))
        assert got[2].cpu().tolist() == np.clip(ks, 0, K).tolist()


# ---- decode ------------------------------------------------------------------------------------------------------------------------------
@DTYPES
@ROUTES
def test_decode_is_sparsify_hard_on_tie_free_data_in_one_backing_allocation(dtype, route, monkeypatch, canaries):
    force(monkeypatch, route)
    monkeypatch.setattr(SP, "FORCE_STREAM", route == "stream")
    for name, (coeffs, lead) in _real_containers(dtype).items():
        ts = leaves(coeffs[1:])
        images = int(np.prod(ts[0].shape[:lead]))
        n = sum(t.numel() for t in ts) // images
        fill(ts, R.tie_free(NP[dtype], images, n, seed=3))
        for keep in (1, 0.05, n - 1):
            s = ptwt_amd.sparse_encode(coeffs, keep)
            back = ptwt_amd.sparse_decode(s)
            want = ptwt_amd.sparsify(coeffs, keep, "hard")
            assert back[0] is coeffs[0] is want[0]
            outs = leaves(back[1:])
            for a, b in zip(outs, leaves(want[1:])):
                assert a.shape == b.shape and same_bits(a.cpu().numpy(), b.cpu().numpy()), (name, keep)
            assert all(o.is_contiguous() and o.data_ptr() % 256 == 0 for o in outs)
            assert len({o.untyped_storage().data_ptr() for o in outs}) == 1  # one backing allocation
            assert int(sum((o != 0).sum() for o in outs)) == images * R0.k_of(keep, n)


@DTYPES
def test_two_runs_give_the_same_bits(dtype, canaries):
    values = R.pools(NP[dtype], 2, 70001, seed=9)["three"]
    coeffs = segmented(values, dtype)
    a, b = ptwt_amd.sparse_encode(coeffs, 0.4), ptwt_amd.sparse_encode(coeffs, 0.4)
    assert torch.equal(a.values, b.values) and torch.equal(a.indices, b.indices) and torch.equal(a.counts, b.counts)
    for p, q in zip(leaves(ptwt_amd.sparse_decode(a)), leaves(ptwt_amd.sparse_decode(b))):
        assert torch.equal(p, q)


# ---- gradients ---------------------------------------------------------------------------------------------------------------------------
def _grad_container(dtype, requires_grad=True):
    base, _ = _real_containers(dtype)["wavedec2"]
    xs = [t.detach().clone().requires_grad_(requires_grad) for t in leaves(base[1:])]
    it = iter(xs)
    return [base[0]] + [type(e)(*[next(it) for _ in e]) for e in base[1:]], xs


@DTYPES
@ROUTES
def test_first_order_gradients_are_the_composed_ones(dtype, route, monkeypatch, canaries, events):
    force(monkeypatch, route)
    coeffs, xs = _grad_container(dtype)
    k = 200
    g = torch.Generator().manual_seed(7)
    wv = torch.randn(3, k, generator=g, dtype=dtype).to(DEV)
    ws = [torch.randn(t.shape, generator=g, dtype=dtype).to(DEV) for t in xs]
    del events[:]
    s = ptwt_amd.sparse_encode(coeffs, k)
    assert s.values.requires_grad and not s.indices.requires_grad and not s.counts.requires_grad
    got_x = torch.autograd.grad((s.values * wv).sum(), xs)  # the encode backward: a scatter
    assert [e[0] for e in events] == ["select_kth", "compact_encode", "compact_scatter"]
    v = s.values.detach().clone().requires_grad_(True)
    sv = S.SparseCoeffs(values=v, indices=s.indices, counts=s.counts, approx=s.approx, layout=s.layout)
    del events[:]
    back = ptwt_amd.sparse_decode(sv)
    got_v, = torch.autograd.grad(sum((y * w).sum() for y, w in zip(leaves(back[1:]), ws)), [v])  # the decode backward: a gather
    assert [e[0] for e in events] == ["compact_scatter", "compact_gather"]
    # the composed route
    values, indices, counts = S._composed_encode(xs, 1, k, None, k)
    assert torch.equal(values, s.values) and torch.equal(indices, s.indices) and torch.equal(counts, s.counts)
    want_x = torch.autograd.grad((values * wv).sum(), xs)
    v2 = values.detach().clone().requires_grad_(True)
    outs = S._composed_decode(v2, indices, counts, [tuple(t.shape) for t in xs], s.layout.n)
    want_v, = torch.autograd.grad(sum((y * w).sum() for y, w in zip(outs, ws)), [v2])
    for a, b in zip(got_x + (got_v,), want_x + (want_v,)):
        assert a.dtype == dtype and same_bits(a.cpu().numpy(), b.cpu().numpy())
    assert bool((got_v != 0).any()) and int(sum((a != 0).sum() for a in got_x)) == 3 * k


@ROUTES
def test_second_order_runs_on_the_composition(route, monkeypatch):
    force(monkeypatch, route)
    dtype = torch.float64
    g = torch.Generator().manual_seed(11)
    a = torch.randn(2, 4, generator=g, dtype=dtype).to(DEV)
    x0 = torch.randn(2, 50, generator=g, dtype=dtype).to(DEV)
    w = torch.randn(2, 50, generator=g, dtype=dtype).to(DEV)

    def second(encode_decode):
        x = x0.clone().requires_grad_(True)
        values, dense = encode_decode(x)
        loss = (values ** 3).sum() + (dense ** 3 * w).sum()
        g1, = torch.autograd.grad(loss, x, create_graph=True)
        g2, = torch.autograd.grad((g1 ** 2).sum(), x)
        return g1.detach(), g2

    def kernels(x):
        s = ptwt_amd.sparse_encode([a, x], 12)
        return s.values, ptwt_amd.sparse_decode(s)[1]

    def composed(x):
        values, indices, counts = S._composed_encode([x], 1, 12, None, 12)
        return values, S._composed_decode(values, indices, counts, [(2, 50)], 50)[0]

    got, want = second(kernels), second(composed)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert int((got[1] != 0).sum()) == 24


# ---- no launch ---------------------------------------------------------------------------------------------------------------------------
def test_no_launch_cases(events):
    a = torch.randn(3, 4, device=DEV)
    x = torch.randn(3, 9, device=DEV, dtype=torch.float32)
    for keep, kw in ((0, {}), (0.0, {}), (torch.tensor([1, 2, 3], device=DEV), {"capacity": 0})):  # K == 0
        s = ptwt_amd.sparse_encode([a, x], keep, **kw)
        assert s.values.shape == (3, 0) and s.values.dtype == torch.float32 and s.indices.shape == (3, 0) and s.indices.dtype == torch.int32
        assert s.counts.shape == (3,) and s.counts.dtype == torch.int32 and s.counts.tolist() == [0, 0, 0] and s.approx is a
        back = ptwt_amd.sparse_decode(s)
        assert back[0] is a and back[1].shape == (3, 9) and not bool(back[1].any())
    empty = [a, torch.empty((3, 0), device=DEV), torch.empty((3, 0), device=DEV)]  # an empty pool
    for keep, kw in ((0, {}), (0.5, {}), (torch.tensor([1], device=DEV), {"capacity": 0})):
        s = ptwt_amd.sparse_encode(empty, keep, **kw)
        assert s.values.shape == (3, 0) and s.counts.tolist() == [0, 0, 0] and s.layout.n == 0
        back = ptwt_amd.sparse_decode(s)
        assert back[0] is a and [t.shape for t in back[1:]] == [(3, 0), (3, 0)]
    none = [torch.empty((0, 4), device=DEV, dtype=torch.float64), torch.empty((0, 4), device=DEV, dtype=torch.float64)]  # no image
    for keep, cap in ((0, 0), (3, 3), (0.5, 4)):
        s = ptwt_amd.sparse_encode(none, keep, approx=True)
        assert s.values.shape == (0, cap) and s.values.dtype == torch.float64 and s.indices.shape == (0, cap) and s.counts.shape == (0,)
        assert [t.shape for t in ptwt_amd.sparse_decode(s)] == [(0, 4), (0, 4)]
    assert events == []
