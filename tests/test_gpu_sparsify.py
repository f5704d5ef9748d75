"""keep_threshold / sparsify on the GPU (kernel ids 54 / 55, csrc/mifwt_select.hip) against the numpy reference of
tests/_sparsify_ref.py: per image ``abs``, concatenate, ``numpy.sort``, ``s[n - k]``.

Tolerance 0 everywhere: the selection moves bits and computes nothing, so values are compared bit for bit; ``sparsify`` must equal
``ptwt_amd.threshold`` with the reference value on every pooled tensor, bit for bit.  Every allocation a kernel writes is carved out of
canary bytes (tests/test_gpu_canaries.py)."""
import importlib

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, estimators as E, thresholding as T
from tests import _sparsify_ref as R
from tests.test_gpu_canaries import _GuardedTorch

S = importlib.import_module("ptwt_amd.sparsify")  # (the package attribute of that name is the function)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NP = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
ROUTES = pytest.mark.parametrize("route", ["default", "stream"])


@pytest.fixture()
def canaries(monkeypatch):
    g = _GuardedTorch()
    for mod in (S, E, T, _engine):
        monkeypatch.setattr(mod, "torch", g)
    yield g
    g.check("sparsify")


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


def to_np(ts):
    return [t.detach().cpu().numpy() for t in ts]


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def fill(tensors, values):
    """Write the pool ``values`` [images, n] into ``tensors`` in place of their values, in pooling order."""
    off = 0
    for t in tensors:
        m = t[0].numel()
        t.copy_(torch.from_numpy(values[:, off:off + m].copy()).reshape(t.shape))
        off += m
    assert off == values.shape[1]


def pooled(coeffs, approx=False):
    return leaves(coeffs if approx else coeffs[1:])


def check_value(coeffs, keep, approx=False, what=""):
    """keep_threshold bit-equal to the reference; returns (the reference value as a device tensor, the pooled arrays, lead)."""
    ts = pooled(coeffs, approx)
    lead = ts[-1].dim() - _axes(coeffs)
    tn = to_np(ts)
    n = R.pool(tn, lead).shape[1]
    k = keep.cpu().numpy() if isinstance(keep, torch.Tensor) else R.k_of(keep, n)
    want = R.kth(tn, lead, k)
    got = ptwt_amd.keep_threshold(coeffs, keep, approx=approx)
    assert got.dtype == ts[0].dtype and got.device == ts[0].device and not got.requires_grad
    assert same_bits(got.cpu().numpy(), want), (what, keep, got.cpu().numpy(), want)
    return torch.from_numpy(want).to(DEV), tn, lead


def _axes(coeffs):
    """Transformed axes of a container, from its last entry."""
    last = coeffs[-1]
    if isinstance(last, torch.Tensor):
        return 1
    if isinstance(last, dict):
        return len(next(iter(last)))
    return 2


def check_sparsify(coeffs, keep, mode, v, approx=False, what=""):
    """sparsify bit-equal to ``threshold`` with the reference value ``v`` on every pooled entry; returns the pooled outputs."""
    got = ptwt_amd.sparsify(coeffs, keep, mode, approx=approx)
    want = ptwt_amd.threshold(coeffs, ([v] if approx else [None]) + [v] * (len(coeffs) - 1), mode)
    assert type(got) is type(coeffs) and len(got) == len(coeffs)
    if not approx:
        assert got[0] is coeffs[0]
    for a, b, x in zip(leaves(got), leaves(want), leaves(coeffs)):
        assert a.shape == x.shape and a.dtype == x.dtype and same_bits(a.cpu().numpy(), b.cpu().numpy()), (what, keep, mode)
    return pooled(got, approx)


def container2(dtype):
    g = torch.Generator().manual_seed(1)
    return ptwt_amd.wavedec2(torch.randn(3, 37, 41, generator=g, dtype=dtype).to(DEV), "db2", level=2)


# ---- adversarial pools, every rank -----------------------------------------------------------------------------------------------------
@DTYPES
@ROUTES
def test_adversarial_pools_every_rank(dtype, route, monkeypatch, canaries, events):
    force(monkeypatch, route)
    coeffs = container2(dtype)
    ts = pooled(coeffs)
    assert any(not t.is_contiguous() for t in ts)  # strided views of level buffers
    n = sum(t[0].numel() for t in ts)
    assert n == 1716
    for name, values in R.pools(NP[dtype], 3, n, seed=2).items():
        fill(ts, values)
        for keep in (0, 1, 2, n // 2, n - 1, n, 0.0, 0.05, 0.5, 1.0):
            v, tn, lead = check_value(coeffs, keep, what=f"{name} {route}")
            out = check_sparsify(coeffs, keep, "hard", v, what=f"{name} {route}")
            vb = v.reshape(-1, 1)
            alive = torch.stack([(o.reshape(3, -1).abs() >= vb).sum(1) for o in out]).sum(0).cpu().numpy()
            assert alive.tolist() == R.survivors(tn, lead, v.cpu().numpy()).tolist(), (name, keep)
            k = R.k_of(keep, n)
            assert bool((alive >= k).all())
    assert {e[1] for e in events if e[0] == "select_kth"} == ({55} if route == "stream" else {54})


@DTYPES
@ROUTES
def test_tie_free_input_keeps_exactly_k(dtype, route, monkeypatch, canaries):
    force(monkeypatch, route)
    coeffs = container2(dtype)
    ts = pooled(coeffs)
    n = sum(t[0].numel() for t in ts)
    values = R.tie_free(NP[dtype], 3, n, seed=3)
    for g in range(3):
        assert np.unique(np.abs(values[g])).size == n  # distinct by construction
    fill(ts, values)
    for k in (1, 86, n - 1):
        out = ptwt_amd.sparsify(coeffs, k, "hard")
        nonzero = torch.stack([(o.reshape(3, -1) != 0).sum(1) for o in pooled(out)]).sum(0).tolist()
        assert nonzero == [k] * 3, (k, nonzero)


# ---- routes ------------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_capacity_boundary(dtype, canaries, events):
    cap = E.lds_capacity(dtype)
    for extra, kid in ((0, 54), (1, 55)):
        g = torch.Generator().manual_seed(4)
        coeffs = [torch.randn(2, 4, generator=g, dtype=dtype).to(DEV), torch.randn(2, cap - 1001, generator=g, dtype=dtype).to(DEV),
                  torch.randn(2, 1001 + extra, generator=g, dtype=dtype).to(DEV)]
        del events[:]
        for keep in (1, 0.05, cap // 2, cap + extra):
            check_value(coeffs, keep, what=f"cap + {extra}")
        assert [e[:2] for e in events] == [("select_kth", kid)] * 4


@DTYPES
def test_several_chunks_per_image_on_adversarial_pools(dtype, canaries, events):
    n = 70001  # 5 (float32) / 9 (float64) workgroups per image flush into the same counters
    for name, values in R.pools(NP[dtype], 2, n, seed=10).items():
        x = torch.from_numpy(values).to(DEV)
        for keep in (1, 0.05, n // 2, n):
            got = ptwt_amd.keep_threshold(x, keep, lead=1)
            assert same_bits(got.cpu().numpy(), R.kth([values], 1, R.k_of(keep, n))), (name, keep)
    assert {e[1] for e in events} == {55}


@DTYPES
@ROUTES
def test_more_tensors_than_one_launch_holds(dtype, route, monkeypatch, canaries, events):
    force(monkeypatch, route)
    g = torch.Generator().manual_seed(5)
    coeffs = ptwt_amd.wavedec3(torch.randn(2, 20, 20, 20, generator=g, dtype=dtype).to(DEV), "haar", level=4)
    assert len(leaves(coeffs)) == 29 > S.max_segments()
    del events[:]
    for keep in (1, 0.05, 4000):
        v, _, _ = check_value(coeffs, keep, approx=True, what="wavedec3")
        check_sparsify(coeffs, keep, "hard", v, approx=True, what="wavedec3")
        v, _, _ = check_value(coeffs, keep, what="wavedec3 details")  # 28 tensors: still more than a launch holds
        check_sparsify(coeffs, keep, "soft", v, what="wavedec3 details")
    assert {e[1] for e in events if e[0] == "select_kth"} == {55}  # (whatever the pool's size: the LDS launch holds one table)


@DTYPES
@ROUTES
def test_lists_of_wavedec_and_swt(dtype, route, monkeypatch, canaries):
    force(monkeypatch, route)
    g = torch.Generator().manual_seed(6)
    c1 = ptwt_amd.wavedec(torch.randn(5, 1003, generator=g, dtype=dtype).to(DEV), "db5", level=4)
    cs = ptwt_amd.swt(torch.randn(4, 96, generator=g, dtype=dtype).to(DEV), "db2", level=2)
    for name, coeffs in (("wavedec", c1), ("swt", cs)):
        for keep in (0, 3, 0.05, 0.5):
            for approx in (False, True):
                v, _, _ = check_value(coeffs, keep, approx=approx, what=name)
                for mode in ("hard", "soft", "garrote"):
                    if keep != 0:  # (soft / garrote at +inf divide inf by inf where the data holds inf; hard has no arithmetic)
                        check_sparsify(coeffs, keep, mode, v, approx=approx, what=name)
                check_sparsify(coeffs, keep, "hard", v, approx=approx, what=name)


# ---- k on the device ---------------------------------------------------------------------------------------------------------------------
@DTYPES
@ROUTES
def test_per_image_k_on_the_device(dtype, route, monkeypatch, canaries):
    force(monkeypatch, route)
    coeffs = container2(dtype)
    n = 1716
    for ks in ([5, 900, n], [-7, 0, n + 100], [1, 1, 2]):  # below 0 and above n: clipped
        kt = torch.tensor(ks, dtype=torch.int64, device=DEV)
        v, _, _ = check_value(coeffs, kt, what=f"k = {ks}")
        check_sparsify(coeffs, kt, "hard", v, what=f"k = {ks}")
    for k1 in (17, -1, 10 ** 12):
        kt = torch.tensor([k1], dtype=torch.int64, device=DEV)  # one element: every image
        v, _, _ = check_value(coeffs, kt, what=f"k = [{k1}]")
        assert same_bits(v.cpu().numpy(), ptwt_amd.keep_threshold(coeffs, min(max(k1, 0), n)).cpu().numpy())
    # a bare tensor: everything pooled, lead as in estimate_sigma
    x = leaves(coeffs)[1]
    xn = x.cpu().numpy()
    got = ptwt_amd.keep_threshold(x, torch.tensor([3, 0, 50], dtype=torch.int64, device=DEV), lead=1)
    assert same_bits(got.cpu().numpy(), R.kth([xn], 1, np.array([3, 0, 50])))
    got = ptwt_amd.keep_threshold(x, 0.25)
    assert got.shape == () and same_bits(got.cpu().numpy(), R.kth([xn], 0, R.k_of(0.25, xn.size)))
    out = ptwt_amd.sparsify(x, 10)
    assert same_bits(out.cpu().numpy(), ptwt_amd.threshold(x, float(R.kth([xn], 0, 10)), "hard").cpu().numpy())


# ---- approx ------------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_approx_semantics(dtype, canaries):
    coeffs = container2(dtype)
    coeffs[0].mul_(1000.0)  # the approximation dominates whatever pool it is in
    k = 50
    apart = ptwt_amd.keep_threshold(coeffs, k)
    whole = ptwt_amd.keep_threshold(coeffs, k, approx=True)
    assert same_bits(apart.cpu().numpy(), R.kth(to_np(leaves(coeffs)[1:]), 1, k))
    assert same_bits(whole.cpu().numpy(), R.kth(to_np(leaves(coeffs)), 1, k))
    assert bool((whole > apart).all())
    out = ptwt_amd.sparsify(coeffs, k)
    assert out[0] is coeffs[0]
    out = ptwt_amd.sparsify(coeffs, k, approx=True)
    assert out[0] is not coeffs[0] and out[0].data_ptr() != coeffs[0].data_ptr()
    assert torch.equal(out[0], torch.where(coeffs[0].abs() >= whole.reshape(3, 1, 1), coeffs[0], torch.zeros_like(coeffs[0])))
    assert sum(int((o != 0).sum()) for o in leaves(out)) == 3 * k  # (random data: no ties)


# ---- gradient ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["hard", "soft", "garrote"])
def test_data_gradient(mode, canaries, events):
    dtype = torch.float64
    base = container2(dtype)
    xs = [t.detach().clone().requires_grad_(True) for t in leaves(base[1:])]
    it = iter(xs)
    coeffs = [base[0]] + [type(e)(*[next(it) for _ in e]) for e in base[1:]]
    g = torch.Generator().manual_seed(7)
    ws = [torch.randn(t.shape, generator=g, dtype=dtype).to(DEV) for t in xs]
    k = 200
    del events[:]
    out = ptwt_amd.sparsify(coeffs, k, mode)
    got = torch.autograd.grad(sum((y * w).sum() for y, w in zip(leaves(out[1:]), ws)), xs)
    assert [e[0] for e in events] == ["select_kth", "thresh_fwd", "thresh_bwd"]
    v = torch.from_numpy(R.kth(to_np(xs), 1, k)).to(DEV)  # held constant
    ref = ptwt_amd.threshold(coeffs, [None, v, v], mode)
    want = torch.autograd.grad(sum((y * w).sum() for y, w in zip(leaves(ref[1:]), ws)), xs)
    for a, b in zip(got, want):
        assert a.dtype == dtype and torch.equal(a, b)
    assert any(bool((a != 0).any()) for a in got)


# ---- capture -----------------------------------------------------------------------------------------------------------------------------
@DTYPES
@ROUTES
def test_captured_pipeline_replays_on_new_data_and_new_k(dtype, route, monkeypatch):
    force(monkeypatch, route)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 64, 72, generator=g, dtype=dtype).to(DEV)
    kt = torch.tensor([100, 400], dtype=torch.int64, device=DEV)

    def fn(t):
        return ptwt_amd.waverec2(ptwt_amd.sparsify(ptwt_amd.wavedec2(t, "db4", level=3), kt), "db4")

    cap = ptwt_amd.capture(fn, x)
    first = cap(x).clone()
    assert torch.equal(first, fn(x))
    y = torch.randn(2, 64, 72, generator=g, dtype=dtype).to(DEV) * 3
    assert torch.equal(cap(y).clone(), fn(y))  # new data
    kt.copy_(torch.tensor([7, 3000], dtype=torch.int64, device=DEV))
    third = cap(y).clone()
    assert torch.equal(third, fn(y))  # new contents of the k tensor
    assert not torch.equal(third, first)
    kt.copy_(torch.tensor([100, 400], dtype=torch.int64, device=DEV))
    assert torch.equal(cap(x), first)


# ---- reproducibility and edge launches -----------------------------------------------------------------------------------------------------
@DTYPES
@ROUTES
def test_two_runs_give_the_same_bits(dtype, route, monkeypatch, canaries):
    force(monkeypatch, route)
    g = torch.Generator().manual_seed(9)
    coeffs = ptwt_amd.wavedec2(torch.randn(2, 300, 290, generator=g, dtype=dtype).to(DEV), "db3", level=2)  # two chunks per fine band
    a, b = ptwt_amd.keep_threshold(coeffs, 0.1), ptwt_amd.keep_threshold(coeffs, 0.1)
    assert same_bits(a.cpu().numpy(), b.cpu().numpy())
    assert same_bits(a.cpu().numpy(), R.kth(to_np(leaves(coeffs[1:])), 1, R.k_of(0.1, sum(t[0].numel() for t in leaves(coeffs[1:])))))
    o1, o2 = ptwt_amd.sparsify(coeffs, 0.1, "soft"), ptwt_amd.sparsify(coeffs, 0.1, "soft")
    assert all(torch.equal(p, q) for p, q in zip(leaves(o1), leaves(o2)))


def test_empty_pools_and_no_images_launch_nothing(events):
    a = torch.randn(3, 4, device=DEV)
    coeffs = [a, torch.empty((3, 0), device=DEV), torch.empty((3, 0), device=DEV)]
    for keep in (0, 0.5, 1.0, torch.tensor([1, 2, 3], device=DEV)):
        v = ptwt_amd.keep_threshold(coeffs, keep)
        assert v.shape == (3,) and v.dtype == torch.float32 and bool(torch.isinf(v).all()) and bool((v > 0).all())
        out = ptwt_amd.sparsify(coeffs, keep)
        assert out[0] is a and out[1].shape == (3, 0) and out[2].shape == (3, 0)
    none = [torch.empty((0, 4), device=DEV), torch.empty((0, 4), device=DEV), torch.empty((0, 7), device=DEV)]
    for keep in (0, 3, 0.5):
        assert ptwt_amd.keep_threshold(none, keep).shape == (0,)
        out = ptwt_amd.sparsify(none, keep, approx=True)
        assert [o.shape for o in out] == [(0, 4), (0, 4), (0, 7)]
    assert ptwt_amd.keep_threshold(torch.empty((0, 5), device=DEV), 2, lead=1).shape == (0,)
    assert events == []
