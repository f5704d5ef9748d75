"""threshold / threshold_firm on the GPU (kernel ids 48 / 49, csrc/mifwt_thresh.hip) against the float64 reference of
tests/_thresh_ref.py on the same representable inputs.

Forward bound, element by element: ``|err| <= 8 eps max(|x|, v, |substitute|)`` with ``eps`` of the arithmetic type (float32 for
float32 / complex64 / 16-bit storage, float64 otherwise) — each closed form is at most four roundings of quantities bounded by that
maximum — plus half an ulp of the storage type for float16 / bfloat16; the decisions (kept, replaced, zeroed) must agree EXACTLY,
thresholds being multiples of 1/8.  Every allocation a kernel writes is carved out of a block of canary bytes that must stay intact
(the helper of tests/test_gpu_canaries.py)."""
import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, thresholding as T
from tests import _thresh_ref as R
from tests.test_gpu_canaries import _GuardedTorch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}  # unit roundoffs; the bound's "eps" is the spacing, twice that
HALF_ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 257, 1023, 4099)
MODES = ("soft", "hard", "garrote", "greater", "less", "firm")


@pytest.fixture(autouse=True)
def canaries(monkeypatch):
    """Every tensor the thresholding module or the launch path allocates sits between guard bytes; they are checked after each test."""
    g = _GuardedTorch()
    monkeypatch.setattr(T, "torch", g)
    monkeypatch.setattr(_engine, "torch", g)
    yield g
    g.check("threshold")


def arith_of(dtype):
    return torch.float64 if dtype in (torch.float64, torch.complex128) else torch.float32


def draw(shape, dtype, seed, values=(), scale=2.0):
    """Data of ``dtype`` on the device with exact ties planted: +-v for every threshold, 0."""
    g = torch.Generator().manual_seed(seed)
    real = dtype if not dtype.is_complex else arith_of(dtype)
    n = int(np.prod(shape))
    if dtype.is_complex:
        x = torch.complex(torch.randn(n, generator=g, dtype=torch.float64), torch.randn(n, generator=g, dtype=torch.float64)) * scale
        x = x.to(dtype)
        special = [0j] + [c * v / 5 for v in values for c in (3 + 4j, -4 + 3j)]  # |3 + 4i| = 5: magnitudes exactly v
    else:
        x = (torch.randn(n, generator=g, dtype=torch.float64) * scale).to(real)
        special = [0.0] + [s * v for v in values for s in (1.0, -1.0)]
    for k, s in enumerate(special):
        if 3 * k + 1 < n:
            x[3 * k + 1] = s
    return x.reshape(shape).to(DEV)


def run(x, mode, value=1.25, hi=2.5, sub=0.0):
    if mode == "firm":
        return ptwt_amd.threshold_firm(x, value, hi), R.threshold_firm(up(x), value, hi)
    return ptwt_amd.threshold(x, value, mode, sub), R.threshold(up(x), value, mode, sub)


def up(t):
    if not isinstance(t, torch.Tensor):
        return R._map(up, t, ())
    return t.to(torch.complex128 if t.is_complex() else torch.float64)


def check(got, x, ref, vmax, sub=0.0, what=""):
    """The element-wise bound and the exact agreement of the decisions; ``vmax``: the largest threshold of each element."""
    assert got.dtype == x.dtype and got.shape == x.shape, what
    x64, got64 = up(x), up(got)
    eps = 2 * EPS[arith_of(x.dtype)]
    bound = 8 * eps * torch.maximum(x64.abs(), torch.as_tensor(vmax, dtype=torch.float64, device=x.device)).clamp(min=abs(sub))
    if x.dtype in HALF_ULP:
        bound = bound + HALF_ULP[x.dtype] * ref.abs() + 2.0 ** -25
    err = (got64 - ref).abs()
    assert bool((err <= bound).all()), f"{what}: error {float((err / bound.clamp(min=1e-300)).max()):.3g} x the bound"
    assert torch.equal(got64 == 0, ref == 0), f"{what}: the zeroed elements differ"
    if x.dtype not in HALF_ULP:  # (rounded to 16 bits a shrunk element may land on its input again)
        assert torch.equal(got64 == x64, ref == x64), f"{what}: the kept elements differ"
    if sub != 0.0:
        assert torch.equal(got64 == sub, ref == sub), f"{what}: the replaced elements differ"


# ---- forward, single tensors -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode", MODES)
def test_forward_sizes_and_views(dtype, mode):
    before = _engine.launch_count(48)
    calls = 0
    for n in SIZES:
        x = draw((n,), dtype, n, (1.25, 2.5))
        keep = x.clone()
        for sub in (0.0, -0.75) if mode != "firm" and n in (5, 257) else (0.0,):
            got, ref = run(x, mode, sub=sub)
            check(got, x, ref, 2.5 if mode == "firm" else 1.25, sub, f"{mode} n={n} sub={sub}")
            calls += 1
        assert torch.equal(x, keep)
    # a [3, 7, 13] view of a [3, 4, 7, 13] buffer; a view whose base is one element past a 16-byte boundary (the scalar path: it must
    # neither fault nor round the address down); rows whose misalignment the output shares (the bands of one buffer, all four at once)
    buf = draw((3, 4, 7, 13), dtype, 77, (1.25, 2.5))
    flat = draw((4099 + 8,), dtype, 78, (1.25, 2.5))
    for x in (buf[:, 1], flat[1:4100], flat[5:70]):
        got, ref = run(x, mode)
        check(got, x, ref, 2.5 if mode == "firm" else 1.25, 0.0, f"{mode} view {tuple(x.shape)}")
        calls += 1
    bands = [buf[:, s] for s in range(4)]
    got, ref = run(bands, mode)
    for s in range(4):
        check(got[s], bands[s], ref[s], 2.5 if mode == "firm" else 1.25, 0.0, f"{mode} band {s}")
        assert got[s].stride() == bands[s].stride() and got[s].data_ptr() % 16 == bands[s].data_ptr() % 16  # (the mirrored buffer)
    assert _engine.launch_count(48) - before == calls + 1


def test_forward_threshold_edges():
    for dtype in (torch.float32, torch.float64):
        x = draw((130,), dtype, 5, (1.25,))
        for mode in ("soft", "garrote", "hard"):
            assert torch.equal(ptwt_amd.threshold(x, 0.0, mode), x)  # v = 0: the identity, 0 stays 0 (no 0 / 0)
        got = ptwt_amd.threshold_firm(x, 1.25, 1.25)  # v_hi == v_lo: hard thresholding with substitute 0, a tie is not kept
        assert torch.equal(got, torch.where(x.abs() > 1.25, x, torch.zeros_like(x)))
        assert not bool(torch.isnan(ptwt_amd.threshold_firm(torch.zeros(9, dtype=dtype, device=DEV), 0.0, 0.0)).any())
    e = torch.empty((2, 0, 5), device=DEV)
    before = _engine.launch_count(48)
    out = ptwt_amd.threshold([e, torch.ones(3, device=DEV)], 2.0)
    assert out[0].shape == e.shape and out[0] is not e and not out[1].any()
    assert ptwt_amd.threshold(e, 1.0).shape == e.shape
    assert _engine.launch_count(48) - before == 1  # (empty tensors pass through without a launch)


# ---- forward, 16-bit storage and complex data ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_forward_half_storage(dtype):
    x = draw((4099,), dtype, 9, (1.25, 2.5))
    with pytest.raises(ValueError, match="Input dtype .* not supported"):
        ptwt_amd.threshold(x, 1.25)
    with ptwt_amd.half_storage():
        for mode in MODES:
            for t in (x, x[3:70], x[:5]):
                got, ref = run(t, mode, sub=0.0)
                check(got, t, ref, 2.5 if mode == "firm" else 1.25, 0.0, f"{mode} {dtype} {tuple(t.shape)}")
        got, ref = run(x, "hard", sub=-0.75)
        check(got, x, ref, 1.25, -0.75, f"hard {dtype} substitute")


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128], ids=["c64", "c128"])
def test_forward_complex(dtype):
    for n in (1, 3, 64, 65, 1023, 4099):
        x = draw((n,), dtype, 20 + n, (1.25, 2.5))
        for mode in ("soft", "hard", "garrote", "firm"):
            for t in (x, x[1:]) if n > 1 else (x,):
                got, ref = run(t, mode)
                check(got, t, ref, 2.5 if mode == "firm" else 1.25, 0.0, f"{mode} {dtype} n={n}")
        got, ref = run(x, "hard", sub=-0.75)
        check(got, x, ref, 1.25, -0.75, f"hard {dtype} substitute")
    with pytest.raises(ValueError, match="real data only"):
        ptwt_amd.threshold(x, 1.0, "greater")


# ---- containers ---------------------------------------------------------------------------------------------------------------------
def containers():
    g = torch.Generator().manual_seed(3)
    x1 = (torch.randn(2, 37, generator=g) * 2).to(DEV)
    x2 = (torch.randn(2, 17, 19, generator=g) * 2).to(DEV)
    x3 = (torch.randn(2, 9, 10, 11, generator=g) * 2).to(DEV)
    return {
        "wavedec": ptwt_amd.wavedec(x1, "db2", level=2),
        "wavedec2": ptwt_amd.wavedec2(x2, "db2", level=2),
        "wavedec3": ptwt_amd.wavedec3(x3, "db2", level=3),
        "fswavedec2": ptwt_amd.fswavedec2(x2, "db2", level=2),
        "swt2": ptwt_amd.swt2(x2[:, :16, :16].contiguous(), "db2", level=2),
    }


def same_structure(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.shape == b.shape and a.dtype == b.dtype
    if isinstance(a, dict):
        return type(b) is dict and list(a) == list(b) and all(same_structure(a[k], b[k]) for k in a)
    return type(a) is type(b) and len(a) == len(b) and all(same_structure(u, v) for u, v in zip(a, b))


def own_threshold(values, entry, t):
    """The largest threshold of each element of tensor ``t`` of container entry ``entry``, float64, broadcast against ``t``."""
    best = torch.zeros((), dtype=torch.float64, device=t.device)
    for vals in values:
        v = torch.as_tensor(vals[entry] if isinstance(vals, list) else vals, dtype=torch.float64, device=t.device)
        best = torch.maximum(best, v.reshape(()) if v.numel() == 1 else v.reshape(tuple(v.shape) + (1,) * (t.dim() - v.dim())))
    return best


@pytest.mark.parametrize("name", ["wavedec", "wavedec2", "wavedec3", "fswavedec2", "swt2"])
def test_containers(name):
    data = containers()[name]
    leaves = R.leaves(data)
    owner = T._flatten(data)[1]
    if name == "wavedec3":
        assert len(leaves) == 22
    keep = [t.clone() for t in leaves]
    per_image = torch.tensor([0.5, 1.25], device=DEV)
    per_entry = [None] + [0.25 * (i + 1) for i in range(len(data) - 1)]
    cases = [
        ("soft", (0.75,)), ("garrote", (per_entry,)), ("hard", (per_image,)), ("firm", (0.5, 1.5)), ("firm", (per_image, [2.0] * len(data))),
        ("soft", ([None, per_image] + [0.5] * (len(data) - 2),)),
    ]
    for mode, values in cases:
        _engine.level_events = []
        before = _engine.launch_count(48)
        try:
            if mode == "firm":
                got, ref = ptwt_amd.threshold_firm(data, *values), R.threshold_firm(up(data), *values)
            else:
                got, ref = ptwt_amd.threshold(data, values[0], mode), R.threshold(up(data), values[0], mode)
            events = [e for e in _engine.level_events if e[0] == "thresh_fwd"]
        finally:
            _engine.level_events = None
        assert len(events) == 1 and events[0][1] == 48 and _engine.launch_count(48) - before == 1, (name, mode)
        assert same_structure(data, got) and type(got) is type(data)
        spared = isinstance(values[0], list) and values[0][0] is None
        assert (got[0] is data[0]) == spared
        for i, (g_, x_, r_) in enumerate(zip(R.leaves(got), leaves, R.leaves(ref))):
            if spared and i == 0:
                continue
            assert g_.data_ptr() != x_.data_ptr()
            check(g_, x_, r_, own_threshold(values, owner[i], x_), 0.0, f"{name} {mode} tensor {i}")
    assert all(torch.equal(a, b) for a, b in zip(leaves, keep))  # the library's outputs are not modified


def test_more_tensors_than_one_launch_holds():
    xs = [draw((5 + i,), torch.float32, i, (1.25,)) for i in range(T.max_segments() + 3)]
    before = _engine.launch_count(48)
    got = ptwt_amd.threshold(xs, 1.25, "garrote")
    assert _engine.launch_count(48) - before == 2
    for g_, x_ in zip(got, xs):
        check(g_, x_, R.threshold(up(x_), 1.25, "garrote"), 1.25)


# ---- gradients ----------------------------------------------------------------------------------------------------------------------
def weight(t, i):
    return torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64, device=t.device) + i).reshape(t.shape).to(t.dtype)


def loss_of(out):
    return sum((weight(t, i) * t).sum() for i, t in enumerate(R.leaves(out)))


def pushed(shape, dtype, seed, thresholds):
    """Data at least 1e-3 away from every threshold in magnitude (``thresholds``: tensors that broadcast against ``shape`` from the
    left), so that no tie can flip between the float32 kernel and the float64 reference."""
    x = draw(shape, torch.float64, seed)
    for v in thresholds:
        v = torch.as_tensor(v, dtype=torch.float64, device=DEV)
        v = v.reshape(tuple(v.shape) + (1,) * (x.dim() - v.dim()))
        near = (x.abs() - v).abs() < 2e-3
        x = torch.where(near, torch.where(x < 0, -(v + 4e-3), v + 4e-3), x)
    return x.to(dtype)


# float32 threshold gradients.  The kernel sums g dT/dv per thread in float32 over at most 4 slots x 4 elements = 16 terms (15
# additions), converts to float64 and stays there (wave shuffles, LDS, per-unit store, second launch).  Each float32 term carries R
# roundings of its own (soft: -sign(x) g, exact, R = 0; garrote: -2 v / x * g, a division and a product, R = 2; firm: two products, a
# difference (hi - v), its square and a division per term, R <= 6), and the float64 sum is rounded once to the float32 threshold dtype.
# Worst case: |error| <= (15 + R + 1) eps32 sum |term|, eps32 = 2^-24 the unit roundoff; the float64 part adds ~1e-13 relative.
TERMS_PER_PARTIAL = 16
TERM_ROUNDINGS = {"soft": 0, "garrote": 2, "firm": 6}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("mode", ["soft", "garrote", "firm"])
@pytest.mark.parametrize("form", ["one", "per_level", "leading"])
def test_gradients(dtype, mode, form):
    shapes = [(2, 3, 5), (2, 3, 67), (2, 4099)]  # the tensors of a container: shared leading axes
    if form == "one":
        lo = [torch.tensor([1.25], dtype=dtype, device=DEV)] * 3
        hi = [torch.tensor(2.5, dtype=dtype, device=DEV)] * 3
    elif form == "per_level":
        lo = [torch.tensor([1.0 + 0.25 * i], dtype=dtype, device=DEV) for i in range(3)]
        hi = [torch.tensor([2.0 + 0.5 * i], dtype=dtype, device=DEV) for i in range(3)]
    else:
        lo = [torch.tensor([1.0, 1.5], dtype=dtype, device=DEV)] * 3
        hi = [torch.tensor([2.0, 3.0], dtype=dtype, device=DEV)] * 3
    xs = [pushed(s, dtype, 40 + i, (lo[i], hi[i]) if mode == "firm" else (lo[i],)) for i, s in enumerate(shapes)]
    distinct = []
    for v in lo + (hi if mode == "firm" else []):
        if not any(v is u for u in distinct):
            distinct.append(v)

    def grads(fn, xs_, lo_, hi_):
        out = fn(xs_, lo_, hi_) if mode == "firm" else fn(xs_, lo_, mode)
        return torch.autograd.grad(loss_of(out), xs_ + [v for v in dict.fromkeys(lo_ + (hi_ if mode == "firm" else []))])

    def fresh(ts, to=None):
        memo = {}
        return [memo.setdefault(id(t), t.detach().to(to or t.dtype).requires_grad_(True)) for t in ts]

    fn, ref_fn = (ptwt_amd.threshold_firm, R.threshold_firm) if mode == "firm" else (ptwt_amd.threshold, R.threshold)
    _engine.level_events = []
    try:
        got = grads(fn, fresh(xs), fresh(lo), fresh(hi))
        tags = [e[0] for e in _engine.level_events]
    finally:
        _engine.level_events = None
    assert tags == ["thresh_fwd", "thresh_bwd"]  # one launch each way for the container
    want = grads(ref_fn, fresh(xs, torch.float64), fresh(lo, torch.float64), fresh(hi, torch.float64))
    assert len(got) == len(want) == 3 + len(distinct)
    if dtype == torch.float64:
        for g_, w_ in zip(got, want):
            assert g_.dtype == torch.float64 and g_.shape == w_.shape
            assert float((g_ - w_).norm()) <= 1e-12 * float(w_.norm()) + 1e-300
        return
    eps32 = EPS[torch.float32]
    for i, (g_, w_) in enumerate(zip(got[:3], want[:3])):  # d/dx: the forward's element-wise bound times |g|
        vmax = (hi if mode == "firm" else lo)[i].double()
        vmax = vmax.reshape(tuple(vmax.shape) + (1,) * (g_.dim() - vmax.dim())) if vmax.numel() > 1 else vmax.reshape(())
        bound = 8 * 2 * eps32 * torch.maximum(xs[i].double().abs(), vmax) * weight(xs[i], i).double().abs()
        assert g_.dtype == torch.float32 and bool(((g_.double() - w_).abs() <= bound).all()), (mode, form, i)
    # d/dvalue: sum |term| per destination from the float64 reference with |g| in place of g and |dT/dv| in place of dT/dv
    comp = grads(lambda d, *a: [T._composed(t, a[0][k], a[1][k] if mode == "firm" else None, T.FIRM if mode == "firm" else T.MODES[mode], 0.0)
                                for k, t in enumerate(d)], fresh(xs), fresh(lo), fresh(hi))
    for k, v in enumerate(distinct):
        users = [i for i in range(3) if lo[i] is v or (mode == "firm" and hi[i] is v)]
        total = torch.zeros(v.numel(), dtype=torch.float64, device=DEV)
        for i in users:
            jac = _abs_terms(xs[i].double(), lo[i].double(), hi[i].double(), mode, hi[i] is v and lo[i] is not v)
            contrib = (jac * weight(xs[i], i).double().abs()).reshape(v.numel() if v.numel() > 1 else 1, -1).sum(1)
            total += contrib
        bound = (TERMS_PER_PARTIAL - 1 + TERM_ROUNDINGS[mode] + 1) * eps32 * total
        err = (got[3 + k].double() - want[3 + k]).abs().reshape(-1)
        err_composed = (comp[3 + k].double() - want[3 + k]).abs().reshape(-1)
        print(f"threshold gradient {mode} {form} #{k}: kernel error {float(err.max()):.3e}, composed float32 route {float(err_composed.max()):.3e}, "
              f"bound {float(bound.min()):.3e}, sum|terms| {float(total.max()):.3e}")
        assert got[3 + k].dtype == torch.float32 and got[3 + k].shape == v.shape
        assert bool((err <= bound + 1e-12 * total).all()), (mode, form, k)


def _abs_terms(x, lo, hi, mode, for_hi):
    """|dT/dv| of every element, float64, from the derivatives' closed forms (thresholds broadcast from the left)."""
    def b(v):
        return v.reshape(()) if v.numel() == 1 else v.reshape(tuple(v.shape) + (1,) * (x.dim() - v.dim()))

    m, lo, hi = x.abs(), b(lo), b(hi)
    if mode == "soft":
        return (m > lo).double()
    if mode == "garrote":
        return torch.where(m > lo, 2 * lo / m, torch.zeros_like(m))
    mid = (m > lo) & (m <= hi)
    d = hi - lo
    return torch.where(mid, (lo * (m - lo) if for_hi else hi * (hi - m)) / (d * d), torch.zeros_like(m))


def test_hard_gradient_is_the_keep_mask():
    for dtype in (torch.float32, torch.float64):
        x = pushed((3, 257), dtype, 60, (1.25,)).requires_grad_(True)
        v = torch.tensor([1.25], dtype=dtype, device=DEV, requires_grad=True)
        for mode, mask in (("hard", x.abs() >= 1.25), ("greater", x >= 1.25), ("less", x <= 1.25)):
            gx, gv = torch.autograd.grad(loss_of(ptwt_amd.threshold(x, v, mode, 0.5)), (x, v))
            assert torch.equal(gx, torch.where(mask, weight(x, 0), torch.zeros_like(x)))
            assert gv.shape == v.shape and not gv.any()


@pytest.mark.parametrize("mode", ["soft", "garrote"])
def test_second_derivative_through_the_composed_route(mode):
    x0 = pushed((2, 9), torch.float64, 70, (1.25,))
    res = []
    for fn in (ptwt_amd.threshold, R.threshold):
        x = x0.clone().requires_grad_(True)
        v = torch.tensor([1.25], dtype=torch.float64, device=DEV, requires_grad=True)
        gx, gv = torch.autograd.grad(loss_of(fn(x, v, mode)), (x, v), create_graph=True)
        s = (gx * weight(gx, 11)).sum() + 0.7 * gv.sum()
        second = torch.autograd.grad(s, (x, v), allow_unused=True)
        res.append([gx.detach(), gv.detach()] + [torch.zeros_like(t) if g is None else g for g, t in zip(second, (x, v))])
    for g_, w_ in zip(*res):  # (soft's second derivative is zero: the scale of the comparison is that of the first, O(1))
        assert float((g_ - w_).norm()) <= 1e-12 * max(float(w_.norm()), 1.0)
    if mode == "garrote":
        assert float(res[1][2].norm()) > 0 and float(res[1][3].norm()) > 0


def test_complex_data_that_requires_grad_runs_composed():
    x = draw((2, 33), torch.complex128, 80).requires_grad_(True)
    v = torch.tensor([1.25], dtype=torch.float64, device=DEV, requires_grad=True)
    before = _engine.launch_count(48)
    got = torch.autograd.grad(ptwt_amd.threshold(x, v, "soft").abs().sum(), (x, v))
    want = torch.autograd.grad(R.threshold(x, v, "soft").abs().sum(), (x, v))
    assert _engine.launch_count(48) == before
    for g_, w_ in zip(got, want):
        assert float((g_ - w_).abs().max()) <= 1e-12 * float(w_.abs().max())


# ---- capture ------------------------------------------------------------------------------------------------------------------------
def test_capture_reads_the_threshold_at_replay_time():
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(2, 17, 19, generator=g) * 2).to(DEV)
    v = torch.tensor([0.5], device=DEV)

    def fn(t):
        return ptwt_amd.threshold(ptwt_amd.wavedec2(t, "db2", level=2), v, "soft")

    cap = ptwt_amd.capture(fn, x)
    first = [t.clone() for t in R.leaves(cap(x))]
    assert all(torch.equal(a, b) for a, b in zip(first, R.leaves(fn(x))))
    v.fill_(1.5)  # in place: the replay reads the tensor on the device
    second = [t.clone() for t in R.leaves(cap(x))]
    assert all(torch.equal(a, b) for a, b in zip(second, R.leaves(fn(x))))
    assert any(not torch.equal(a, b) for a, b in zip(first, second))
