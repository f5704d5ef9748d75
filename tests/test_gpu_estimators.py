"""estimate_sigma / estimate_thresholds / shrink on the GPU (kernel ids 50 .. 53, csrc/mifwt_estim.hip) against the float64 numpy
reference of tests/_estimator_ref.py.

Order statistics are compared bit by bit with ``np.sort(np.abs(x))``; sigma within one ulp of the data's type of the float64 value (the
kernel rounds its float64 quotient once; the reference's own last bit is the second half ulp).  Sums of squares: relative error at most
``n 2^-53``, the serial float64 bound for ``n`` terms.  Thresholds: ``4 eps + 2 kappa n 2^-53`` relative, ``eps`` the spacing of the
data's type (the final rounding, and the rounding of a sigma that arrives in that type, each amplified at most twice by the square) and
``kappa = mean(d^2) / |mean(d^2) - sigma^2|`` the condition of BayesShrink's difference; bands built with ``mean(d^2) < sigma^2
(1 - 1e-3)`` must take the clamp.  Every allocation a kernel writes is carved out of canary bytes (tests/test_gpu_canaries.py)."""
import math

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, estimators as E, thresholding as T
from ptwt_amd.constants import WaveletDetailTuple2d
from tests import _estimator_ref as R
from tests.test_gpu_canaries import _GuardedTorch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NP = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
ROUTES = pytest.mark.parametrize("route", ["lds", "stream"])
U = 2.0 ** -53


@pytest.fixture()
def canaries(monkeypatch):
    g = _GuardedTorch()
    for mod in (E, T, _engine):
        monkeypatch.setattr(mod, "torch", g)
    yield g
    g.check("estimators")


@pytest.fixture()
def events():
    _engine.level_events = []
    try:
        yield _engine.level_events
    finally:
        _engine.level_events = None


def force(monkeypatch, route):
    monkeypatch.setattr(E, "FORCE_STREAM", route == "stream")
    return 51 if route == "stream" else 50


def to_np(obj):
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu().numpy()
    if obj is None:
        return None
    if isinstance(obj, dict):
        return {k: to_np(v) for k, v in obj.items()}
    if isinstance(obj, tuple) and hasattr(obj, "_fields"):
        return type(obj)(*[to_np(v) for v in obj])
    return type(obj)(to_np(v) for v in obj)


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def within_ulp(got, ref64, what=""):
    """``got`` (the data's type) within one ulp of the float64 reference; infinities and NaNs must agree."""
    got64 = got.astype(np.float64)
    fin = np.isfinite(ref64)
    assert np.array_equal(got64[~fin], ref64[~fin], equal_nan=True), what
    ulp = np.spacing(np.abs(ref64[fin]).astype(got.dtype)).astype(np.float64)
    err = np.abs(got64[fin] - ref64[fin])
    assert bool((err <= ulp).all()), f"{what}: {float((err / ulp).max()):.3g} ulp"


def check_selection(x, lead, kid, events, what):
    """Order statistics of the device tensor ``x`` bit-equal to a sort, sigma within an ulp, on the route ``kid``."""
    xn = x.cpu().numpy()
    del events[:]
    stats = E._order_stats(x, lead).cpu().numpy()
    sigma = ptwt_amd.estimate_sigma(x, lead=lead)
    assert [e[:2] for e in events] == [("estim_sigma", kid)] * 2, (what, [e[:2] for e in events])
    assert same_bits(stats, R.order_stats(xn, lead)), what
    assert sigma.dtype == x.dtype and sigma.shape == x.shape[:lead] and sigma.device == x.device and not sigma.requires_grad
    within_ulp(sigma.cpu().numpy(), R.estimate_sigma(xn, lead), what)
    return stats, sigma


# ---- order statistics ---------------------------------------------------------------------------------------------------------------
@DTYPES
@ROUTES
def test_order_statistics_counts_and_adversarial_inputs(dtype, route, monkeypatch, canaries, events):
    kid = force(monkeypatch, route)
    cap = E.lds_capacity(dtype)
    counts = [1, 2, 3, 63, 64, 65, cap - 1, cap] + ([cap + 1] if route == "stream" else [])
    for count in counts:
        cases = R.adversarial(NP[dtype], count, seed=count)
        x = torch.from_numpy(np.stack(list(cases.values()))).to(DEV)  # one image per input kind
        check_selection(x, 1, kid, events, f"{route} count={count}")
    # one element per leading index, and a single image (lead 0) that starts one element past a 16-byte boundary
    flat = torch.from_numpy(R.adversarial(NP[dtype], 131, seed=7)["random"]).to(DEV)
    check_selection(flat, 1, kid, events, "lead == dim")
    check_selection(flat[1:130], 0, kid, events, "misaligned")


@DTYPES
def test_capacity_plus_one_takes_the_streaming_route(dtype, canaries, events):
    cap = E.lds_capacity(dtype)
    for count, kid in ((cap, 50), (cap + 1, 51)):
        cases = R.adversarial(NP[dtype], count, seed=3)
        x = torch.from_numpy(np.stack([cases["random"], cases["low_bits"]])).to(DEV)
        check_selection(x, 1, kid, events, f"count={count}")


@DTYPES
def test_streaming_batch_permutes_and_repeats(dtype, canaries, events):
    rng = np.random.default_rng(5)
    count = 70001
    imgs = [rng.standard_normal(count) * 0.01, rng.standard_cauchy(count) * 300.0, np.abs(rng.standard_normal(count)) + 1e6]
    x = torch.from_numpy(np.stack(imgs).astype(NP[dtype])).to(DEV)
    stats, sigma = check_selection(x, 1, 51, events, "3 x 70001")
    perm = [2, 0, 1]
    stats_p, sigma_p = check_selection(x[perm].contiguous(), 1, 51, events, "permuted")
    assert same_bits(stats_p, stats[perm]) and torch.equal(sigma_p, sigma[perm])
    again = E._order_stats(x, 1).cpu().numpy()
    assert same_bits(again, stats) and torch.equal(ptwt_amd.estimate_sigma(x, lead=1), sigma)  # two runs: the same bits
    # an even count, two leading axes
    y = x[:, :70000].reshape(3, 2, 35000)
    check_selection(y, 2, 51, events, "3 x 2 x 35000")


@DTYPES
@ROUTES
def test_strided_bands_of_the_transforms(dtype, route, monkeypatch, canaries, events):
    kid = force(monkeypatch, route)
    g = torch.Generator().manual_seed(2)
    c2 = ptwt_amd.wavedec2(torch.randn(3, 37, 70, generator=g, dtype=dtype).to(DEV), "db2", level=2)
    c3 = ptwt_amd.wavedec3(torch.randn(2, 12, 13, 18, generator=g, dtype=dtype).to(DEV), "haar", level=1)
    c1 = ptwt_amd.wavedec(torch.randn(5, 203, generator=g, dtype=dtype).to(DEV), "db3", level=3)
    bands = [b for lev in c2[1:] for b in lev] + list(c3[1].values()) + list(c1[1:])
    assert any(not b.is_contiguous() for b in bands)
    for b in bands:
        check_selection(b, 1, kid, events, f"band {tuple(b.shape)} strides {b.stride()}")
    for c, axes in ((c2, 2), (c3, 3), (c1, 1)):  # the container forms: the finest all-high band, lead inferred
        d, ax = R.finest(to_np(c))
        assert ax == axes
        got = ptwt_amd.estimate_sigma(c)
        assert got.shape == d.shape[: d.ndim - axes]
        within_ulp(got.cpu().numpy(), R.estimate_sigma(to_np(c)), f"container {axes}-D")
    assert {e[1] for e in events} == {kid}


def test_empty_inputs_launch_nothing(events):
    e0 = torch.empty((0, 5), device=DEV)
    assert ptwt_amd.estimate_sigma(e0, lead=1).shape == (0,)
    s = ptwt_amd.estimate_sigma(torch.empty((3, 0), device=DEV), lead=1)
    assert s.shape == (3,) and bool(torch.isnan(s).all())
    coeffs = [torch.empty((0, 4), device=DEV), torch.empty((0, 4), device=DEV), torch.empty((0, 7), device=DEV)]
    for method in ("visu", "bayes"):
        thr = ptwt_amd.estimate_thresholds(coeffs, method)
        assert thr[0] is None and thr[1].shape == (0,) and thr[2].shape == (0,)
        out = ptwt_amd.shrink(coeffs, method)
        assert out[0] is coeffs[0] and out[1].shape == (0, 4) and out[2].shape == (0, 7)
    assert events == []


# ---- moments ------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_band_moments(dtype, canaries, events):
    g = torch.Generator().manual_seed(4)
    c2 = ptwt_amd.wavedec2((torch.randn(3, 45, 83, generator=g, dtype=dtype) * 3).to(DEV), "db3", level=3)
    big = [torch.zeros(2, 4, device=DEV, dtype=dtype), (torch.randn(2, 301, 303, generator=g, dtype=dtype) * 50).to(DEV)[:, :, 1:],
           (torch.randn(2, 1, generator=g, dtype=dtype)).to(DEV), (torch.randn(2, 9001, generator=g, dtype=dtype) + 7).to(DEV)]
    for coeffs in (c2, big):
        del events[:]
        got = R.leaves(to_np(E._band_moments(coeffs))[1:])
        assert [e[:2] for e in events] == [("estim_bayes", 52)]  # one launch for the container
        details = R.leaves(to_np(coeffs)[1:])
        lead = 1
        for m, t in zip(got, details):
            want = R.moments(t, lead)
            n = t.size // want.size
            assert m.dtype == np.float64 and m.shape == want.shape
            rel = np.abs(m - want) / want
            assert bool((rel <= n * U).all()), (t.shape, float(rel.max() / (n * U)))


def test_more_bands_than_one_launch_holds(canaries, events):
    g = torch.Generator().manual_seed(6)
    k = E.max_segments() + 3
    coeffs = [torch.zeros(2, 3, device=DEV)] + [(torch.randn(2, 5 + i, generator=g) * (i + 1)).to(DEV) for i in range(k)]
    thr = ptwt_amd.estimate_thresholds(coeffs, "bayes", sigma=0.5)
    assert [e[:2] for e in events] == [("estim_bayes", 52)] * 2
    ref = R.estimate_thresholds(to_np(coeffs), "bayes", sigma=0.5)
    for i in range(1, k + 1):
        assert np.allclose(thr[i].cpu().numpy(), ref[i], rtol=1e-6, atol=0), i


# ---- thresholds -----------------------------------------------------------------------------------------------------------------------
def threshold_tolerance(t, lead, sigma, eps):
    """Per leading index: (whether the band takes the clamp, the relative tolerance of its BayesShrink threshold)."""
    n = int(np.prod(t.shape[lead:]))
    m2 = R.moments(t, lead) / n
    clamp = m2 < np.asarray(sigma) ** 2 * (1 - 1e-3)
    kappa = R.kappa(t, lead, sigma)
    assert bool((clamp | (kappa <= 100)).all()), "a band of the test is neither clamped nor well conditioned"
    return clamp, np.where(clamp, 4 * eps, 4 * eps + 2 * kappa * n * U)


def check_thresholds(thr, coeffs, sigma_ref, dtype, what):
    eps = float(torch.finfo(dtype).eps)
    cn = to_np(coeffs)
    ref = R.estimate_thresholds(cn, "bayes", sigma=sigma_ref)
    d, axes = R.finest(cn)
    lead = d.ndim - axes
    assert thr[0] is None
    clamped = 0
    for got, want, t in zip(R.leaves(to_np(thr)[1:]), R.leaves(ref[1:]), R.leaves(cn[1:])):
        assert got.dtype == NP[dtype] and got.shape == t.shape[:lead]
        clamp, tol = threshold_tolerance(t, lead, sigma_ref, eps)
        clamped += int(clamp.sum())
        rel = np.abs(got.astype(np.float64) - want) / want
        assert bool((rel <= tol).all()), f"{what} {t.shape}: {float((rel / tol).max()):.3g} x the tolerance"
        if clamp.any():  # the clamp itself: sigma^2 / sqrt(eps)
            assert bool((np.abs(got[clamp] - (np.asarray(sigma_ref)[clamp] ** 2 / math.sqrt(eps))) <= 4 * eps * want[clamp]).all())
    return clamped


@DTYPES
@pytest.mark.parametrize("form", ["number", "tensor"])
def test_thresholds_with_sigma_given(dtype, form, canaries, events):
    g = torch.Generator().manual_seed(8)
    sig = np.array([0.75, 3.0]) if form == "tensor" else np.array([1.5, 1.5])
    s = torch.from_numpy(sig).reshape(2, 1, 1)

    def band(k, shape):  # a band of standard deviation k sigma per image
        return (torch.randn(shape, generator=g, dtype=torch.float64) * k * s).to(dtype).to(DEV)

    levels = [WaveletDetailTuple2d(band(0.5, (2, 33, 35)), band(2.0, (2, 33, 35)), band(5.0, (2, 33, 35))),
              WaveletDetailTuple2d(band(5.0, (2, 64, 67)), band(0.5, (2, 64, 67)), band(2.0, (2, 64, 67)))]
    coeffs = [band(9.0, (2, 33, 35))] + levels
    sigma = torch.from_numpy(sig).to(dtype).to(DEV) if form == "tensor" else 1.5
    thr = ptwt_amd.estimate_thresholds(coeffs, "bayes", sigma)
    assert [e[:2] for e in events] == [("estim_bayes", 52)]
    assert isinstance(thr[1], WaveletDetailTuple2d) and isinstance(thr[2], WaveletDetailTuple2d)
    assert check_thresholds(thr, coeffs, sig, dtype, f"bayes {form}") == 4  # the two 0.5 sigma bands of both images
    # visu: one factor for every detail tensor, n over the whole container or given
    for n in (None, 4096):
        del events[:]
        thr = ptwt_amd.estimate_thresholds(coeffs, "visu", sigma, n=n)
        assert [e[:2] for e in events] == [("estim_visu", 53)]
        ref = R.estimate_thresholds(to_np(coeffs), "visu", sigma=sig, n=n)
        for got, want in zip(R.leaves(to_np(thr)[1:]), R.leaves(ref[1:])):
            assert got.dtype == NP[dtype] and bool((np.abs(got - want) <= 4 * float(torch.finfo(dtype).eps) * want).all())


def noisy_image(dtype, seed=9, shape=(3, 96, 100), noise=(0.5, 1.0, 4.0)):
    """Sparse spikes under Gaussian noise of another level per image: the median sees the noise, the second moments see the spikes."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float64) * torch.tensor(noise, dtype=torch.float64).reshape(-1, 1, 1)
    spikes = (torch.rand(shape, generator=g) < 0.04).double() * torch.randn(shape, generator=g, dtype=torch.float64) * 200.0
    return (x + spikes * torch.tensor(noise, dtype=torch.float64).reshape(-1, 1, 1)).to(dtype).to(DEV)


@DTYPES
def test_thresholds_end_to_end_with_sigma_estimated(dtype, canaries, events):
    coeffs = ptwt_amd.wavedec2(noisy_image(dtype), "db2", level=2)
    del events[:]
    thr = ptwt_amd.estimate_thresholds(coeffs)  # bayes, sigma from the finest diagonal band
    assert [e[:2] for e in events] == [("estim_sigma", 50), ("estim_bayes", 52)]
    sigma_ref = R.estimate_sigma(to_np(coeffs))
    check_thresholds(thr, coeffs, sigma_ref, dtype, "end to end")
    given = ptwt_amd.estimate_thresholds(coeffs, "bayes", ptwt_amd.estimate_sigma(coeffs))
    for a, b in zip(R.leaves(to_np(thr)[1:]), R.leaves(to_np(given)[1:])):
        assert same_bits(a, b)  # sigma=None is estimate_sigma


# ---- shrink ---------------------------------------------------------------------------------------------------------------------------
def containers(dtype):
    x = noisy_image(dtype, seed=10, shape=(2, 40, 52), noise=(1.0, 2.0))
    return {"wavedec2": ptwt_amd.wavedec2(x, "db2", level=2),
            "wavedec": ptwt_amd.wavedec(x.reshape(2, -1), "db3", level=3),
            "wavedec3": ptwt_amd.wavedec3(x.reshape(2, 8, 10, 26), "haar", level=1),
            "fswavedec2": ptwt_amd.fswavedec2(x, "db2", level=2)}


@DTYPES
@pytest.mark.parametrize("mode", ["soft", "hard", "garrote", "firm"])
def test_shrink_is_the_threshold_launch_on_the_estimated_thresholds(dtype, mode, canaries, events):
    eps = float(torch.finfo(dtype).eps)
    for name, coeffs in containers(dtype).items():
        for method in ("bayes", "visu"):
            del events[:]
            got = ptwt_amd.shrink(coeffs, method, mode)
            tags = [e[:2] for e in events]
            assert tags == [("estim_sigma", 50), ("estim_bayes", 52) if method == "bayes" else ("estim_visu", 53), ("thresh_fwd", 48)], tags
            # the same container, the approximation spared
            assert type(got) is type(coeffs) and got[0] is coeffs[0] and len(got) == len(coeffs)
            for a, b in zip(got[1:], coeffs[1:]):
                assert type(a) is type(b) and (not isinstance(b, dict) or list(a) == list(b))
            thr = ptwt_amd.estimate_thresholds(coeffs, method)
            xs, vs, ys = R_leaves(coeffs[1:]), R_leaves(thr[1:]), R_leaves(got[1:])
            assert all(y.shape == x.shape and y.dtype == x.dtype and y.data_ptr() != x.data_ptr() for x, y in zip(xs, ys))
            direct = T._launches(xs, vs, [2 * v for v in vs] if mode == "firm" else None, E._MODES[mode], 0.0)
            assert all(torch.equal(a, b) for a, b in zip(ys, direct)), (name, method)
            if mode in ("soft", "garrote"):  # against float64: the thresholding bound, plus what the threshold's own tolerance moves
                cn = to_np(coeffs)
                sigma_ref = R.estimate_sigma(cn)
                ref = R.shrink(cn, method, mode)
                d, axes = R.finest(cn)
                lead = d.ndim - axes
                for x, v, y, r in zip(R.leaves(cn[1:]), vs, ys, R.leaves(ref[1:])):
                    tol = threshold_tolerance(x, lead, sigma_ref, eps)[1] if method == "bayes" else 4 * eps
                    vb = v.double().cpu().numpy().reshape(v.shape + (1,) * (x.ndim - v.dim()))
                    tb = np.asarray(tol).reshape(vb.shape) if np.ndim(tol) else tol
                    bound = 8 * eps * np.maximum(np.abs(x.astype(np.float64)), vb) + 2 * tb * vb
                    err = np.abs(y.double().cpu().numpy() - r)
                    assert bool((err <= bound).all()), (name, method, float((err / bound).max()))


def R_leaves(obj):
    if isinstance(obj, torch.Tensor):
        return [obj]
    if isinstance(obj, dict):
        return [t for v in obj.values() for t in R_leaves(v)]
    return [t for v in obj for t in R_leaves(v)]


@DTYPES
@pytest.mark.parametrize("mode", ["soft", "hard", "garrote", "firm"])
def test_shrink_data_gradient(dtype, mode, canaries, events):
    from tests import _thresh_ref as TR

    g = torch.Generator().manual_seed(12)
    base = containers(dtype)["wavedec2"]
    xs = [t.detach().clone().requires_grad_(True) for t in R_leaves(base[1:])]
    it = iter(xs)
    coeffs = [base[0]] + [WaveletDetailTuple2d(next(it), next(it), next(it)) for _ in base[1:]]
    ws = [torch.randn(t.shape, generator=g, dtype=torch.float64).to(DEV) for t in xs]
    del events[:]
    out = ptwt_amd.shrink(coeffs, "bayes", mode)
    loss = sum((y.double() * w).sum() for y, w in zip(R_leaves(out[1:]), ws))
    got = torch.autograd.grad(loss, xs)
    assert [e[0] for e in events] == ["estim_sigma", "estim_bayes", "thresh_fwd", "thresh_bwd"]
    thr = [v.double() for v in R_leaves(ptwt_amd.estimate_thresholds(coeffs, "bayes")[1:])]  # constants
    x64 = [t.detach().double().requires_grad_(True) for t in xs]
    if mode == "firm":
        ref_out = [TR._firm(x, v, 2 * v) for x, v in zip(x64, thr)]
    else:
        ref_out = [TR._one(x, v, mode, 0.0) for x, v in zip(x64, thr)]
    want = torch.autograd.grad(sum((y * w).sum() for y, w in zip(ref_out, ws)), x64)
    eps = float(torch.finfo(dtype).eps)
    for x, v, w, g_, w_ in zip(x64, thr, ws, got, want):
        # d/dx is at most 2 (garrote at the threshold, firm's slope v_hi / (v_hi - v_lo)) and a handful of roundings of that
        assert g_.dtype == dtype and bool(((g_.double() - w_).abs() <= 16 * eps * w.abs()).all()), mode
        assert torch.equal(g_ == 0, w_ == 0)


# ---- capture ----------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_captured_pipeline_sees_the_noise_of_the_replayed_data(dtype, monkeypatch):
    """``waverec2(shrink(wavedec2(x)))`` and sigma in one graph, replayed on data with ten times the noise.

    The estimator stage is held to one ulp: the replayed sigma against the float64 reference of the band the replay itself produced,
    and — on coefficients with 19-bit mantissas, whose tenfold is exact — against ten times the reference sigma of the first data.
    Through the transform ``10 x`` does not give ten times the coefficients bit by bit (measured: on spiky data sigma came 2.5 ulp off
    ten times the float32 sigma of ``x``; on this data 0.7 ulp in float32 and exactly 1 ulp in float64): a db4 level-1 coefficient is a sum of 64 products, off by at most ``66 eps (sum |g|)^2 max|x|`` with
    ``(sum |g|)^2 <= 8`` for eight orthonormal taps, and the median moves by no more than its data; that bound, for both runs, is
    what the whole pipeline's tenfold sigma is held to."""
    g = torch.Generator().manual_seed(13)
    x = (torch.randn((2, 64, 72), generator=g, dtype=torch.float64) * torch.tensor([1.0, 2.0], dtype=torch.float64).reshape(2, 1, 1))
    x = x.to(dtype).to(DEV)
    eps = float(torch.finfo(dtype).eps)

    def fn(t):
        coeffs = ptwt_amd.wavedec2(t, "db4", level=3)
        return ptwt_amd.waverec2(ptwt_amd.shrink(coeffs, "bayes", "soft"), "db4"), ptwt_amd.estimate_sigma(coeffs), coeffs[-1].diagonal

    cap = ptwt_amd.capture(fn, x)
    rec1, sigma1, band1 = [t.clone() for t in cap(x)]
    eager = fn(x)
    assert torch.equal(rec1, eager[0]) and torch.equal(sigma1, eager[1])
    ref1 = R.estimate_sigma(band1.cpu().numpy(), lead=1)
    within_ulp(sigma1.cpu().numpy(), ref1, "captured sigma")
    x10 = x * 10
    rec10, sigma10, band10 = [t.clone() for t in cap(x10)]
    eager = fn(x10)
    assert torch.equal(rec10, eager[0]) and torch.equal(sigma10, eager[1])  # the replay ran the estimators on the new data
    within_ulp(sigma10.cpu().numpy(), R.estimate_sigma(band10.cpu().numpy(), lead=1), "replayed sigma against its own band")
    s10 = sigma10.double().cpu().numpy()
    moved = 2 * 66 * eps * 8 * float(x10.abs().max()) / R.MAD_SCALE + np.spacing(sigma10.cpu().numpy()).astype(np.float64)
    print("sigma10 - 10 sigma1 in ulps of sigma10:", (s10 - 10 * ref1) / np.spacing(sigma10.cpu().numpy()), "allowed:", moved)
    assert bool((np.abs(s10 - 10 * ref1) <= moved).all())

    # the estimator stage alone, on coefficients whose tenfold is exact: ten times the noise, ten times sigma, to one ulp — on both
    # routes (the streaming one zeroes its counters on the stream: a memset node of the graph)
    band = (torch.round(band1.double() * 1024).clamp(-2 ** 18, 2 ** 18) / 1024).to(dtype)
    ref = R.estimate_sigma(band.cpu().numpy(), lead=1)
    tenfold = band * 10
    assert torch.equal(tenfold.double(), band.double() * 10)
    for route in ("lds", "stream"):
        kid = force(monkeypatch, route)
        _engine.level_events = []
        try:
            ptwt_amd.estimate_sigma(band, lead=1)
            assert [e[1] for e in _engine.level_events] == [kid]
        finally:
            _engine.level_events = None
        stage = ptwt_amd.capture(lambda t: ptwt_amd.estimate_sigma(t, lead=1), band)
        within_ulp(stage(band).clone().cpu().numpy(), ref, f"stage {route}")
        within_ulp(stage(tenfold).cpu().numpy(), 10 * ref, f"ten times the noise, ten times sigma ({route})")
