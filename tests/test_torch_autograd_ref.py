"""CPU tests of the differentiable float64 reference (oracle/torch_autograd_ref.py) that judges the learnable-filter-bank kernels in
tests/test_gpu_learnable_lengths.py.  Before it may judge anything it is pinned here against what the reference library itself
produced — the values of tests/golden/ptwt_ref.npz, the data gradients of ptwt_ref_grads.npz, the tap gradients of
ptwt_ref_tapgrads.npz and the second-order tap derivatives of ptwt_ref_tapgrads2.npz (level transforms only; fp64 1e-12 norm-wise, the
second order 1e-11) — and against the independent numpy oracle (oracle/fwt_oracle.py) at long and odd filter lengths, with random
four-filter banks, in all five modes.  Its stationary transform (``swt`` / ``iswt``) is pinned against every case of
ptwt_ref_swt.npz and the swt cases of both tap-gradient goldens, and the numpy level stand-ins of tests/_oracle_engine.py
(``swt_level_fwd`` / ``swt_level_inv``: the float64 oracle of single level calls in tests/test_gpu_swt_kernels.py) against it."""
import numpy as np
import pytest
import torch

from oracle import fwt_oracle as O
from oracle import torch_autograd_ref as R
from tests import _golden as G

MODES = ("zero", "constant", "reflect", "periodic", "symmetric")
TAPS = ("dec_lo", "dec_hi", "rec_lo", "rec_hi")


def weight(t, i):
    return torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64) + i).reshape(t.shape).to(t.dtype)


def weight2(t, i):
    return torch.cos(0.53 * torch.arange(t.numel(), dtype=torch.float64) + i).reshape(t.shape).to(t.dtype)


def flat(coeffs):
    return [t for _, t in G.flatten_coeffs(coeffs)]


def rebuild(coeffs, leaves):
    it = iter(leaves)
    out = [next(it)]
    for c in coeffs[1:]:
        if isinstance(c, torch.Tensor):
            out.append(next(it))
        elif isinstance(c, dict):
            out.append({k: next(it) for k in c})
        else:
            out.append(tuple(next(it) for _ in c))
    return out if isinstance(coeffs, list) else tuple(out)


def _kw(case):
    return {a: (tuple(v) if isinstance(v, list) else v) for a, v in case["kw"].items()}


def _rkw(kw):
    return {a: v for a, v in kw.items() if a in ("axis", "axes")}


def _taps(wavelet):
    return [t.clone().requires_grad_(True) for t in R.bank_of(wavelet)]


def test_values_vs_reference_goldens():
    z, idx = G.load("ptwt_ref.npz")
    for case in idx:
        k, kw = case["key"], _kw(case)
        x = torch.from_numpy(z[k + "_x"])
        tol = 1e-12 if x.dtype == torch.float64 else 1e-6  # (float32 cases: the reference ran in float32, and so does this)
        coeffs = getattr(R, case["fn"])(x, case["wavelet"], **kw)
        got = G.flatten_coeffs(coeffs)
        assert [n for n, _ in got] == case["names"], case
        for name, t in got:
            assert t.dtype == x.dtype
            assert G.relerr(t.numpy(), z["%s_%s" % (k, name)]) < tol, (case, name)
        y = getattr(R, case["rec"])(coeffs, case["wavelet"], **_rkw(kw))
        assert G.relerr(y.numpy(), z[k + "_rec"]) < tol, (case, "rec")


def test_data_gradients_vs_reference_goldens():
    z, idx = G.load("ptwt_ref_grads.npz")
    for case in idx:
        k, kw = case["key"], _kw(case)
        x = torch.from_numpy(z[k + "_x"]).requires_grad_(True)
        coeffs = getattr(R, case["fn"])(x, case["wavelet"], **kw)
        fl = flat(coeffs)
        assert len(fl) == case["ncoef"]
        (gx,) = torch.autograd.grad(sum((weight(t, i) * t).sum() for i, t in enumerate(fl)), x)
        assert G.relerr(gx.numpy(), z[k + "_gx"]) < 1e-12, (case, "analysis")
        leaves = [t.detach().clone().requires_grad_(True) for t in fl]
        y = getattr(R, case["rec"])(rebuild(coeffs, leaves), case["wavelet"], **_rkw(kw))
        for i, g in enumerate(torch.autograd.grad((weight(y, 7) * y).sum(), leaves)):
            assert G.relerr(g.numpy(), z["%s_gc%d" % (k, i)]) < 1e-12, (case, "synthesis", i)


def test_tap_gradients_vs_reference_goldens():
    z, idx = G.load("ptwt_ref_tapgrads.npz")
    cases = [c for c in idx if not c["fn"].startswith("packet")]
    assert len(cases) == 41 and sum(c["fn"] == "swt" for c in cases) == 3
    for case in cases:
        k, kw = case["key"], _kw(case)
        x = torch.from_numpy(z[k + "_x"])
        taps = _taps(case["wavelet"])
        coeffs = getattr(R, case["fn"])(x, tuple(taps), **kw)
        loss = sum((weight(t, i) * t).sum() for i, t in enumerate(flat(coeffs)))
        g_dec = torch.autograd.grad(loss, taps[:2], retain_graph=True)
        assert G.relerr(g_dec[0].numpy(), z[k + "_gdec_lo"]) < 1e-12, (case, "dec_lo")
        assert G.relerr(g_dec[1].numpy(), z[k + "_gdec_hi"]) < 1e-12, (case, "dec_hi")
        y = getattr(R, case["rec"])(coeffs, tuple(taps), **_rkw(kw))
        for nme, g in zip(TAPS, torch.autograd.grad((weight(y, 7) * y).sum(), taps)):
            assert G.relerr(g.numpy(), z["%s_gall_%s" % (k, nme)]) < 1e-12, (case, nme)


def test_second_order_tap_derivatives_vs_reference_goldens():
    z, idx = G.load("ptwt_ref_tapgrads2.npz")
    cases = [c for c in idx if not c["fn"].startswith("packet")]
    assert cases and sum(c["fn"] == "swt" for c in cases) == 3
    for case in cases:
        k, kw = case["key"], _kw(case)
        x = torch.from_numpy(z[k + "_x"]).requires_grad_(True)
        taps = _taps(case["wavelet"])
        fl = flat(getattr(R, case["fn"])(x, tuple(taps), **kw))
        f = sum((weight(t, i) * t.square()).sum() for i, t in enumerate(fl)) / 2
        g_x, t_lo, t_hi = torch.autograd.grad(f, [x, taps[0], taps[1]], create_graph=True)
        s1 = (g_x * weight2(g_x, 1)).sum() + (t_lo * weight2(t_lo, 2)).sum() + (t_hi * weight2(t_hi, 3)).sum()
        for got, nme in zip(torch.autograd.grad(s1, [x, taps[0], taps[1]]), ("a_dx", "a_dlo", "a_dhi")):
            assert G.relerr(got.numpy(), z["%s_%s" % (k, nme)]) < 1e-11, (case, nme)
        coeffs = getattr(R, case["fn"])(x.detach(), case["wavelet"], **kw)
        leaves = [t.detach().clone().requires_grad_(True) for t in flat(coeffs)]
        y = getattr(R, case["rec"])(rebuild(coeffs, leaves), tuple(taps), **_rkw(kw))
        grads = torch.autograd.grad((weight(y, 7) * y.square()).sum() / 2, leaves + taps[2:], create_graph=True)
        s2 = sum((gc * weight2(gc, 4 + i)).sum() for i, gc in enumerate(grads[:-2]))
        s2 = s2 + (grads[-2] * weight2(grads[-2], 2)).sum() + (grads[-1] * weight2(grads[-1], 3)).sum()
        d2 = torch.autograd.grad(s2, leaves + taps[2:])
        for i, got in enumerate(d2[:-2]):
            assert G.relerr(got.numpy(), z["%s_s_dc%d" % (k, i)]) < 1e-11, (case, "s_dc", i)
        assert G.relerr(d2[-2].numpy(), z[k + "_s_dlo"]) < 1e-11, (case, "s_dlo")
        assert G.relerr(d2[-1].numpy(), z[k + "_s_dhi"]) < 1e-11, (case, "s_dhi")


def test_swt_vs_reference_goldens():
    """Every case of ptwt_ref_swt.npz (incl. axis=1, the 1-D input, windows that wrap more than once, 22 - 102 taps): coefficients,
    reconstruction and both data gradients, at the bounds of tests/test_gpu_swt.py."""
    z, idx = G.load("ptwt_ref_swt.npz")
    assert len(idx) == 28 and any(c["kw"] for c in idx) and any(len(c["shape"]) == 1 for c in idx)
    for case in idx:
        k = case["key"]
        x = torch.from_numpy(z[k + "_x"]).requires_grad_(True)
        c = R.swt(x, case["wavelet"], case["level"], **case["kw"])
        assert len(c) == case["ncoef"]
        for i, t in enumerate(c):
            want = z["%s_c%d" % (k, i)]
            assert tuple(t.shape) == want.shape and t.dtype == torch.float64
            assert G.relerr(t.detach().numpy(), want) < 1e-12, (case, i)
        (gx,) = torch.autograd.grad(sum((weight(t, i) * t).sum() for i, t in enumerate(c)), x)
        assert G.relerr(gx.numpy(), z[k + "_gx"]) < 1e-11, (case, "swt backward")
        leaves = [t.detach().clone().requires_grad_(True) for t in c]
        y = R.iswt(leaves, case["wavelet"], **case["kw"])
        assert G.relerr(y.detach().numpy(), z[k + "_rec"]) < 1e-12, (case, "iswt")
        for i, g in enumerate(torch.autograd.grad((weight(y, 7) * y).sum(), leaves)):
            assert G.relerr(g.numpy(), z["%s_gc%d" % (k, i)]) < 1e-11, (case, "iswt backward", i)


def random_bank(flen, seed):
    """Four independent filters (no orthogonality relation between them: a kernel that reads the wrong filter of a pair shows)."""
    g = np.random.default_rng(seed)
    return tuple(g.standard_normal(flen) / np.sqrt(flen) for _ in range(4))


# extents keep every level's padding within what torch's reflect / circular pads accept, and odd filter lengths run one level (a second
# one would need the reference's adjust_trim to hold)
@pytest.mark.parametrize("flen", [22, 32, 40, 3, 5, 21, 33])
@pytest.mark.parametrize("mode", MODES)
def test_forward_and_reconstruction_vs_numpy_oracle(flen, mode):
    bank = random_bank(flen, flen)
    tbank = tuple(torch.from_numpy(f) for f in bank)
    rng = np.random.default_rng(100 + flen)
    level = 2 if flen % 2 == 0 else 1
    n = 2 * flen + 9
    cases = [("wavedec", "waverec", (3, 2 * n + 1), {}), ("wavedec2", "waverec2", (2, n, n + 4), {}),
             ("fswavedec2", "fswaverec2", (2, n + 1, n), {})]
    if flen <= 22:
        cases.append(("fswavedec3", "fswaverec3", (1, flen + 3, flen + 2, flen + 4), {"level": 1}))
    if flen <= 5:
        cases.append(("wavedec3", "waverec3", (2, n, n + 1, n + 2), {}))
    for fn, rec, shape, extra in cases:
        x = rng.standard_normal(shape)
        kw = {"mode": mode, "level": level, **extra}
        got = getattr(R, fn)(torch.from_numpy(x), tbank, **kw)
        want = getattr(O, fn)(x, bank, **kw)
        gf, wf = G.flatten_coeffs(got), G.flatten_coeffs(want)
        assert [a for a, _ in gf] == [a for a, _ in wf], fn
        for (name, g), (_, w) in zip(gf, wf):
            assert g.shape == w.shape and G.relerr(g.numpy(), w) < 1e-12, (fn, mode, flen, name)
        y = getattr(R, rec)(got, tbank)
        assert G.relerr(y.numpy(), getattr(O, rec)(want, bank)) < 1e-12, (rec, mode, flen)


def test_odd_filter_lengths_follow_the_general_pad_arithmetic():
    """With an odd filter length the reference's pad amounts give (n + n % 2 + L - 2) // 2 coefficients — one fewer than
    (n + L - 1) // 2 on even extents — and a reconstruction of 2 m - L + 2 samples."""
    for flen in (3, 5, 21, 33):
        bank = tuple(torch.from_numpy(f) for f in random_bank(flen, 7))
        for n in (40, 41):
            c = R.wavedec(torch.zeros(1, n, dtype=torch.float64), bank, mode="zero", level=1)
            assert c[0].shape[-1] == (n + n % 2 + flen - 2) // 2
            assert R.waverec(c, bank).shape[-1] == 2 * c[0].shape[-1] - flen + 2


@pytest.mark.parametrize("flen", [14, 20])
def test_3d_per_axis_form_equals_dense_form(flen):
    """The per-axis 3-D levels (long filters) against the dense conv3d of the reference's op sequence: values, data and tap gradients."""
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((2, flen + 3, flen + 2, flen + 5)))
    outs = []
    for dense_max in (flen, flen - 1):
        R.DENSE_3D_MAX_TAPS, saved = dense_max, R.DENSE_3D_MAX_TAPS
        try:
            xl = x.clone().requires_grad_(True)
            taps = [torch.from_numpy(f).requires_grad_(True) for f in random_bank(flen, 3)]
            c = R.wavedec3(xl, tuple(taps), mode="symmetric", level=1)
            y = R.waverec3(c, tuple(taps))
            loss = sum((weight(t, i) * t).sum() for i, t in enumerate(flat(c))) + (weight(y, 7) * y).sum()
            outs.append([*flat(c), y, *torch.autograd.grad(loss, [xl, *taps])])
        finally:
            R.DENSE_3D_MAX_TAPS = saved
    for a, b in zip(*outs):
        assert G.relerr(a.detach().numpy(), b.detach().numpy()) < 1e-12


# (N, L, D): odd extents, rows shorter than one tap step, D L > 2 N (windows that wrap several times), D L/2 a multiple of N
STANDIN_CELLS = [(1, 4, 2), (3, 8, 1), (5, 2, 3), (24, 16, 4), (37, 6, 2), (41, 22, 8), (257, 10, 64), (48, 12, 8), (1001, 34, 3)]


@pytest.mark.parametrize("n,flen,dilation", STANDIN_CELLS)
@pytest.mark.parametrize("scale", [1.0, 0.5, float(np.pi / 7)])
def test_numpy_level_stand_ins_vs_reference(n, flen, dilation, scale):
    """``swt_level_fwd`` / ``swt_level_inv`` (tests/_oracle_engine.py) against one level of the reference with four independent random
    filters: what makes them a legitimate float64 oracle for single level calls on the GPU tier (any dilation, any scale)."""
    from tests import _oracle_engine as oe

    bank = random_bank(flen, 3 * n + flen)
    tb = [torch.from_numpy(f) for f in bank]
    g = torch.Generator().manual_seed(n + dilation)
    x, a, d = (torch.randn(3, n, generator=g, dtype=torch.float64) for _ in range(3))
    lo, hi = R.swt_level(x, tb[0], tb[1], dilation)
    got = oe.swt_level_fwd(x, list(bank[0]), list(bank[1]), dilation, scale)
    assert got.dtype == torch.float64 and got.shape == (3, 2, n)
    assert G.relerr(got[:, 0].numpy(), scale * lo.numpy()) < 1e-13 and G.relerr(got[:, 1].numpy(), scale * hi.numpy()) < 1e-13
    y = R.iswt_level(a, d, tb[2], tb[3], dilation)  # (the reference's level carries the mean of the pair: scale 1/2)
    got = oe.swt_level_inv(a, d, list(bank[2]), list(bank[3]), dilation, scale)
    assert got.shape == (3, n) and G.relerr(got.numpy(), 2 * scale * y.numpy()) < 1e-13
