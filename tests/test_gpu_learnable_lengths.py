"""GPU tests (``-m gpu``) of learnable filter banks at every filter length against the differentiable float64 CPU reference
(oracle/torch_autograd_ref.py, pinned to the reference library's goldens by tests/test_torch_autograd_ref.py).

Each case is one differentiable call with the four taps as leaf tensors: a forward, a reconstruction and one backward of a
``weight``-style loss; the coefficients, the reconstruction, the gradient w.r.t. the data and the gradients w.r.t. all four filters are
compared with the reference on the same inputs and the same taps (float32 cases: float32 taps, so both sides see the same rounded
values).  Every case runs with device taps (``set_device_taps("auto")``: the kernels read the filters from device memory) and with host
taps (``"never"``); the two agree with each other and with the reference.

Banks: seeded random banks of four INDEPENDENT filters (for a pywt bank rec is dec reversed and hi the alternating flip of lo, so a
kernel that reads the wrong filter of a pair, or ignores the ``rev`` flag of device taps, can still give the expected numbers), and the
pywt banks of the lengths the 2-D tap gradients used to fail at (db11, db13-15, sym16, coif5).  Lengths: every even L from 2 to 32, 34
and 40 (the generic kernels, tap correlation above 32), odd 3, 5, 9, 21, 31 and 33.  The level events of the whole module are recorded
and the last test asserts that the device-tap runs reached every kernel that reads device taps on the legs where it serves, and that the
host-tap 3-D cases reached the 3-D kernels: a matrix that silently falls back to the generic passes fails.

Tolerances: float64 1e-10 norm-wise (the goldens' bound), float32 see F32_TOL; each plus a max-abs bound scaled by the largest
value.
"""
import json
import os

import numpy as np
import pytest
import torch

import ptwt_amd
from oracle import torch_autograd_ref as R
from ptwt_amd import _engine
from tests import _golden as G

pytestmark = pytest.mark.gpu

MODES = ("zero", "constant", "reflect", "periodic", "symmetric")
TAPS = ("dec_lo", "dec_hi", "rec_lo", "rec_hi")
F64_TOL = 1e-10
# float32: the worst norm-wise error of the module on the MI355X was 6.4e-7 (every f32 case, device and host taps): the bound is ten
# times that
F32_TOL = 6e-6

# level events of every call of the module, by tap form: (function, dtype, leg, kernel id)
EVENTS = {"auto": set(), "never": set()}
WORST = {}  # worst norm-wise error per dtype (reported by the last test)


def dev():
    return torch.device("cuda:0")


def weight(t, i):
    return torch.cos(0.37 * torch.arange(t.numel(), dtype=torch.float64, device=t.device) + i).reshape(t.shape).to(t.dtype)


def flat(coeffs):
    return [t for _, t in G.flatten_coeffs(coeffs)]


def random_bank(flen, seed):
    g = np.random.default_rng(1000 + seed)
    return [g.standard_normal(flen) / np.sqrt(flen) for _ in range(4)]


def pywt_bank(name):
    with open(os.path.join(G.GOLDEN, "pywt_filter_banks.json")) as f:
        b = json.load(f)[name]
    return [np.asarray(b[k], dtype=np.float64) for k in TAPS]


def _check(got, want, tol, what):
    got = got.detach().double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = G.relerr(got.numpy(), want.numpy())
    scale = float(want.abs().max())
    assert err < tol, (what, err)
    assert float((got - want).abs().max()) <= 10 * tol * max(scale, 1e-30), (what, "max-abs")
    return err


def _reference(fn, rec, x, bank, kw):
    """Coefficients, reconstruction and the gradients w.r.t. the data and the four filters, float64 on the host."""
    xr = x.detach().double().cpu().requires_grad_(True)
    taps = [torch.tensor(b, dtype=torch.float64).requires_grad_(True) for b in bank]
    coeffs = getattr(R, fn)(xr, tuple(taps), **kw)
    fl = flat(coeffs)
    y = getattr(R, rec)(coeffs, tuple(taps))
    loss = sum((weight(t, i) * t).sum() for i, t in enumerate(fl)) + (weight(y, 7) * y).sum()
    grads = torch.autograd.grad(loss, [xr] + taps)
    return [t.detach() for t in fl], y.detach(), [g.detach() for g in grads]


def run_case(fn, rec, shape, bank, mode, level, dtype, seed=0):
    """One case: the reference once, then the library with device taps and with host taps; each compared with the reference, and the
    two tap forms with each other."""
    tol = F64_TOL if dtype == torch.float64 else F32_TOL
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)
    tap_vals = [torch.tensor(b, dtype=dtype) for b in bank]  # (f32 taps: the reference sees the same rounded values)
    kw = {"mode": mode, "level": level}
    want_c, want_y, want_g = _reference(fn, rec, x, [t.double().numpy() for t in tap_vals], kw)
    res = {}
    for how in ("auto", "never"):
        ptwt_amd.set_device_taps(how)
        _engine.level_events = []
        try:
            taps = [t.to(dev()).requires_grad_(True) for t in tap_vals]
            xd = x.to(dev()).requires_grad_(True)
            coeffs = getattr(ptwt_amd, fn)(xd, tuple(taps), **kw)
            fl = flat(coeffs)
            y = getattr(ptwt_amd, rec)(coeffs, tuple(taps))
            loss = sum((weight(t, i) * t).sum() for i, t in enumerate(fl)) + (weight(y, 7) * y).sum()
            grads = torch.autograd.grad(loss, [xd] + taps)
            torch.cuda.synchronize()
            ev = _engine.level_events
        finally:
            _engine.level_events = None
            ptwt_amd.set_device_taps("auto")
        EVENTS[how].update((fn, dtype, e[0], e[1]) for e in ev)
        where = (fn, shape, len(bank[0]), mode, level, str(dtype), how)
        assert len(fl) == len(want_c), where
        errs = [_check(a, b, tol, where + ("coefficient", i)) for i, (a, b) in enumerate(zip(fl, want_c))]
        errs.append(_check(y, want_y, tol, where + ("reconstruction",)))
        errs.append(_check(grads[0], want_g[0], tol, where + ("d/dx",)))
        errs += [_check(a, b, tol, where + ("d/d" + n,)) for a, b, n in zip(grads[1:], want_g[1:], TAPS)]
        assert all(a.dtype == dtype and a.shape == t.shape for a, t in zip(grads[1:], taps)), where
        WORST[dtype] = max(WORST.get(dtype, 0.0), *errs)
        res[how] = [t.detach() for t in fl] + [y.detach()] + [t.detach() for t in grads]
    for a, b in zip(res["auto"], res["never"]):
        assert G.relerr(a.double().cpu().numpy(), b.double().cpu().numpy()) < tol, (fn, shape, len(bank[0]), mode, "device vs host taps")


EVEN = list(range(2, 33, 2))
LONG = [34, 40]
ODD = [3, 5, 9, 21, 31, 33]
ALL = EVEN + LONG + ODD


def _mode(i):
    return MODES[i % len(MODES)]


def _level(fn, shape, flen):
    """Level 2 where the extents allow it: the reference's pads must fit the second level (reflect: pad < n, periodic: pad <= n), and
    an odd filter needs odd first-level extents for the reference's adjust_trim to hold."""
    ext = shape[-3:] if fn.endswith("3") else shape[-2:] if fn.endswith("2") else shape[-1:]
    m = [(n + n % 2 + flen - 2) // 2 for n in ext]
    ok = all(k > flen - 1 + k % 2 for k in m) and (flen % 2 == 0 or all(k % 2 for k in m))
    return 2 if ok else 1


# ---- 1-D: wavedec / waverec on rows (axis kernels 3 / 4, generic passes for odd and > 32) --------------------------------------------
@pytest.mark.parametrize("flen", ALL)
def test_1d_random_banks(flen):
    shape = (3, 4 * flen + 37 + (flen % 2))
    run_case("wavedec", "waverec", shape, random_bank(flen, flen), _mode(ALL.index(flen)), _level("wavedec", shape, flen), torch.float64,
             flen)


@pytest.mark.parametrize("flen", [2, 8, 14, 20, 24, 32, 40, 5])
def test_1d_random_banks_f32(flen):
    shape = (4, 6 * flen + 41)
    run_case("wavedec", "waverec", shape, random_bank(flen, 50 + flen), _mode(ALL.index(flen) + 2), _level("wavedec", shape, flen),
             torch.float32, flen)


# ---- 2-D: wavedec2 / waverec2 at every length (tiles 7 / 8 with the long 18 / 20 / 24 / 32 builds, border kernels, generic) --------------
def _shape2(flen):
    """Odd and even extents, batch 2; every extent at least 2 (L + 1) (the border kernels of the non-zero modes)."""
    return (2, 2 * flen + 11, 2 * flen + 14)


@pytest.mark.parametrize("flen", ALL)
def test_2d_random_banks(flen):
    modes = MODES if flen in (22, 32) else (_mode(ALL.index(flen) + 1),)
    shape = _shape2(flen)
    for mode in modes:
        run_case("wavedec2", "waverec2", shape, random_bank(flen, 2 * flen), mode, _level("wavedec2", shape, flen), torch.float64, flen)


@pytest.mark.parametrize("flen", [4, 8, 12, 16, 18, 20, 24, 26, 32, 34, 9])
def test_2d_random_banks_f32(flen):
    shape = _shape2(flen)
    run_case("wavedec2", "waverec2", shape, random_bank(flen, 3 * flen), _mode(ALL.index(flen) + 3), _level("wavedec2", shape, flen),
             torch.float32, flen)


@pytest.mark.parametrize("mode", MODES)
def test_2d_f32_plane_one_level_through_the_streaming_kernels(mode):
    """A plane of 256 rows and 896..1280 columns: one level runs on the streaming kernels (ids 16 / 22) with device taps."""
    flen = (4, 6, 8)[MODES.index(mode) % 3]
    run_case("wavedec2", "waverec2", (2, 256, 1030), random_bank(flen, 77), mode, 1, torch.float32, 9)


@pytest.mark.parametrize("name", ["db11", "db13", "db14", "db15", "sym16", "coif5"])
def test_2d_pywt_long_banks(name):
    """The pywt banks of 22, 26, 28, 30, 32 and 30 taps: a backward through a learnable 2-D bank of 22-30 taps used to ask the
    outer-axis kernels for a length they do not serve (libmifwt: valid request this build has no kernel for)."""
    bank = pywt_bank(name)
    flen = len(bank[0])
    shape = _shape2(flen)
    for dtype in (torch.float64, torch.float32):
        run_case("wavedec2", "waverec2", shape, bank, _mode(flen + (dtype == torch.float32)), _level("wavedec2", shape, flen), dtype, flen)


@pytest.mark.parametrize("flen", [6, 16, 26, 34, 5])
def test_fs2d_random_banks(flen):
    shape = (2, 2 * flen + 13, 2 * flen + 8)
    run_case("fswavedec2", "fswaverec2", shape, random_bank(flen, 4 * flen), _mode(ALL.index(flen) + 4), _level("fswavedec2", shape, flen),
             torch.float64, flen)


# ---- 3-D: wavedec3 / waverec3 (host taps: bricks 9 / 10, composed 5 / 6, walk 24 / 25; device taps: generic) ----------------------------
@pytest.mark.parametrize("flen,dtype", [(2, torch.float32), (4, torch.float64), (6, torch.float32), (8, torch.float64),
                                        (10, torch.float64), (3, torch.float64), (14, torch.float64)])
def test_3d_random_banks(flen, dtype):
    shape = (2, flen + 9, flen + 8, flen + 11) if flen <= 10 else (1, 2 * flen - 3, 2 * flen - 2, 2 * flen + 1)
    run_case("wavedec3", "waverec3", shape, random_bank(flen, 5 * flen), _mode(flen), _level("wavedec3", shape, flen), dtype, flen)


def test_3d_f64_volume_on_the_depth_walking_kernels():
    """f64, 4 taps, a volume of more than 2^16 samples: the depth-walking 3-D kernels (ids 24 / 25) with host taps."""
    run_case("wavedec3", "waverec3", (2, 40, 41, 42), random_bank(4, 99), "reflect", 1, torch.float64, 4)


def test_fs3d_random_bank():
    run_case("fswavedec3", "fswaverec3", (2, 15, 14, 17), random_bank(6, 123), "symmetric", 1, torch.float64, 6)


@pytest.mark.parametrize("flen,dtype", [(3, torch.float64), (9, torch.float32), (21, torch.float64)])
def test_zero_mode_analysis_adjoint_of_odd_filters_on_even_extents(flen, dtype):
    """An odd filter on an even extent leaves the reference's pads one coefficient short of a synthesis level of the same extent
    (2 M - L + 2 = N - 1), so the zero-mode analysis adjoint is not that synthesis level; the library used to run it as one anyway and
    the backward failed with "libmifwt: bad argument".  1-D rows and a 2-D plane, every extent even."""
    run_case("wavedec", "waverec", (2, 4 * flen + 40), random_bank(flen, 11 * flen), "zero", 1, dtype, flen)
    run_case("wavedec2", "waverec2", (2, 2 * flen + 12, 2 * flen + 14), random_bank(flen, 13 * flen), "zero", 1, dtype, flen)


# ---- second order ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flen", [22, 32, 5])
def test_2d_double_backward_vs_reference(flen):
    """create_graph=True through a learnable 2-D bank (the mixed second derivatives of _AnalysisLevelGrad / _SynthesisLevelGrad)
    against the reference's own double backward."""
    bank = random_bank(flen, 7 * flen)
    mode = ("reflect", "symmetric", "periodic")[flen % 3]
    x = torch.randn(2, 2 * flen + 5, 2 * flen + 8, generator=torch.Generator().manual_seed(flen), dtype=torch.float64)

    def second(mod, xx, taps):
        coeffs = mod.wavedec2(xx, tuple(taps), mode=mode, level=1)
        f = sum((weight(t, i) * t.square()).sum() for i, t in enumerate(flat(coeffs))) / 2
        y = mod.waverec2(coeffs, tuple(taps))
        f = f + (weight(y, 7) * y.square()).sum() / 2
        first = torch.autograd.grad(f, [xx] + taps, create_graph=True)
        s = sum((gr * weight(gr, 11 + i)).sum() for i, gr in enumerate(first))
        return [t.detach() for t in first] + list(torch.autograd.grad(s, [xx] + taps))

    want = second(R, x.clone().requires_grad_(True), [torch.tensor(b).requires_grad_(True) for b in bank])
    for how in ("auto", "never"):
        ptwt_amd.set_device_taps(how)
        try:
            got = second(ptwt_amd, x.to(dev()).requires_grad_(True), [torch.tensor(b, device=dev()).requires_grad_(True) for b in bank])
        finally:
            ptwt_amd.set_device_taps("auto")
        for i, (a, b) in enumerate(zip(got, want)):
            _check(a, b, F64_TOL, (flen, mode, how, i))


# ---- routes ---------------------------------------------------------------------------------------------------------------------------
def test_routes_of_the_module():
    """Runs last (file order): the device-tap runs reached every kernel that reads device taps, and the generic passes; the forward
    kernels 3 / 7 / 16 on the forward leg and on the synthesis-adjoint leg, the inverse kernels 4 / 8 / 22 on the inverse leg and on the
    analysis-adjoint leg (test_gpu_autograd.test_backward_routes pins that mapping for host taps); the host-tap 3-D cases reached the
    LDS-brick kernels (9 / 10), the composed route (5 / 6) and the depth-walking kernels (24 / 25)."""
    assert EVENTS["auto"], "run the whole module"
    dev_ids = {k for _, _, _, k in EVENTS["auto"]}
    assert {0, 3, 4, 7, 8, 16, 22} <= dev_ids, sorted(dev_ids)
    legs = {leg: {k for _, _, l, k in EVENTS["auto"] if l == leg} for leg in ("fwd", "inv", "fwd_adj", "inv_adj")}
    for leg in ("fwd", "inv_adj"):
        assert {3, 7, 16} <= legs[leg], (leg, sorted(legs[leg]))
    for leg in ("inv", "fwd_adj"):
        assert {4, 8, 22} <= legs[leg], (leg, sorted(legs[leg]))
    host3 = {k for fn, _, _, k in EVENTS["never"] if fn == "wavedec3"}
    assert {5, 6, 9, 10, 24, 25} <= host3, sorted(host3)
    print("\nworst norm-wise error vs the float64 reference:", {str(k): f"{v:.3e}" for k, v in WORST.items()})
