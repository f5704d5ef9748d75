"""GPU tests (``-m gpu``) of bfloat16 storage (C ABI MIFWT_BF16; f32 arithmetic): the bf16 instantiations of the LDS-tile kernels
(ids 7 / 8), the matrix-core kernels (11 / 23), the streaming axis kernels (3 / 4), the generic kernel (0) and the 1-D stationary
kernel.

The reference refuses 16-bit input, so the oracle is the float64 transform (oracle/fwt_oracle.py) of the bf16-quantised input, as
for float16 (tests/test_gpu_parity.py::test_half_storage_extension).  Tolerances, norm-wise per sub-band: the float16 ones times 8 —
every term of the float16 budget is proportional to the unit roundoff of the storage type (2^-11 -> 2^-8), the f32 accumulation terms
are four orders smaller: 4e-3 per level and sub-band (float16: 5e-4), 1.6e-2 for the two-level 1-D round trip (2e-3),
(4e-3 | 8e-3) + 8e-4 for the matrix cores against the tile kernel ((5e-4 | 1e-3) + 1e-4).  DESIGN.md 4.17.
Shapes are those of the float16 tests: ragged tiles, odd pitches (2-byte aligned rows), several tiles per workgroup.
"""
import numpy as np
import pytest
import torch

import ptwt_amd
from oracle import fwt_oracle as O
from oracle import torch_cpu_port as TP
from ptwt_amd import _engine
from tests import _golden as G

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
TOL = 4e-3          # one level, one sub-band
MODES = ["reflect", "zero", "constant", "periodic", "symmetric"]


def dev():
    return torch.device("cuda:0")


def to_np(t):
    return t.detach().double().cpu().numpy()


def bf16_randn(rng, shape):
    return torch.from_numpy(rng.standard_normal(shape)).to(BF16)


def events(fn):
    """fn() with the level events recorded: (result, [(tag, kernel id)])."""
    _engine.level_events = []
    try:
        out = fn()
        torch.cuda.synchronize()
        ev = [(e[0], e[1]) for e in _engine.level_events]
    finally:
        _engine.level_events = None
    return out, ev


@pytest.fixture()
def half():
    ptwt_amd.set_half_storage(True)
    try:
        yield
    finally:
        for key in (6, 7):
            _engine.set_option(key, 0)
        _engine.level_events = None
        ptwt_amd.set_half_storage(False)


def leaves(c):
    return [t for _, t in G.flatten_coeffs(c)]


def check_bands(got, want, tol, what):
    gf, wf = G.flatten_coeffs(got), G.flatten_coeffs(want)
    assert [n for n, _ in gf] == [n for n, _ in wf]
    for (n, a), (_, b) in zip(gf, wf):
        assert a.dtype == BF16 and tuple(a.shape) == tuple(np.shape(b)), (what, n)
        err = G.relerr(to_np(a), b)
        assert err < tol, f"{what} {n}: rel err {err:.3e} >= {tol}"


def test_refused_outside_the_scope_bfloat16_inside_tile_kernels(half):
    """Outside ``half_storage`` bfloat16 is refused as the reference refuses it; inside, db4 ``wavedec2`` and sym16 ``fswavedec2`` (option
    7 = 2: the vector tile kernel), level 2 on (2, 200, 232), run on kernel id 7 and return bfloat16 within 4e-3 per level; the
    reconstructions run on id 8."""
    x = torch.randn(2, 200, 232).to(BF16)
    ptwt_amd.set_half_storage(False)
    with pytest.raises(ValueError, match="Input dtype torch.bfloat16 not supported"):
        ptwt_amd.wavedec2(x.to(dev()), "db4", level=1)
    ptwt_amd.set_half_storage(True)
    _engine.set_option(7, 2)
    for wavelet, fn, ofn, rec, orec in [("sym16", "fswavedec2", O.fswavedec2, "fswaverec2", O.fswaverec2), ("db4", "wavedec2", O.wavedec2, "waverec2", O.waverec2)]:
        cur = x.to(dev())
        got, ev = events(lambda: getattr(ptwt_amd, fn)(cur, wavelet, mode="symmetric", level=2))
        assert [k for _, k in ev] == [7, 7], ev
        # level by level: each against the oracle fed the bf16 approximation the kernel was fed
        for lev in (1, 2):
            one = getattr(ptwt_amd, fn)(cur, wavelet, mode="symmetric", level=1)
            check_bands(one, ofn(to_np(cur), wavelet, mode="symmetric", level=1), TOL, f"{fn} {wavelet} level {lev}")
            for a, b in zip(leaves(one)[1:], leaves((one[0], got[3 - lev]))[1:]):
                assert torch.equal(a, b)
            cur = one[0]
        assert torch.equal(cur, got[0])
        last = (got[0], got[1])
        y, ev = events(lambda: getattr(ptwt_amd, rec)(last, wavelet))
        assert [k for _, k in ev] == [8], ev
        want = orec((to_np(got[0]), {k: to_np(v) for k, v in got[1].items()} if isinstance(got[1], dict) else tuple(to_np(t) for t in got[1])), wavelet)
        assert y.dtype == BF16 and G.relerr(to_np(y), want) < TOL


@pytest.mark.parametrize("wavelet", ["db9", "db10", "db12", "sym16"])
def test_tile_kernels_long_filters(half, wavelet):
    """ids 7 / 8 at 18 / 20 / 24 / 32 taps (option 7 = 2), tile heights automatic, 8 and 24, all five modes, ragged planes and the
    smallest plane the kernels take; synthesis of RANDOM bf16 coefficients of the same extents (not images of an analysis)."""
    rng = np.random.default_rng(len(wavelet) + 700)
    flen = len(O.filter_bank(wavelet)[0])
    _engine.set_option(7, 2)
    for tr in (0, 8, 24):
        _engine.set_option(6, tr)
        for shape in [(2, 131, 3 * flen + 70), (1, 2 * flen, 2 * flen + 1)]:
            assert _engine.kernel_id(2, BF16, "symmetric", flen, shape[0], shape[1:]) == 7
            xq = bf16_randn(rng, shape)
            for mode in MODES:
                try:
                    want = O.wavedec2(to_np(xq), wavelet, mode=mode, level=1)
                except RuntimeError:
                    continue
                got, ev = events(lambda: ptwt_amd.wavedec2(xq.to(dev()), wavelet, mode=mode, level=1))
                assert [k for _, k in ev] == [7], ev
                check_bands(got, want, TOL, f"{wavelet} {mode} {shape} rows={tr}")
            cq = (bf16_randn(rng, want[0].shape), tuple(bf16_randn(rng, b.shape) for b in want[1]))
            ref = O.waverec2((to_np(cq[0]), tuple(to_np(t) for t in cq[1])), wavelet)
            y, ev = events(lambda: ptwt_amd.waverec2((cq[0].to(dev()), tuple(t.to(dev()) for t in cq[1])), wavelet))
            assert [k for _, k in ev] == [8], ev
            assert y.dtype == BF16 and G.relerr(to_np(y), ref) < TOL, (wavelet, shape, tr)


_MFMA_SHAPES = [lambda L: (2, 131, 3 * L + 70), lambda L: (1, 2 * L, 2 * L + 1), lambda L: (3, 300, 402), lambda L: (40, 96, 200)]


@pytest.mark.parametrize("wavelet", ["db9", "db10", "db12", "db14", "sym16"])
def test_mfma_analysis(half, wavelet):
    """Kernel id 11 in bf16 (v_mfma_f32_32x32x16_bf16, taps as bf16 pairs): every mode, ragged tiles, odd and even pitches, several
    tiles per workgroup.  The walk kernel serves every level; each level is within 4e-3 of the oracle fed the same bf16 approximation
    (one bf16 rounding of the intermediate image, one of the output); the multi-level call is bit-identical to its per-level launches;
    and it agrees with the vector tile kernel, which keeps the intermediate image in f32."""
    rng = np.random.default_rng(len(wavelet) + 800)
    flen = len(O.filter_bank(wavelet)[0])
    for mk in _MFMA_SHAPES:
        shape = mk(flen)
        assert _engine.kernel_id(2, BF16, "symmetric", flen, shape[0], shape[1:]) == 11
        xq = bf16_randn(rng, shape).to(dev())
        for mode in MODES:
            level = 2 if min(shape[1:]) > 4 * flen else 1
            try:
                O.wavedec2(to_np(xq[:1]), wavelet, mode=mode, level=level)
            except RuntimeError:
                continue
            n_walk, n_tile = _engine.launch_count(_engine.VARIANT_FWD_MFMA_WALK), _engine.launch_count(_engine.VARIANT_FWD_MFMA_TILE)
            got, ev = events(lambda: ptwt_amd.wavedec2(xq, wavelet, mode=mode, level=level))
            assert [k for _, k in ev] == [11] * level, ev
            assert _engine.launch_count(_engine.VARIANT_FWD_MFMA_WALK) - n_walk == level, (wavelet, mode, shape)
            assert _engine.launch_count(_engine.VARIANT_FWD_MFMA_TILE) == n_tile
            vec = None
            if flen in (18, 20, 24, 32):  # lengths the vector tile kernel is instantiated for
                _engine.set_option(7, 2)
                try:
                    vec = ptwt_amd.wavedec2(xq, wavelet, mode=mode, level=level)
                finally:
                    _engine.set_option(7, 0)
            cur = xq
            for lev in range(1, level + 1):
                one = ptwt_amd.wavedec2(cur, wavelet, mode=mode, level=1)
                check_bands(one, O.wavedec2(to_np(cur), wavelet, mode=mode, level=1), TOL, f"{wavelet} {mode} {shape} level {lev}")
                for a, b in zip(one[1], got[level + 1 - lev]):
                    assert torch.equal(a, b), (wavelet, mode, shape, lev)
                cur = one[0]
            assert torch.equal(cur, got[0])
            if vec is not None:
                for (n, a), (_, c) in zip(G.flatten_coeffs(got), G.flatten_coeffs(vec)):
                    assert G.relerr(to_np(a), to_np(c)) < (4e-3 if level == 1 else 8e-3) + 8e-4, (wavelet, mode, shape, n)


@pytest.mark.parametrize("wavelet", ["db9", "db10", "db12", "db14", "sym16"])
def test_mfma_synthesis(half, wavelet):
    """Kernel id 23 in bf16 (option 7 = 4: wherever it can run): random bf16 coefficient sets, ragged tiles both ways, odd extents
    (trims), segments of any length, against the oracle fed the same coefficients at 4e-3; then the engine's own padded-pitch planes in
    a two-level separable round trip (two levels of bf16 storage: 8e-3; there and back, four: 1.6e-2)."""
    rng = np.random.default_rng(len(wavelet) + 900)
    flen = len(O.filter_bank(wavelet)[0])
    _engine.set_option(7, 4)
    for mk, seg in zip(_MFMA_SHAPES, (0, 0, 3, 1)):
        shape = mk(flen)
        for mode in ("reflect", "periodic", "zero"):
            try:
                c64 = O.wavedec2(rng.standard_normal(shape), wavelet, mode=mode, level=1)
            except RuntimeError:
                continue
            cq = (bf16_randn(rng, c64[0].shape), tuple(bf16_randn(rng, b.shape) for b in c64[1]))
            want = O.waverec2((to_np(cq[0]), tuple(to_np(t) for t in cq[1])), wavelet)
            cdev = (cq[0].to(dev()), tuple(t.to(dev()) for t in cq[1]))
            _engine.set_option(6, seg)
            got, ev = events(lambda: ptwt_amd.waverec2(cdev, wavelet))
            _engine.set_option(6, 0)
            assert [k for _, k in ev] == [23], ev
            assert got.dtype == BF16 and tuple(got.shape) == tuple(want.shape)
            assert G.relerr(to_np(got), want) < TOL, (wavelet, mode, shape, seg)
    x = bf16_randn(rng, (2, 500, 620)).to(dev())
    cs = ptwt_amd.fswavedec2(x, wavelet, mode="symmetric", level=2)
    assert cs[1]["dd"].stride(-2) != cs[1]["dd"].shape[-1] and cs[1]["dd"].stride(-2) * 2 % 128 == 0  # (128-byte aligned rows, as for float16)
    rec, ev = events(lambda: ptwt_amd.fswaverec2(cs, wavelet))
    assert [k for _, k in ev] == [23, 23], ev
    want = O.fswaverec2(tuple([to_np(cs[0])] + [{k: to_np(v) for k, v in d.items()} for d in cs[1:]]), wavelet)
    assert G.relerr(to_np(rec), want) < 2 * TOL
    assert G.relerr(to_np(rec)[..., :500, :620], to_np(x)) < 4 * TOL


def test_streaming_axis_kernels_1d_and_3d(half):
    """ids 3 / 4: ``wavedec`` / ``waverec`` db4 level 2 on (3, 1001) — the round trip at 1.6e-2 (four roundings on the way), each level
    at 4e-3 against the oracle fed the same bf16 values; one long filter, sym16 on (2, 300).  3-D, ``wavedec3`` / ``waverec3`` db2 level 2
    on (2, 20, 22, 25): 16-bit volumes have no fused 3-D kernel and no planes-plus-depth route (ids 5 / 6 are float32 / float64 only), so
    every level runs on the streaming axis passes, ids 3 / 4, rounding to bf16 after each of its three passes: 3 x 4e-3 per level."""
    rng = np.random.default_rng(11)
    for wavelet, shape in (("db4", (3, 1001)), ("sym16", (2, 300))):
        x1 = bf16_randn(rng, shape).to(dev())
        c, ev = events(lambda: ptwt_amd.wavedec(x1, wavelet, level=2))
        assert [k for _, k in ev] == [3, 3], ev
        cur = x1
        for lev in (1, 2):
            one = ptwt_amd.wavedec(cur, wavelet, level=1)
            check_bands(one, O.wavedec(to_np(cur), wavelet, level=1), TOL, f"wavedec {wavelet} level {lev}")
            assert torch.equal(one[1], c[3 - lev])
            cur = one[0]
        assert torch.equal(cur, c[0])
        y, ev = events(lambda: ptwt_amd.waverec(c, wavelet))
        assert [k for _, k in ev] == [4, 4], ev
        assert y.dtype == BF16 and G.relerr(to_np(y)[..., :shape[-1]], to_np(x1)) < 1.6e-2
        cur = c[0]
        for d in c[1:]:
            cur = cur[..., : d.shape[-1]]
            nxt = ptwt_amd.waverec([cur, d], wavelet)
            assert G.relerr(to_np(nxt), O.waverec([to_np(cur), to_np(d)], wavelet)) < TOL
            cur = nxt
    x3 = bf16_randn(rng, (2, 20, 22, 25)).to(dev())
    c3, ev = events(lambda: ptwt_amd.wavedec3(x3, "db2", level=2))
    assert [k for _, k in ev] == [3, 3], ev
    cur = x3
    for lev in (1, 2):
        one = ptwt_amd.wavedec3(cur, "db2", level=1)
        check_bands(one, O.wavedec3(to_np(cur), "db2", level=1), 3 * TOL, f"wavedec3 level {lev}")
        cur = one[0]
    y3, ev = events(lambda: ptwt_amd.waverec3(c3, "db2"))
    assert [k for _, k in ev] == [4, 4], ev
    want = O.waverec3(tuple([to_np(c3[0])] + [{k: to_np(v) for k, v in d.items()} for d in c3[1:]]), "db2")
    assert y3.dtype == BF16 and G.relerr(to_np(y3), want) < 2 * 3 * TOL


def test_generic_kernel_outside_the_fused_envelopes(half):
    """id 0 in bf16 storage: filter lengths no other kernel is instantiated for (40 taps in 2-D, 30 taps in 1-D).  The two passes of
    a 2-D level round to bf16 each: 2 x 4e-3 per level, as float16 has 2e-3 per level there."""
    torch.manual_seed(21)
    for fn, ofn, shape, wavelet, mode, level, passes in [("wavedec2", O.wavedec2, (2, 90, 86), "db20", "reflect", 1, 2),
                                                         ("wavedec", O.wavedec, (3, 300), "coif5", "periodic", 2, 1)]:
        x = torch.randn(*shape, device=dev()).to(BF16)
        got, ev = events(lambda: getattr(ptwt_amd, fn)(x, wavelet, mode=mode, level=level))
        assert [k for _, k in ev] == [0] * level, ev
        check_bands(got, ofn(to_np(x), wavelet, mode=mode, level=level), passes * TOL * level, f"{fn} {wavelet}")


def test_stationary_1d(half):
    """``swt`` / ``iswt`` db2 level 3 on (3, 1001) in bf16 against the same calls on the float32 copy of the same values: 8e-3 where the
    float16 test has 1e-3 (level k has been rounded k times)."""
    x = torch.randn(3, 1001, device=dev()).to(BF16)
    cb = ptwt_amd.swt(x, "db2", 3)
    cf = ptwt_amd.swt(x.float(), "db2", 3)
    for a, b in zip(cb, cf):
        assert a.dtype == BF16 and G.relerr(to_np(a), to_np(b)) < 8e-3
    y = ptwt_amd.iswt(cb, "db2")
    assert y.dtype == BF16 and G.relerr(to_np(y), to_np(ptwt_amd.iswt([t.float() for t in cb], "db2"))) < 8e-3


def test_range_five_levels_of_a_constant_plane(half):
    """The range argument: a 2-D haar pyramid of depth 5 multiplies a constant by 32.  4096 everywhere gives an approximation of
    exactly 131072 = 2^17 in bfloat16 (periodic: no border effect; a level's f32 result 2 c (1 + O(2^-24)) rounds to the power of two
    2 c) and ``inf`` in float16 (65536 is past its largest finite value at the fourth level)."""
    x = torch.full((2, 64, 64), 4096.0, device=dev())
    cb = ptwt_amd.wavedec2(x.to(BF16), "haar", level=5, mode="periodic")
    assert cb[0].dtype == BF16 and tuple(cb[0].shape) == (2, 2, 2) and bool((cb[0].float() == 131072.0).all())
    ch = ptwt_amd.wavedec2(x.half(), "haar", level=5, mode="periodic")
    assert bool(torch.isinf(ch[0]).all())


def test_data_gradients_against_float64_autograd(half):
    """``wavedec2`` db4 level 1 on (2, 40, 52), reflect mode, and ``waverec2`` of its coefficients: the gradient w.r.t. the data against
    float64 autograd through oracle/torch_cpu_port.py on the same (bf16-quantised) operands and upstream gradients.

    Roundings on the route, counted from the code (they are the float16 route's):
      * analysis backward: the boundary part of a mirrored-mode adjoint (mifwt_adjoint_border.hip) exists for float32 / float64 only, so
        a 16-bit adjoint never takes the interior-kernel-plus-border-kernel route; it runs on the generic adjoint passes (kernel id 0),
        one per axis, the first writing 16-bit scratch: TWO roundings, 8e-3;
      * synthesis backward: a zero-mode analysis level with reversed taps on the LDS-tile kernel (id 7), the intermediate image in f32
        in LDS: ONE rounding, 4e-3."""
    rng = np.random.default_rng(31)
    xq = bf16_randn(rng, (2, 40, 52))
    x = xq.to(dev()).requires_grad_(True)
    c = ptwt_amd.wavedec2(x, "db4", mode="reflect", level=1)
    leaves = [t for _, t in G.flatten_coeffs(c)]
    ws = [bf16_randn(rng, tuple(t.shape)) for t in leaves]
    (gx,), ev = events(lambda: torch.autograd.grad(leaves, x, [w.to(dev()) for w in ws]))
    assert ev == [("fwd_adj", 0)], ev  # (the generic adjoint passes)
    x64 = xq.double().requires_grad_(True)
    c64 = TP.wavedec2(x64, "db4", mode="reflect", level=1)
    (want,) = torch.autograd.grad([c64[0], *c64[1]], x64, [w.double() for w in ws])
    assert gx.dtype == BF16 and G.relerr(to_np(gx), want.numpy()) < 2 * TOL

    cq = [t.detach().clone().requires_grad_(True) for t in leaves]
    y = ptwt_amd.waverec2((cq[0], tuple(cq[1:])), "db4")
    wy = bf16_randn(rng, tuple(y.shape))
    gc, ev = events(lambda: torch.autograd.grad(y, cq, wy.to(dev())))
    assert ev == [("inv_adj", 7)], ev
    c64 = [t.detach().double().cpu().requires_grad_(True) for t in leaves]
    y64 = TP.waverec2((c64[0], tuple(c64[1:])), "db4")
    want = torch.autograd.grad(y64, c64, wy.double())
    for a, b in zip(gc, want):
        assert a.dtype == BF16 and G.relerr(to_np(a), b.numpy()) < TOL


def test_public_refusals_on_the_device(half):
    """What float16 is refused on the device, bfloat16 is refused with the same exception type and message: the Matrix* transforms
    (their device check comes before the dtype's, tests/test_bf16_host.py), the periodized and value-map modes, swt2 / swt3."""
    calls = [lambda t: ptwt_amd.MatrixWavedec("db2", 1)(t.reshape(2, -1)), lambda t: ptwt_amd.MatrixWavedec2("db2", 1)(t),
             lambda t: ptwt_amd.MatrixWavedec3("db2", 1)(t.reshape(2, 8, 8, 16)), lambda t: ptwt_amd.wavedec2(t, "db2", mode="periodization"),
             lambda t: ptwt_amd.wavedec2(t, "db2", mode="smooth"), lambda t: ptwt_amd.swt2(t, "haar", level=1),
             lambda t: ptwt_amd.swt3(t.reshape(2, 8, 8, 16), "haar", level=1)]
    x = torch.randn(2, 32, 32, device=dev())
    for call in calls:
        seen = []
        for dt in (torch.float16, BF16):
            with pytest.raises((ValueError, NotImplementedError)) as e:
                call(x.to(dt))
            seen.append((type(e.value), str(e.value).replace(str(dt), "DT")))
        assert seen[0] == seen[1], seen


def test_axes_and_packets_on_padded_modes(half):
    """``axes`` and the packet trees behave as for float16: the same call on the bf16 values held in float32 is the reference.  A level
    rounds to bf16 once on a fused kernel and twice on the axis passes (what a permuted layout may take); a level's rounding error
    passes through the next, orthogonal, level unamplified: two levels are at most four roundings, 4 x 4e-3, a round trip eight."""
    x = torch.randn(3, 64, 72, 5, device=dev()).to(BF16)
    got = ptwt_amd.wavedec2(x, "db3", level=2, axes=(1, 2))
    want = ptwt_amd.wavedec2(x.float(), "db3", level=2, axes=(1, 2))
    for a, b in zip(leaves(got), leaves(want)):
        assert a.dtype == BF16 and a.shape == b.shape and G.relerr(to_np(a), to_np(b)) < 4 * TOL
    y = ptwt_amd.waverec2(got, "db3", axes=(1, 2))
    assert y.dtype == BF16 and G.relerr(to_np(y)[:, :64, :72], to_np(x)) < 8 * TOL
    p = torch.randn(4, 64, 96, device=dev()).to(BF16)
    for key in ("aa", "ad", "dd"):
        a = ptwt_amd.WaveletPacket2D(p, "db2", mode="reflect", maxlevel=2)[key]
        b = ptwt_amd.WaveletPacket2D(p.float(), "db2", mode="reflect", maxlevel=2)[key]
        assert a.dtype == BF16 and G.relerr(to_np(a), to_np(b)) < 4 * TOL, key


def test_captured_call_replays_bit_identically(half):
    """``capture()`` of a bf16 ``fswavedec2`` / ``wavedec2`` on (2, 300, 402) — the matrix-core kernel and the tile kernel — replays
    bit-identically to the eager call on fresh data."""
    xh = torch.randn(2, 300, 402, device=dev()).to(BF16)
    x2 = torch.randn(2, 300, 402, device=dev()).to(BF16)
    for fn, wavelet in ((ptwt_amd.fswavedec2, "sym16"), (ptwt_amd.wavedec2, "db4")):
        g = ptwt_amd.capture(lambda t: fn(t, wavelet, level=2), xh)
        for (_, a), (_, b) in zip(G.flatten_coeffs(g(x2)), G.flatten_coeffs(fn(x2, wavelet, level=2))):
            assert a.dtype == BF16 and torch.equal(a, b)
