"""GPU tests (``-m gpu``) of complex data: the fused interleaved levels (csrc/mifwt_cplx.hip, kernel ids 46 / 47), the composed route and
the ten public functions on ``torch.complex64`` / ``torch.complex128`` tensors, against tests/_cplx_ref.py (the float64 reference of each
mode applied to ``.real`` and ``.imag``; tests/test_cplx_host.py pins it to PyWavelets' recordings).

1. Single levels and their inverses through ``_cplx.level_fwd`` / ``level_inv``, the five index-map modes and both dtypes, on the fused
   route and again under ``FORCE_COMPOSED``: rows of 1, 2, 3, 5, 8, 13, 33, 127, 128, 129, 131 and 1031 samples plus 511 / 512 / 513 and
   1023 / 1024 / 1025 (batch 3; the 1-D tiles are 512 samples of the synthesis and 256 / 512 coefficients of the analysis), planes 1x7,
   2x2, 5x7, 13x10, 33x65, 34x130 and 67x131, each a slice of a wider tensor with an odd row pitch that starts at an odd element (the
   8-byte path of complex64), volumes 5x6x7 and 9x8x12; haar, db2, db4, bior3.5, db10, one random 24-tap bank (composed on both routes)
   and one bank of four independent random 8-tap filters.  Where the real call's pad check raises, the complex call raises the same
   error; everywhere else the values are compared.  ``mifwt_launch_count`` must show the intended ids per cell.
2. Whole calls: ``wavedec`` / ``wavedec2`` / ``wavedec3`` at levels 1 to 3 against the oracle, ``waverec*`` of the results against the
   reference and back to the input; ``fswavedec2`` / ``fswaverec2``, a permuted-axes call, one call each in "periodization" and "smooth".
3. Exactness, bitwise: the real plane of every output depends on the real plane of the input alone and the other way round; a zero
   imaginary part stays zero; swapping the components swaps the outputs.
4. Data gradients against float64 autograd through the reference with complex Gaussian cotangents, second order under
   ``create_graph=True`` in complex128, tap gradients of a learnable db2 bank in 1-D and 2-D.
5. Entry by entry: real and imaginary unit impulses through the fused level and its inverse at N = 13 and 16 under db4, "symmetric" and
   "reflect": the operator is the reference operator and no entry couples the components.
6. ``ptwt_amd.capture`` replays to the same bits; guard regions around every output of ids 46 / 47 stay intact.

The fused tests run with ``_cplx.COMPOSED_CELLS`` emptied: which cells a default call fuses is a measured routing decision
(tools/cplx_bench.py), not a matter of these tests; ``test_default_routing_follows_the_cell_sets`` pins that a default call follows it.

Bounds, norm-wise per tensor over both components (``_cplx_ref.relerr``): complex128 1e-12 (values) / 1e-10 (gradients).  complex64
values: max(1e-6, 10 x e_ref32(cell)), e_ref32 = the error of the REFERENCE's complex64 run against its own complex128 run on the same
inputs.  Only a band that is zero in exact arithmetic (below ``ZERO_BAND`` of the input's norm) is measured relative to the norm of the
transform's input.  complex64 gradients: ``python -m tests.test_gpu_cplx`` runs the reference in complex64 on the host over GRAD_CASES x
GRAD_MODES x GRAD_WAVELETS and prints its worst norm-wise gradient error against its complex128 run, over d wavedec* / d x and d waverec* / d coefficient: 1.84e-7
(wavedec3 of 1x9x8x12 under db4, "symmetric"); the bound is ten times that, C64_GRAD_TOL = 1.8e-6.  Tap gradients in complex64: ten times
the error of the reference's own float32 run of the same loss, computed in the test.

On the MI355X (67 cases, 10 s; 14 760 comparisons): complex128 values at 1.4e-15 and below on whole calls and 4.1e-14 and below on single
levels (the inverse of the 1x7 plane under the random 8-tap bank, a badly conditioned cell), complex128 gradients at 6.3e-16 and below,
second order 2.6e-16; complex64 whole calls at 5.2e-7, data and coefficient gradients at 1.8e-7, tap gradients at 2.4e-7.  The check
closest to its bound: complex128 at 0.04 of it (that inverse), complex64 at 0.33 of it (`wavedec3` db2 in "smooth", composed: 1.11e-6
against 3.4e-6).  Swapping the two components swapped the outputs BIT FOR BIT in every cell tried (rows of 1031, the 67x131 plane, the
9x8x12 volume, five modes, both dtypes, level and inverse).
"""
import ctypes

import numpy as np
import pytest
import torch

import ptwt_amd
from oracle import fwt_oracle as O
from oracle import torch_autograd_ref as A
from ptwt_amd import _cplx, _engine, _fwt
from ptwt_amd._wavelets import host_taps
from tests import _cplx_ref as R
from tests import _ext_ref

pytestmark = pytest.mark.gpu

C128_TOL, C128_GRAD_TOL = 1e-12, 1e-10
C64_GRAD_TOL = 1.8e-6  # 10 x the complex64 reference's own worst gradient error over the gradient cases (module docstring)
MODES = R.OLD_MODES
DTYPES = (torch.complex64, torch.complex128)
ROWS = [1, 2, 3, 5, 8, 13, 33, 127, 128, 129, 131, 1031, 511, 512, 513, 1023, 1024, 1025]
PLANES = [(1, 7), (2, 2), (5, 7), (13, 10), (33, 65), (34, 130), (67, 131)]
VOLUMES = [(5, 6, 7), (9, 8, 12)]
WAVELETS = ("haar", "db2", "db4", "bior3.5", "db10", "rand24", "indep8")
KIDS = (46, 47)
WORST = {}
_REFS = {}


def dev():
    return torch.device("cuda:0")


def _name(dtype):
    return str(dtype).split(".")[-1]


def _rand_bank(flen, seed):
    g = np.random.default_rng(seed)
    return tuple(tuple(float(np.float32(v)) for v in g.standard_normal(flen) / np.sqrt(flen)) for _ in range(4))


def _bank(wavelet):
    if wavelet == "rand24":
        return _rand_bank(24, 24)
    if wavelet == "indep8":  # four INDEPENDENT filters: a kernel that took rec for dec, or lo for hi, cannot pass
        return _rand_bank(8, 8)
    return host_taps(wavelet)


def _counts():
    return [_engine.launch_count(k) for k in KIDS]


def _delta(before):
    return [a - b for a, b in zip(_counts(), before)]


def _check(got, want, tol, what, key=None, scale=0.0):
    return R.check(got, want, tol, what, scale, WORST if key is not None else None, key)


def _tol(dtype, e32):
    return C128_TOL if dtype == torch.complex128 else max(1e-6, 10 * e32)


@pytest.fixture
def fused_cells(monkeypatch):
    """Every cell of the fused envelope on the fused kernels, whatever the measured routing says."""
    monkeypatch.setattr(_cplx, "COMPOSED_CELLS", set())
    _cplx._plans.clear()
    yield
    _cplx._plans.clear()


def _cell(mode, wavelet, shape):
    """The complex128 reference of one cell, computed once and shared: input, the level, its inverse, the reference's complex64 errors."""
    key = (mode, wavelet, shape)
    if key not in _REFS:
        bank, ndim = _bank(wavelet), len(shape) - 1
        x = R.gauss(shape, 11 * sum(shape) + len(bank[0]))
        fwd = lambda t: R.level_fwd(t, bank, mode, ndim)  # noqa: E731
        bands = fwd(x)
        inv = lambda *b: R.level_inv(list(b), bank, ndim, None, shape[1:])  # noqa: E731
        g = [b.to(torch.complex64).to(torch.complex128) for b in bands]  # the inverse's input: the bands as complex64 holds them
        _REFS[key] = {"x": x, "fwd": bands, "g": g, "inv": inv(*g), "e_fwd": R.e_ref32(fwd, x, scale=float(x.norm())),
                      "e_inv": R.e_ref32(inv, *g)}
    return _REFS[key]


def _on_device(t, dtype, pitched=False):
    """``t`` on the device; ``pitched``: as a slice of a wider tensor with an odd row pitch that starts at an odd element."""
    t = t.to(dtype)
    if pitched:
        wide = torch.zeros(*t.shape[:-1], t.shape[-1] + 4 + (t.shape[-1] + 1) % 2, dtype=dtype)
        wide[..., 1:1 + t.shape[-1]] = t
        assert wide.stride(-2) % 2 == 1
        return wide.to(dev())[..., 1:1 + t.shape[-1]]
    return t.to(dev())


def _pad_check_raises(shape, flen, mode):
    try:
        _fwt._check_pad(shape[1:], flen, mode)
    except RuntimeError as err:
        return err
    return None


# ---- 1. single levels ------------------------------------------------------------------------------------------------------------------
_DEC = {1: (ptwt_amd.wavedec, ptwt_amd.waverec), 2: (ptwt_amd.wavedec2, ptwt_amd.waverec2), 3: (ptwt_amd.wavedec3, ptwt_amd.waverec3)}


def _run_cell(mode, dtype, wavelet, shape, route):
    bank, ndim = _bank(wavelet), len(shape) - 1
    flen = len(bank[0])
    what = (mode, _name(dtype), wavelet, shape, route)
    err = _pad_check_raises(shape, flen, mode)
    if err is not None:  # the real call's pad check raises: the complex call raises the same error
        x = torch.zeros(shape, dtype=dtype, device=dev())
        with pytest.raises(RuntimeError) as real:
            _DEC[ndim][0](x.real.contiguous(), bank, mode=mode, level=1)
        with pytest.raises(RuntimeError) as cplx:
            _DEC[ndim][0](x, bank, mode=mode, level=1)
        assert str(real.value) == str(cplx.value) == str(err), what
        return
    ref = _cell(mode, wavelet, shape)
    pitched = ndim == 2
    x = _on_device(ref["x"], dtype, pitched)
    bands = [_on_device(b, dtype, pitched) for b in ref["g"]]
    fused = route == "fused"
    _cplx.FORCE_COMPOSED = not fused
    try:
        before = _counts()
        buf = _cplx.level_fwd(x, bank[0], bank[1], _engine.MODE_IDS[mode])
        d_fwd = _delta(before)
        before = _counts()
        y = _cplx.level_inv(bands, bank[2], bank[3], shape[1:])
        d_inv = _delta(before)
    finally:
        _cplx.FORCE_COMPOSED = False
    if fused and flen <= 20:
        assert (d_fwd, d_inv) == ([1, 0], [0, 1]), (what, d_fwd, d_inv)
    else:
        assert (d_fwd, d_inv) == ([0, 0], [0, 0]), (what, d_fwd, d_inv)
    assert buf.dtype == dtype and y.dtype == dtype
    scale = float(ref["x"].norm())
    for s, want in enumerate(ref["fwd"]):
        _check(buf[:, s], want, _tol(dtype, ref["e_fwd"]), what + ("band", s), "level %s %s" % (route, _name(dtype)), scale)
    _check(y, ref["inv"], _tol(dtype, ref["e_inv"]), what + ("inverse",), "inverse %s %s" % (route, _name(dtype)))


@pytest.mark.parametrize("route", ["fused", "composed"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("mode", MODES)
def test_single_levels(mode, dtype, route, fused_cells):
    for wavelet in WAVELETS:
        for shape in [(3, n) for n in ROWS] + [(2, *p) for p in PLANES] + [(2, *v) for v in VOLUMES]:
            _run_cell(mode, dtype, wavelet, shape, route)


def test_default_routing_follows_the_cell_sets():
    """Without the fixture: a default call fuses exactly the cells of ``_cplx.FUSED_AHEAD``."""
    _cplx._plans.clear()
    for dtype in DTYPES:
        for wavelet, shape in (("db4", (3, 131)), ("db4", (2, 33, 65)), ("db8", (2, 33, 65)), ("db5", (3, 1031)), ("db2", (2, 9, 8, 12))):
            bank, ndim = host_taps(wavelet), len(shape) - 1
            x = R.gauss(shape, 5).to(dtype).to(dev())
            before = _counts()
            buf = _cplx.level_fwd(x, bank[0], bank[1], 4)
            _cplx.level_inv(list(buf.unbind(1)), bank[2], bank[3], shape[1:])
            want = [int((0, dtype, len(bank[0]), ndim) in _cplx.FUSED_AHEAD), int((1, dtype, len(bank[0]), ndim) in _cplx.FUSED_AHEAD)]
            assert _delta(before) == want, (dtype, wavelet, shape)


# ---- 2. whole calls ----------------------------------------------------------------------------------------------------------------------
_ORACLE = {1: (O.wavedec, "axis"), 2: (O.wavedec2, "axes"), 3: (O.wavedec3, "axes")}
API_CASES = [((3, 131), 1, "db4"), ((2, 33, 65), 2, "db4"), ((2, 13, 10), 2, "bior3.5"), ((1, 9, 8, 12), 3, "db2")]


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("mode", MODES)
def test_whole_calls_and_round_trip(mode, dtype, fused_cells):
    for shape, ndim, wavelet in API_CASES:
        bank = host_taps(wavelet)
        x64 = R.gauss(shape, sum(shape))
        scale = float(x64.norm())
        dec, rec = _DEC[ndim]
        for level in (1, 2, 3):
            what = (mode, _name(dtype), shape, wavelet, level)
            try:
                _fwt._check_pad_levels(shape[1:], len(bank[0]), mode, level)
            except RuntimeError as err:
                with pytest.raises(RuntimeError) as got:
                    dec(x64.to(dtype).to(dev()), wavelet, mode=mode, level=level)
                assert str(got.value) == str(err), what
                continue
            want = R.wavedecn(x64, bank, mode, ndim, level)
            oracle = R.flat(R.api_to_ref(R.oracle_call(_ORACLE[ndim][0], x64, wavelet, mode=mode, level=level), ndim))
            e32 = R.e_ref32(lambda t: R.flat(R.wavedecn(t, bank, mode, ndim, level)), x64, scale=scale)
            before = _counts()
            coeffs = dec(x64.to(dtype).to(dev()), wavelet, mode=mode, level=level)
            assert _delta(before) == [level, 0], what
            for i, (a, b) in enumerate(zip(R.flat(R.api_to_ref(coeffs, ndim)), oracle)):
                assert a.dtype == dtype
                _check(a, b, _tol(dtype, e32), what + ("coefficient", i), "api values %s" % _name(dtype), scale)
            want_rec = R.waverecn(want, bank, ndim)
            e32r = R.e_ref32(lambda t: R.waverecn(R.wavedecn(t, bank, mode, ndim, level), bank, ndim), x64)
            before = _counts()
            y = rec(coeffs, wavelet)
            assert _delta(before) == [0, level] and y.dtype == dtype, what
            _check(y, want_rec, _tol(dtype, e32r), what + ("round trip vs reference",), "api round trip %s" % _name(dtype))
            # back to the input: the reference's round trip is the input to 1e-10 (float64, biorthogonal banks included), so the
            # library's is within its bound against the reference plus that
            crop = (slice(None),) + tuple(slice(0, n) for n in shape[1:])
            assert R.relerr(want_rec[crop], x64) < 1e-10, what
            _check(y[crop], x64, _tol(dtype, e32r) + 1e-10, what + ("round trip vs input",))


def test_separable_permuted_and_the_composed_modes(fused_cells):
    dtype = torch.complex128
    bank = host_taps("db2")
    x64 = R.gauss((2, 13, 10), 5)
    x = x64.to(dev())
    want = R.wavedecn(x64, bank, "symmetric", 2, 2)
    fs = ptwt_amd.fswavedec2(x, "db2", mode="symmetric", level=2)
    _check(fs[0], want[0], C128_TOL, ("fswavedec2 approximation",))
    for lvl, det in zip(fs[1:], want[1:]):
        for key, band in (("ad", 0), ("da", 1), ("dd", 2)):
            _check(lvl[key], det[band], C128_TOL, ("fswavedec2", key))
    before = _counts()
    _check(ptwt_amd.fswaverec2(fs, "db2"), R.waverecn(want, bank, 2), C128_TOL, ("fswaverec2",))
    assert _delta(before) == [0, 2]
    # permuted axes: the samples are not contiguous, the first level is composed, the second one (a dense buffer) fused
    xp = x64.permute(1, 2, 0).contiguous().to(dev())  # [13, 10, 2], transformed axes (0, 1)
    before = _counts()
    cp = ptwt_amd.wavedec2(xp, "db2", mode="symmetric", level=2, axes=(0, 1))
    assert _delta(before) == [1, 0]
    for a, b in zip(R.flat(R.api_to_ref(cp, 2)), R.flat(want)):
        _check(a.permute(2, 0, 1), b, C128_TOL, ("permuted axes",))
    _check(ptwt_amd.waverec2(cp, "db2", axes=(0, 1)).permute(2, 0, 1), R.waverecn(want, bank, 2), C128_TOL, ("permuted axes, waverec2",))
    # the modes without fused complex levels: composed from the real calls
    for mode in ("periodization", "smooth"):
        for ndim, shape in ((1, (3, 37)), (2, (2, 13, 10)), (3, (1, 9, 8, 12))):
            for dt in DTYPES:
                x64 = R.gauss(shape, 7 + ndim)
                want = R.wavedecn(x64, bank, mode, ndim, 2)
                e32 = R.e_ref32(lambda t: R.flat(R.wavedecn(t, bank, mode, ndim, 2)), x64, scale=float(x64.norm()))
                before = _counts()
                coeffs = _DEC[ndim][0](x64.to(dt).to(dev()), "db2", mode=mode, level=2)
                for a, b in zip(R.flat(R.api_to_ref(coeffs, ndim)), R.flat(want)):
                    assert a.dtype == dt
                    _check(a, b, _tol(dt, e32), (mode, ndim, _name(dt), "values"), "composed modes %s" % _name(dt), float(x64.norm()))
                y = _DEC[ndim][1](coeffs, "db2", mode=mode)
                assert _delta(before) == [0, 0] and y.dtype == dt
                e32r = R.e_ref32(lambda t: R.waverecn(R.wavedecn(t, bank, mode, ndim, 2), bank, ndim, mode), x64)
                _check(y, R.waverecn(want, bank, ndim, mode), _tol(dt, e32r), (mode, ndim, _name(dt), "round trip"))


def test_device_taps_take_the_composed_route(fused_cells):
    x64 = R.gauss((2, 33, 65), 9)
    bank_t = tuple(torch.tensor(t, dtype=torch.float64, device=dev()) for t in host_taps("db4"))
    want = R.flat(R.wavedecn(x64, host_taps("db4"), "reflect", 2, 2))
    ptwt_amd.set_device_taps("always")
    try:
        before = _counts()
        coeffs = ptwt_amd.wavedec2(x64.to(dev()), bank_t, mode="reflect", level=2)
        y = ptwt_amd.waverec2(coeffs, bank_t)
        assert _delta(before) == [0, 0]
    finally:
        ptwt_amd.set_device_taps("auto")
    for a, b in zip(R.flat(R.api_to_ref(coeffs, 2)), want):
        _check(a, b, C128_TOL, ("device taps",))
    _check(y, R.waverecn(R.wavedecn(x64, host_taps("db4"), "reflect", 2, 2), host_taps("db4"), 2), C128_TOL, ("device taps, round trip",))


# ---- 3. exactness ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("shape", [(3, 1031), (2, 67, 131), (2, 9, 8, 12)], ids=lambda s: "x".join(map(str, s)))
def test_components_never_meet(dtype, shape, fused_cells):
    bank, ndim = host_taps("db4" if len(shape) < 4 else "db2"), len(shape) - 1
    x64 = R.gauss(shape, 21)
    x = x64.to(dtype).to(dev())
    other = R.gauss(shape, 22).to(dtype).to(dev())
    swapped_bit_equal = []
    for mode in MODES:
        if _pad_check_raises(shape, len(bank[0]), mode) is not None:
            continue
        mid = _engine.MODE_IDS[mode]
        # the value bound of this cell: the level and the inverse of its result, as the reference computes them in complex64
        e32 = R.e_ref32(lambda t: [torch.stack(R.level_fwd(t, bank, mode, ndim), 1),
                                   R.level_inv(R.level_fwd(t, bank, mode, ndim), bank, ndim, None, shape[1:])], x64, scale=float(x64.norm()))

        def both(t):
            before = _counts()
            buf = _cplx.level_fwd(t, bank[0], bank[1], mid)
            y = _cplx.level_inv(list(buf.unbind(1)), bank[2], bank[3], shape[1:])
            assert _delta(before) == [1, 1]
            return buf, y

        ref = both(x)
        again = both(x)
        new_im = both(torch.complex(x.real, other.imag))
        new_re = both(torch.complex(other.real, x.imag))
        zero_im = both(torch.complex(x.real, torch.zeros_like(x.real)))
        swapped = both(torch.complex(x.imag, x.real))
        for r, a, ni, nr, z, sw in zip(ref, again, new_im, new_re, zero_im, swapped):
            assert torch.equal(torch.view_as_real(r), torch.view_as_real(a)), (mode, "the same input gives the same bits")
            assert torch.equal(ni.real, r.real), (mode, "the real plane depends on the real plane alone")
            assert torch.equal(nr.imag, r.imag), (mode, "the imaginary plane depends on the imaginary plane alone")
            assert torch.equal(z.real, r.real) and not bool(z.imag.any()), (mode, "a zero imaginary part stays zero")
            _check(torch.complex(sw.imag, sw.real), r, _tol(dtype, e32), (mode, _name(dtype), shape, "components swapped"))
            swapped_bit_equal.append(torch.equal(sw.imag, r.real) and torch.equal(sw.real, r.imag))
    print("swapping the components swaps the outputs bit for bit:", _name(dtype), shape, all(swapped_bit_equal))


# ---- 4. gradients --------------------------------------------------------------------------------------------------------------------------
GRAD_CASES = [((3, 13), 1), ((2, 5, 7), 2), ((2, 33, 65), 2), ((1, 9, 8, 12), 3)]
GRAD_WAVELETS = ("db2", "db4")
GRAD_MODES = ("reflect", "symmetric", "zero")
GRAD_LEVEL = 2


def _cotangents(tensors, seed):
    return [R.gauss(t.shape, 2000 + 17 * seed + i) for i, t in enumerate(tensors)]


def _nest(flat, ndim):
    nb = (1 << ndim) - 1
    return [flat[0]] + [list(flat[1 + i * nb:1 + (i + 1) * nb]) for i in range((len(flat) - 1) // nb)]


def _ref_to_api(nested, ndim):
    """The nested lists of the reference as the container of the public functions."""
    if ndim == 1:
        return [nested[0]] + [d[0] for d in nested[1:]]
    if ndim == 2:
        return (nested[0],) + tuple((d[1], d[0], d[2]) for d in nested[1:])
    return (nested[0],) + tuple({format(s, "03b").replace("0", "a").replace("1", "d"): t for s, t in enumerate(d, start=1)} for d in nested[1:])


def _ref_grad(x64, bank, mode, ndim, dtype):
    """(d <wavedec x, ws> / d x, ws, d <waverec c, wy> / d c, wy) by autograd through the reference in ``dtype``."""
    x = x64.to(dtype).requires_grad_(True)
    flat = R.flat(R.wavedecn(x, bank, mode, ndim, GRAD_LEVEL))
    ws = _cotangents(flat, sum(x64.shape))
    (g_x,) = torch.autograd.grad(flat, x, [w.to(dtype) for w in ws])
    leaves = [c.detach().requires_grad_(True) for c in flat]
    y = R.waverecn(_nest(leaves, ndim), bank, ndim)
    wy = R.gauss(y.shape, 31)
    g_c = torch.autograd.grad(y, leaves, wy.to(dtype))
    return g_x, ws, g_c, wy


def _grad_cases(mode, wavelet):
    flen = len(host_taps(wavelet)[0])
    for shape, ndim in GRAD_CASES:
        try:
            _fwt._check_pad_levels(shape[1:], flen, mode, GRAD_LEVEL)
        except RuntimeError:
            continue
        yield shape, ndim


@pytest.mark.parametrize("wavelet", GRAD_WAVELETS)
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("mode", GRAD_MODES)
def test_data_gradients(mode, dtype, wavelet):
    """A call that wants a graph is composed from the real calls: their autograd Functions and torch's real / imag / complex backward
    give T^T g.real + i T^T g.imag, torch's convention for a real-linear map.  Both directions: the decomposition w.r.t. the data, the
    reconstruction w.r.t. every coefficient."""
    bank = host_taps(wavelet)
    tol = C128_GRAD_TOL if dtype == torch.complex128 else C64_GRAD_TOL
    for shape, ndim in _grad_cases(mode, wavelet):
        x64 = R.gauss(shape, sum(shape))
        want, ws, want_c, wy = _ref_grad(x64, bank, mode, ndim, torch.complex128)
        x = x64.to(dtype).to(dev()).requires_grad_(True)
        before = _counts()
        flat = R.flat(R.api_to_ref(_DEC[ndim][0](x, wavelet, mode=mode, level=GRAD_LEVEL), ndim))
        (g_x,) = torch.autograd.grad(flat, x, [w.to(dtype).to(dev()) for w in ws])
        assert g_x.dtype == dtype
        _check(g_x, want, tol, (mode, _name(dtype), shape, wavelet, "d/dx"), "data gradients %s" % _name(dtype))
        leaves = [c.detach().requires_grad_(True) for c in flat]
        y = _DEC[ndim][1](_ref_to_api(_nest(leaves, ndim), ndim), wavelet)
        got_c = torch.autograd.grad(y, leaves, wy.to(dtype).to(dev()))
        assert _delta(before) == [0, 0]  # (a call that wants a graph takes the composed route)
        for i, (a, b) in enumerate(zip(got_c, want_c)):
            _check(a, b, tol, (mode, _name(dtype), shape, wavelet, "d waverec / d coefficient", i), "coefficient gradients %s" % _name(dtype))


@pytest.mark.parametrize("mode", ["symmetric", "zero"])
def test_second_order_complex128(mode):
    """The level is real-linear: the derivative of <A^T v, w2> w.r.t. the cotangent v is A w2 — through the backward of the backward."""
    bank = host_taps("db4")
    for shape, ndim in (((2, 13), 1), ((2, 5, 7), 2), ((2, 33, 65), 2)):
        x64 = R.gauss(shape, 3 + sum(shape))

        def second(x, dec):
            x = x.requires_grad_(True)
            flat = R.flat(dec(x))
            vs = [w.to(x.device).requires_grad_(True) for w in _cotangents(flat, 5)]
            (g_x,) = torch.autograd.grad(flat, x, vs, create_graph=True)
            w2 = R.gauss(g_x.shape, 77).to(x.device)
            return g_x, torch.autograd.grad(g_x, vs, w2)

        want_g, want = second(x64.clone(), lambda t: R.wavedecn(t, bank, mode, ndim, 2))
        got_g, got = second(x64.clone().to(dev()), lambda t: R.api_to_ref(_DEC[ndim][0](t, "db4", mode=mode, level=2), ndim))
        _check(got_g, want_g, C128_GRAD_TOL, (mode, shape, "first order under create_graph"))
        for i, (a, b) in enumerate(zip(got, want)):
            _check(a, b, C128_GRAD_TOL, (mode, shape, "second order, cotangent %d" % i), "second order complex128")


@pytest.mark.parametrize("ndim", [1, 2])
def test_tap_gradients_of_a_learnable_bank(ndim):
    """A learnable REAL bank under complex data: the tap gradient is the sum of the two components' tap gradients."""
    shape = (3, 37) if ndim == 1 else (2, 13, 10)
    x64 = R.gauss(shape, 41)
    ref_dec = {1: A.wavedec, 2: A.wavedec2}[ndim]
    ref_rec = {1: A.waverec, 2: A.waverec2}[ndim]

    def run(x, bank, dec, rec, composed):
        bank = tuple(t.clone().requires_grad_(True) for t in bank)
        if composed:  # the reference: the differentiable real transform of each component
            cr, ci = dec(x.real, bank, mode="symmetric", level=2), dec(x.imag, bank, mode="symmetric", level=2)
            flat_r, flat_i = R.flat(R.api_to_ref(cr, ndim)), R.flat(R.api_to_ref(ci, ndim))
            flat = [torch.complex(a, b) for a, b in zip(flat_r, flat_i)]
            y = torch.complex(rec(cr, bank), rec(ci, bank))
        else:
            coeffs = dec(x, bank, mode="symmetric", level=2)
            flat = R.flat(R.api_to_ref(coeffs, ndim))
            y = rec(coeffs, bank)
        ws = [w.to(x.device) for w in _cotangents(flat, 9)]
        wy = R.gauss(y.shape, 10).to(x.device)
        loss = sum((c * w.conj()).real.sum() for c, w in zip(flat, ws)) + (y * wy.conj()).real.sum()
        return torch.autograd.grad(loss, bank)

    bank64 = tuple(torch.tensor(t, dtype=torch.float64) for t in host_taps("db2"))
    want = run(x64, bank64, ref_dec, ref_rec, True)
    ref32 = run(x64.to(torch.complex64), tuple(t.float() for t in bank64), ref_dec, ref_rec, True)
    e32 = max(_ext_ref.relerr(a, b) for a, b in zip(ref32, want))  # the reference's own float32 run of the same loss
    print("tap gradients, the reference's float32 error: %.3e" % e32)
    for dtype, tol in ((torch.complex128, C128_GRAD_TOL), (torch.complex64, 10 * e32)):
        comp = torch.float64 if dtype == torch.complex128 else torch.float32
        got = run(x64.to(dtype).to(dev()), tuple(t.to(comp).to(dev()) for t in bank64), _DEC[ndim][0], _DEC[ndim][1], False)
        for name, a, b in zip(("dec_lo", "dec_hi", "rec_lo", "rec_hi"), got, want):
            assert a.dtype == comp and not a.is_complex()
            err = _ext_ref.relerr(a, b)
            print("tap gradient", ndim, _name(dtype), name, "%.3e (bound %.1e)" % (err, tol))
            assert err < tol, (ndim, dtype, name, err)


# ---- 5. entry by entry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("mode", ["symmetric", "reflect"])
def test_operator_entry_by_entry(mode, dtype, fused_cells):
    """Real unit impulses through the fused level give the columns of its matrix in the real plane and exact zeros in the imaginary one,
    imaginary impulses the other way round: entry by entry the reference operator, and no entry couples the components."""
    bank = host_taps("db4")
    tol = 1e-12 if dtype == torch.complex128 else 2e-7  # (one rounding of a tap to float32: 6e-8 relative)
    for n in (13, 16):
        m = (n + 7) // 2
        want = _ext_ref.matrix(n, bank[0], bank[1], mode)  # [2 M, n]
        eye = torch.eye(n, dtype=torch.float64)
        for unit, part, other in ((1.0, "real", "imag"), (1j, "imag", "real")):
            before = _counts()
            buf = _cplx.level_fwd((eye * unit).to(dtype).to(dev()), bank[0], bank[1], _engine.MODE_IDS[mode])  # [n, 2, M]: row i = A e_i
            assert _delta(before) == [1, 0]
            a = getattr(buf, part).reshape(n, 2 * m).T.cpu().double()
            assert float((a - want).abs().max()) < tol * float(want.abs().max()), (mode, dtype, n, part, "level")
            assert not bool(getattr(buf, other).any()), (mode, dtype, n, part, "an entry couples the components")
        # the inverse: impulses on the coefficients give the columns of the synthesis matrix
        eye2 = torch.eye(2 * m, dtype=torch.float64).reshape(2 * m, 2, m)
        want_s = _ext_ref.level_inv([eye2[:, 0], eye2[:, 1]], bank, 1)[:, :n]  # [2 M, n]
        for unit, part, other in ((1.0, "real", "imag"), (1j, "imag", "real")):
            g = (eye2 * unit).to(dtype).to(dev())
            before = _counts()
            y = _cplx.level_inv([g[:, 0], g[:, 1]], bank[2], bank[3], (n,))
            assert _delta(before) == [0, 1]
            s = getattr(y, part).cpu().double()
            assert float((s - want_s).abs().max()) < tol * float(want_s.abs().max()), (mode, dtype, n, part, "inverse")
            assert not bool(getattr(y, other).any()), (mode, dtype, n, part, "an entry of the inverse couples the components")


# ---- 6. capture and canaries -----------------------------------------------------------------------------------------------------------
def test_capture_replays_to_the_same_bits(fused_cells):
    x = R.gauss((3, 45, 80), 8).to(torch.complex64).to(dev())
    x2 = R.gauss((3, 45, 80), 9).to(torch.complex64).to(dev())

    def flat(c):
        return [c[0]] + [t for lv in c[1:] for t in lv]

    fwd = ptwt_amd.capture(lambda t: ptwt_amd.wavedec2(t, "db4", mode="symmetric", level=2), x)
    eager_c = ptwt_amd.wavedec2(x2, "db4", mode="symmetric", level=2)
    eager = flat(eager_c)
    before = _counts()
    replay = flat(fwd(x2))
    torch.cuda.synchronize()
    assert _delta(before) == [0, 0]  # a replay enqueues nothing through the C ABI
    assert len(replay) == len(eager) == 7 and all(torch.equal(torch.view_as_real(a), torch.view_as_real(b)) for a, b in zip(replay, eager))
    inv = ptwt_amd.capture(lambda t: ptwt_amd.waverec2((t, *eager_c[1:]), "db4"), eager_c[0])
    y = inv(eager_c[0])
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(y), torch.view_as_real(ptwt_amd.waverec2(eager_c, "db4")))


@pytest.mark.parametrize("shape", [(5, 7), (33, 65), (67, 131)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_guard_regions_stay_intact(dtype, shape):
    """The outputs of ids 46 / 47 embedded in a poisoned allocation (two guard rows above and below, five / six guard columns left and
    right of every plane, guard images at both ends): every element outside keeps the pattern, every one inside is the reference's."""
    b, (h, w), poison = 3, shape, complex(-12345.5, 54321.25)
    mode, bank = "symmetric", host_taps("db4")
    flen = len(bank[0])
    mh, mw = (h + flen - 1) // 2, (w + flen - 1) // 2
    lib = _cplx._lib()
    ref = _cell(mode, "db4", (b, h, w))
    x = ref["x"].to(dtype).to(dev())
    g = torch.stack([t.to(dtype) for t in ref["g"]], 1).to(dev())
    lo, hi = _engine._taps_array(bank[0]), _engine._taps_array(bank[1])
    rlo, rhi = _engine._taps_array(bank[2]), _engine._taps_array(bank[3])
    stream = _engine._stream_of(x)

    def embedded(nout, eh, ew):
        block = torch.full((nout * b + 2, eh + 4, ew + 11), poison, dtype=dtype, device=dev())
        planes = [block[1 + q * b:1 + (q + 1) * b, 2:2 + eh, 5:5 + ew] for q in range(nout)]
        inside = torch.zeros(block.shape, dtype=torch.bool, device=dev())
        for q in range(nout):
            inside[1 + q * b:1 + (q + 1) * b, 2:2 + eh, 5:5 + ew] = True
        return block, planes, inside

    # id 46
    block, planes, inside = embedded(4, mh, mw)
    d = _cplx._desc(2, dtype, _engine.MODE_IDS[mode], flen, b, (h, w), x.stride(), (mh, mw), planes[0].stride(), planes[1].stride())
    _engine._check(lib.mifwt_cplx_fwd(ctypes.byref(d), x.data_ptr(), planes[0].data_ptr(), _engine._ptr_array(planes[1:]), lo, hi, stream))
    torch.cuda.synchronize()
    assert bool((block[~inside] == poison).all()), "id 46: a guard element was overwritten"
    for q in range(4):
        _check(planes[q], ref["fwd"][q], _tol(dtype, ref["e_fwd"]), ("guarded level", _name(dtype), shape, q))
    # id 47
    block, planes, inside = embedded(1, h, w)
    gs = (g.stride(0), g.stride(2), g.stride(3))
    d = _cplx._desc(2, dtype, 0, flen, b, (h, w), planes[0].stride(), (mh, mw), gs, gs)
    _engine._check(lib.mifwt_cplx_inv(ctypes.byref(d), g[:, 0].data_ptr(), _engine._ptr_array([g[:, s] for s in (1, 2, 3)]),
                                      planes[0].data_ptr(), rlo, rhi, stream))
    torch.cuda.synchronize()
    assert bool((block[~inside] == poison).all()), "id 47: a guard element was overwritten"
    _check(planes[0], ref["inv"], _tol(dtype, ref["e_inv"]), ("guarded inverse", _name(dtype), shape))


def test_print_worst():
    """Runs last (file order)."""
    print("\nworst norm-wise errors vs the complex128 reference:", {k: "%.2e" % v for k, v in sorted(WORST.items())})


def measure_reference_c64():
    """The complex64 reference's own gradient error over the gradient cases (host, no GPU): the yardstick of C64_GRAD_TOL."""
    worst = (0.0, None)
    for wavelet in GRAD_WAVELETS:
        for mode in GRAD_MODES:
            for shape, ndim in _grad_cases(mode, wavelet):
                bank = host_taps(wavelet)
                x64 = R.gauss(shape, sum(shape))
                g32, g64 = _ref_grad(x64, bank, mode, ndim, torch.complex64), _ref_grad(x64, bank, mode, ndim, torch.complex128)
                e = max([R.relerr(g32[0], g64[0])] + [R.relerr(a, b) for a, b in zip(g32[2], g64[2])])
                print(shape, wavelet, mode, "%.3e" % e)
                if e > worst[0]:
                    worst = (e, (shape, wavelet, mode))
    print("complex64 reference, worst gradient error: %.3e at %s" % worst)


if __name__ == "__main__":
    measure_reference_c64()
