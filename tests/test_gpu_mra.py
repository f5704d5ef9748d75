"""mra / imra on the GPU (kernels 63 / 64, csrc/mifwt_mra.hip): every component against the float64 reference of tests/_mra_ref.py.

Bounds, norm-wise per component (``tests._mra_ref.relerr``) plus the max-abs companion of tests/test_gpu_swt_kernels.py (10 x bound x the
largest value): float64 1e-12; float32 ``max(1e-6, 10 x e_ref32)``, ``e_ref32`` being the error of the reference's own float32
tap-by-tap run of the case.  An error is relative to the component's own norm (on white noise every component holds at least 0.03 of
``|x|`` at N >= 37); at N = 5 and 6, where a component can vanish, and for banks that are no wavelets, relative to ``|x|``.

Every test takes the launch whatever ``COMPOSED_CELLS`` routes to the composition by default (the fixture empties the table)."""
import importlib

import pytest
import torch

import ptwt_amd
from oracle import fwt_oracle as O
from ptwt_amd import _engine
from tests import _mra_ref as R

M = importlib.import_module("ptwt_amd.mra")  # (the package attribute of that name is the function)
pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
BANKS = ("haar", "db4", "bior2.2", "db10")
ROWS = 3
_REF: dict = {}


def dev():
    return torch.device("cuda:0")


def tag(v):
    return str(v).replace("torch.", "")


@pytest.fixture(autouse=True)
def launch_everywhere(monkeypatch):
    monkeypatch.setattr(M, "COMPOSED_CELLS", set())


def random_bank(flen=6, seed=5):
    g = torch.Generator().manual_seed(seed)
    return tuple([float(v) for v in torch.randn(flen, generator=g, dtype=F64)] for _ in range(4))


def data(n, dtype, rows=ROWS, seed=0):
    """White noise whose float32 and float64 forms hold the same values."""
    return torch.randn(rows, n, generator=torch.Generator().manual_seed(1000 * seed + n), dtype=F32).to(dtype)


def reference(x, wavelet, level, transform, mode):
    """(float64 components, e_ref32 of the case), computed once per case and shared."""
    key = (tuple(x.shape), float(x.double().sum()), str(wavelet), level, transform, mode)
    if key not in _REF:
        x64 = x.double()
        scale = float(x64.norm())
        want = R.mra(x64, wavelet, level, transform, mode)
        e32 = R.e_ref32(lambda t: R.mra(t, wavelet, level, transform, mode), x64, scale=0.0 if _own_norm(x, wavelet) else scale)
        _REF[key] = (want, e32)
    return _REF[key]


def _own_norm(x, wavelet):
    return x.shape[-1] >= 37 and isinstance(wavelet, str)


def check(parts, x, wavelet, level, transform="swt", mode="periodization", what=""):
    want, e32 = reference(x.cpu(), wavelet, level, transform, mode)
    tol = 1e-12 if x.dtype == F64 else max(1e-6, 10 * e32)
    assert len(parts) == len(want), what
    scale = float(x.double().norm())
    peak = float(x.abs().max())
    for i, (p, w) in enumerate(zip(parts, want)):
        assert p.shape == x.shape and p.dtype == x.dtype and p.device == x.device, (what, i)
        p = p.double().cpu()
        own = _own_norm(x, wavelet)
        den = float(w.norm()) if own else scale
        err = float((p - w).norm()) / den
        top = max(float(w.abs().max()) if own else peak, 1e-30)
        worst = float((p - w).abs().max())
        print(f"{what} component {i}: {err:.3e} (bound {tol:.1e}), max-abs {worst / top:.3e}")
        assert err < tol, (what, i, err, tol)
        assert worst <= 10 * tol * top, (what, i, "max-abs", worst, top)


# ---- stationary ------------------------------------------------------------------------------------------------------------------------
def swt_lengths():
    t = M.tile()
    return (5, 6, 37, 64, 1000, t - 1, t + 1, 2 * t + 3)


@pytest.mark.parametrize("dtype", [F32, F64], ids=tag)
@pytest.mark.parametrize("wavelet", BANKS + ("db11", "random6"))
def test_stationary_components(wavelet, dtype):
    """Every length at levels 1 and 3: rows shorter than a window (many wraps), no multiple of anything, one tile, tile - 1, tile + 1,
    three tiles.  db11 is composed; ``random6`` is four independent random filters."""
    bank = random_bank() if wavelet == "random6" else wavelet
    for n in swt_lengths():
        for level in (1, 3):
            x = data(n, dtype).to(dev())
            check(ptwt_amd.mra(x, bank, level), x, bank, level, what=f"swt {wavelet} {tag(dtype)} N={n} level={level}")


@pytest.mark.parametrize("dtype", [F32, F64], ids=tag)
@pytest.mark.parametrize("wavelet,n", [("haar", 4099), ("db4", 2304), ("db10", 1000)])
def test_the_last_depth_of_the_envelope_and_one_past_it(wavelet, n, dtype):
    """At the deepest level the launch takes, all components are one launch; one level deeper, S_n and D_n are composed and the rest
    of the call stays on the launch."""
    deepest = M.max_depth(dtype, len(R.bank_of(wavelet)[0]))
    x = data(n, dtype).to(dev())
    for level in (deepest, deepest + 1):
        _engine.level_events = []
        try:
            parts = ptwt_amd.mra(x, wavelet, level)
            kids = [e[1] for e in _engine.level_events]
        finally:
            _engine.level_events = None
        assert kids.count(M.KID_MRA_SWT) == 1, kids
        check(parts, x, wavelet, level, what=f"swt {wavelet} {tag(dtype)} N={n} level={level}")


# ---- decimated -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64], ids=tag)
@pytest.mark.parametrize("mode", ["reflect", "zero", "periodization", "smooth"])
@pytest.mark.parametrize("wavelet", BANKS)
def test_decimated_components(wavelet, mode, dtype):
    """N = 37, 64, 1001 (odd extents: levels one sample short of their full synthesis) and three tiles, at levels 1, 3 and 5 where
    ``dwt_max_level`` allows them."""
    flen = len(R.bank_of(wavelet)[0])
    ran = 0
    for n in (37, 64, 1001, 2 * M.tile() + 3):
        for level in (1, 3, 5):
            if level > O.dwt_max_level(n, flen):
                continue
            x = data(n, dtype).to(dev())
            parts = ptwt_amd.mra(x, wavelet, level, transform="dwt", mode=mode)
            check(parts, x, wavelet, level, "dwt", mode, what=f"dwt {wavelet} {mode} {tag(dtype)} N={n} level={level}")
            ran += 1
    assert ran >= 5


def test_decimated_default_mode_is_periodization():
    x = data(64, F64).to(dev())
    check(ptwt_amd.mra(x, "db2", 2, transform="dwt"), x, "db2", 2, "dwt", "periodization", what="default mode")


# ---- layouts ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform,mode", [("swt", "periodization"), ("dwt", "periodization"), ("dwt", "reflect")])
@pytest.mark.parametrize("dtype", [F32, F64], ids=tag)
def test_views_axes_and_batches(dtype, transform, mode):
    n = 2 * M.tile() + 6
    base = data(n + 9, dtype, rows=4).to(dev())
    kw = {"transform": transform, "mode": mode}

    def ref(x, axis=-1):
        want, _ = reference(x.movedim(axis, -1).reshape(-1, x.shape[axis]).cpu(), "db4", 2, transform, mode)
        lead = list(x.movedim(axis, -1).shape)
        return [w.reshape(lead).movedim(-1, axis) for w in want]

    def same(parts, want, what):
        tol = 1e-12 if dtype == F64 else 1e-6
        for p, w in zip(parts, want):
            assert p.shape == w.shape
            assert R.relerr(p, w) < tol, what

    rows = base[1:, 5:5 + n]  # rows of a wider tensor: a row stride that is not the length
    assert not rows.is_contiguous()
    same(ptwt_amd.mra(rows, "db4", 2, **kw), ref(rows), "row view")
    every_other = base[:, ::2]  # a non-unit innermost stride
    same(ptwt_amd.mra(every_other, "db4", 2, **kw), ref(every_other), "strided view")
    cols = data(300, dtype, rows=3).to(dev()).t()  # [300, 3], the transform along axis 0
    same(ptwt_amd.mra(cols, "db4", 2, axis=0, **kw), ref(cols, 0), "axis 0")
    batch = data(200, dtype, rows=6, seed=2).to(dev()).reshape(2, 3, 200)
    same(ptwt_amd.mra(batch, "db4", 2, **kw), ref(batch), "3-D batch")
    mid = batch.transpose(1, 2).contiguous()  # [2, 200, 3]
    same(ptwt_amd.mra(mid, "db4", 2, axis=1, **kw), [w.transpose(1, 2) for w in ref(batch)], "axis 1 of 3")
    one = batch[0, 0]  # a 1-D signal
    same(ptwt_amd.mra(one, "db4", 2, **kw), ref(one), "1-D")


# ---- launches --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform,kid", [("swt", 63), ("dwt", 64)])
def test_one_launch_after_the_analysis(transform, kid):
    x = data(512, F32).to(dev())
    kw = {"transform": transform, "mode": "reflect"}
    ptwt_amd.mra(x, "db4", 3, **kw)
    _engine.level_events = []
    try:
        fused = ptwt_amd.mra(x, "db4", 3, **kw)
        events = list(_engine.level_events)
        _engine.level_events = []
        M.FORCE_COMPOSED = True
        composed = ptwt_amd.mra(x, "db4", 3, **kw)
        events_composed = list(_engine.level_events)
    finally:
        M.FORCE_COMPOSED = False
        _engine.level_events = None
    kids = [e[1] for e in events]
    assert kids.count(kid) == 1 and kids[-1] == kid and events[-1][0] == "mra_" + transform, kids
    assert 63 not in kids[:-1] and 64 not in kids[:-1]
    assert not any(e[1] in (63, 64) for e in events_composed)
    direct = M._composed(x, "db4", 3, -1, transform, "reflect")
    for f, c, d in zip(fused, composed, direct):
        assert torch.equal(c, d)
        assert R.relerr(f, c) < 1e-6
    # the entries of the launch's result share one allocation
    assert fused[1].data_ptr() - fused[0].data_ptr() == x.numel() * x.element_size()


def test_routing_table_sends_a_cell_to_the_composition(monkeypatch):
    x = data(512, F32).to(dev())
    monkeypatch.setattr(M, "COMPOSED_CELLS", {("swt", F32, "short")})
    _engine.level_events = []
    try:
        ptwt_amd.mra(x, "db4", 2)
        short = [e[1] for e in _engine.level_events]
        _engine.level_events = []
        ptwt_amd.mra(data(M.tile() + 1, F32).to(dev()), "db4", 2)
        long = [e[1] for e in _engine.level_events]
    finally:
        _engine.level_events = None
    assert 63 not in short and long.count(63) == 1


def test_calls_that_are_composed():
    """16-bit and complex data, data that requires grad: the composition's result, no launch of ids 63 / 64."""
    x = data(256, F32).to(dev())
    _engine.level_events = []
    try:
        with pytest.raises(ValueError, match="not supported"):  # (16-bit storage is opt-in: the analysis call's refusal)
            ptwt_amd.mra(x.to(torch.bfloat16), "db2", 2)
        with ptwt_amd.half_storage():
            half = ptwt_amd.mra(x.to(torch.bfloat16), "db2", 2)
        z = ptwt_amd.mra(torch.complex(x, x.flip(-1)), "db2", 2, transform="dwt", mode="zero")
        xg = x.double().requires_grad_(True)
        with_grad = ptwt_amd.mra(xg, "db2", 2)
        kids = [e[1] for e in _engine.level_events]
    finally:
        _engine.level_events = None
    assert 63 not in kids and 64 not in kids
    assert half[0].dtype == torch.bfloat16 and z[0].dtype == torch.complex64 and with_grad[0].requires_grad
    want, _ = reference(x.cpu(), "db2", 2, "dwt", "zero")
    for p, w in zip(z, want):
        assert R.relerr(p.real, w) < 1e-6
    with torch.no_grad():
        plain = ptwt_amd.mra(xg, "db2", 2)
    for p, q in zip(with_grad, plain):
        assert R.relerr(p, q) < 1e-12


def test_capture_replays_to_the_same_bits():
    for transform in ("swt", "dwt"):
        a, b = data(3000, F32, seed=3).to(dev()), data(3000, F32, seed=4).to(dev())
        call = ptwt_amd.capture(lambda t: ptwt_amd.mra(t, "db4", 3, transform=transform), a)
        got = call.cloned(b)
        want = ptwt_amd.mra(b, "db4", 3, transform=transform)
        assert all(torch.equal(p, q) for p, q in zip(got, want))
        again = call.cloned(a)
        assert all(torch.equal(p, q) for p, q in zip(again, ptwt_amd.mra(a, "db4", 3, transform=transform)))
        assert not torch.equal(got[0], again[0])


@pytest.mark.parametrize("dtype,tol", [(F32, 1e-6), (F64, 1e-13)], ids=["float32", "float64"])
def test_imra_inverts_mra(dtype, tol):
    for transform, mode, n in (("swt", "periodization", 4100), ("dwt", "periodization", 4099), ("dwt", "smooth", 1001)):
        x = data(n, dtype).to(dev())
        y = ptwt_amd.imra(ptwt_amd.mra(x, "db4", 4, transform=transform, mode=mode))
        assert y.shape == x.shape and y.dtype == dtype
        assert R.relerr(y, x) < tol, (transform, mode, R.relerr(y, x))


@pytest.mark.parametrize("transform,mode", [("swt", "periodization"), ("dwt", "periodization"), ("dwt", "reflect")])
def test_data_gradients_against_float64_autograd_of_the_reference(transform, mode):
    x = data(101 if transform == "dwt" else 96, F64).to(dev()).requires_grad_(True)
    parts = ptwt_amd.mra(x, "db3", 3, transform=transform, mode=mode)
    g = torch.Generator().manual_seed(9)
    ws = [torch.randn(p.shape, generator=g, dtype=F64) for p in parts]
    (got,) = torch.autograd.grad(sum((w.to(dev()) * p).sum() for w, p in zip(ws, parts)), x)
    xr = x.detach().cpu().requires_grad_(True)
    (want,) = torch.autograd.grad(sum((w * p).sum() for w, p in zip(ws, R.mra(xr, "db3", 3, transform, mode))), xr)
    assert R.relerr(got, want) < 1e-10


# ---- canaries --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transform", ["swt", "dwt"])
def test_the_binding_writes_its_tile_of_a_block_and_nothing_else(transform):
    """The private binding writing components of [rows, n] into the middle of a pattern-filled block [comps + 2, rows + 2, n + 16]."""
    rows, n, level, sentinel = 3, M.tile() + 37, 2, -12345.678
    x = data(n, F64).to(dev())
    bank = R.bank_of("db4")
    coeffs = ptwt_amd.swt(x, "db4", level) if transform == "swt" else ptwt_amd.wavedec(x, "db4", mode="zero", level=level)
    nb = level + 1
    block = torch.full((nb + 2, rows + 2, n + 16), sentinel, dtype=F64, device=dev())
    out = block[1:1 + nb, 1:1 + rows, 8:8 + n]
    depths = [level] + [nb - i for i in range(1, nb)]
    level_len = None if transform == "swt" else [n] + [int(c.shape[-1]) for c in coeffs[:0:-1]]
    assert M._project(list(coeffs), depths, level_len, n, bank[2], bank[3], out=out) is out
    torch.cuda.synchronize()
    want, _ = reference(x.cpu(), "db4", level, transform, "zero")
    for i, w in enumerate(want):
        assert R.relerr(out[i], w) < 1e-12
    mask = torch.ones_like(block, dtype=torch.bool)
    mask[1:1 + nb, 1:1 + rows, 8:8 + n] = False
    assert bool((block[mask] == sentinel).all())


# ---- past 2^31 elements ----------------------------------------------------------------------------------------------------------------
def test_output_past_2_to_the_31_elements():
    """``mra`` of [2^18 + 2, 4100] float32 at level 1: two components, 2^31 + 2 113 552 elements in all (8 GiB, next to 4 GiB of data and
    8 GiB of coefficients); the first, the last and a dozen sampled rows against the reference run on those rows alone."""
    free = torch.cuda.mem_get_info()[0]
    if free < 24 << 30:
        pytest.skip(f"mra past 2^31: 24 GiB needed, {free / 2 ** 30:.1f} GiB free")
    rows, n = (1 << 18) + 2, 4100
    assert 2 * rows * n > 1 << 31
    x = torch.empty((rows, n), dtype=F32, device=dev())
    x.normal_(generator=torch.Generator(device=dev()).manual_seed(71))
    parts = ptwt_amd.mra(x, "db2", 1)
    pick = [0, rows - 1] + [int(v) for v in torch.randint(1, rows - 1, (12,), generator=torch.Generator().manual_seed(72))]
    sample = x[pick].cpu()
    want = R.mra(sample.double(), "db2", 1)
    for p, w in zip(parts, want):
        assert p.shape == (rows, n)
        assert R.relerr(p[pick], w) < 1e-6
    del parts, x
