"""coeffs_to_array / array_to_coeffs / ravel_coeffs / unravel_coeffs on the GPU (kernels 59 / 60) against tests/_pack_ref.py on the
``.cpu()`` copies of the same coefficient tensors.  Every comparison is bit-exact: a copy has no tolerance.  The launch events pin that
kernel 59 / 60 ran, once per call inside the capacity of a launch.  The padding is -7.5, so a gap filled wrongly or not at all shows."""
import importlib

import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine
from ptwt_amd.constants import WaveletDetailTuple2d
from tests import _pack_ref as R

pytestmark = pytest.mark.gpu

C = importlib.import_module("ptwt_amd.coeff_array")
PAD = -7.5
ROUTED = set(C.COMPOSED_CELLS)


@pytest.fixture(autouse=True)
def kernels_everywhere(monkeypatch):
    """The tests are about kernels 59 / 60: the cells that the routing rule sends to the composition run on the kernels here."""
    monkeypatch.setattr(C, "COMPOSED_CELLS", set())


def dev():
    return torch.device("cuda:0")


def _x(*shape, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g, dtype=torch.float64)
    if dtype.is_complex:
        x = torch.complex(x, torch.randn(*shape, generator=g, dtype=torch.float64))
    return x.to(dtype).to(dev())


def events(fn):
    """(result, ids of the kernels 59 / 60 that ran)."""
    _engine.level_events = []
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, [e[1] for e in _engine.level_events if e[1] in (59, 60)]
    finally:
        _engine.level_events = None


def fmt_of(coeffs):
    e = coeffs[1] if len(coeffs) > 1 else None
    return "wavedec" if isinstance(e, torch.Tensor) or e is None else "wavedecn" if isinstance(e, dict) else "wavedec2"


def check(coeffs, axes=None, padding=PAD, launches=1):
    """All four calls, both copy variants and the round trips of one container against the reference."""
    ref = R.cpu(coeffs)
    fmt = fmt_of(coeffs)
    want, wslices = R.to_array(ref, padding, axes)
    (arr, slices), ids = events(lambda: ptwt_amd.coeffs_to_array(coeffs, padding, axes=axes))
    assert ids == [59] * launches and slices == wslices
    assert R.same_bits(arr, want) and arr.is_contiguous() and arr.device == coeffs[0].device
    wflat, wsl, wsh = R.ravel(ref, axes)
    (flat, rsl, shapes), ids = events(lambda: ptwt_amd.ravel_coeffs(coeffs, axes=axes))
    assert ids == [59] * launches and (rsl, shapes) == (wsl, wsh) and R.same_bits(flat, wflat) and flat.is_contiguous()
    for copy in (False, True):
        back, ids = events(lambda: ptwt_amd.array_to_coeffs(arr, slices, fmt, copy=copy))
        assert ids == ([60] * launches if copy and arr.numel() else [])
        assert R.same_container(back, ref)  # the round trip: bit for bit the container that went in
        rback, ids = events(lambda: ptwt_amd.unravel_coeffs(flat, rsl, shapes, fmt, copy=copy))
        assert ids == ([60] * launches if copy and arr.numel() else [])
        want_r = R.unravel(wflat, wsl, wsh)
        got_a, got_l = R.levels(rback)
        assert R.same_bits(got_a, want_r[0]) and all(R.same_bits(g[k], w[k]) for g, w in zip(got_l, want_r[1:]) for k in w)
        if axes is None:
            assert R.same_container(rback, ref, ordered=False)  # (the keys of a level come back in sorted order)
        if copy:
            for c in (back, rback):
                leaves = [c[0]] + [t for lv in R.levels(c)[1] for t in lv.values()]
                base = leaves[0].untyped_storage().data_ptr()
                for t in leaves:  # dense, 256-byte aligned starts, one storage
                    assert t.is_contiguous() and t.data_ptr() % 256 == 0 and t.untyped_storage().data_ptr() == base
                if arr.numel():  # (fresh memory; empty tensors have no storage to tell apart)
                    assert leaves[0].untyped_storage().data_ptr() not in (arr.untyped_storage().data_ptr(), flat.untyped_storage().data_ptr())
    return arr, slices


# ---- containers straight from the transforms: strided views, odd extents ------------------------------------------------------------------------
@pytest.mark.parametrize("shape,wavelet,mode,level", [((3, 37), "db4", "symmetric", 3), ((2, 1001), "db4", "symmetric", 3),
                                                      ((2, 64), "haar", "zero", 3), ((3, 64), "db4", "periodization", 3)])
def test_wavedec(shape, wavelet, mode, level):
    check(ptwt_amd.wavedec(_x(*shape), wavelet, mode=mode, level=level), padding=None)  # 1-D is always tight


SHAPES_2D = [((3, 23, 37), "db2", 2), ((3, 23, 37), "db4", 3), ((2, 64, 65), "db2", 3), ((2, 64, 65), "db4", 2)]


@pytest.mark.parametrize("shape,wavelet,level", SHAPES_2D)
def test_wavedec2(shape, wavelet, level):
    c = ptwt_amd.wavedec2(_x(*shape), wavelet, mode="symmetric", level=level)
    assert not c[1].horizontal.is_contiguous()
    check(c)
    with pytest.raises(ValueError, match="padding=None asks for tight packing"):
        ptwt_amd.coeffs_to_array(c, None)
    # waverec2 of the unpacked container: the fresh dense tensors of copy=True from either layout, and the views of the flat layout
    y = ptwt_amd.waverec2(c, wavelet)
    arr, slices = ptwt_amd.coeffs_to_array(c, PAD)
    assert torch.equal(ptwt_amd.waverec2(ptwt_amd.array_to_coeffs(arr, slices, "wavedec2", copy=True), wavelet), y)
    for copy in (False, True):
        assert torch.equal(ptwt_amd.waverec2(ptwt_amd.unravel_coeffs(*ptwt_amd.ravel_coeffs(c), "wavedec2", copy=copy), wavelet), y)


@pytest.mark.parametrize("shape,wavelet,level", SHAPES_2D + [((4, 512, 512), "db4", 3)])
def test_waverec2_of_the_array_views(shape, wavelet, level):
    """``waverec2(array_to_coeffs(arr, slices, copy=False))`` against ``waverec2(c)``: the same kernels and the same bits.  The views carry
    the array's row pitch, which the one-launch small-plane synthesis (kernel id 21) does not read: ``waverec2`` copies such small planes
    and takes the launch it takes for ``c``.  At 4x512x512 every layout takes the streaming kernel 22."""
    c = ptwt_amd.wavedec2(_x(*shape), wavelet, mode="symmetric", level=level)
    arr, slices = ptwt_amd.coeffs_to_array(c, PAD)
    views = ptwt_amd.array_to_coeffs(arr, slices, "wavedec2")
    assert R.same_container(views, R.cpu(c))
    runs = []
    for coeffs in (views, c):
        _engine.level_events = []
        try:
            runs.append((ptwt_amd.waverec2(coeffs, wavelet), [e[1] for e in _engine.level_events if e[0] == "inv"]))  # the synthesis launches
        finally:
            _engine.level_events = None
    (got, got_ids), (want, want_ids) = runs
    assert got_ids == want_ids == ([22] if shape[-1] == 512 else [21])
    assert torch.equal(got, want)


def test_wavedec3_and_fswavedec2():
    c3 = ptwt_amd.wavedec3(_x(2, 9, 10, 11), "db2", mode="symmetric", level=2)
    arr, _ = check(c3)
    assert arr.shape == (2, 4 + 4 + 6, 4 + 4 + 6, 5 + 5 + 7)
    fs = ptwt_amd.fswavedec2(_x(3, 23, 37, seed=1), "db2", mode="symmetric", level=2)
    assert list(fs[1]) == ["da", "ad", "dd"]
    _, slices = check(fs)
    assert list(slices[1]) == ["da", "ad", "dd"]


@pytest.mark.parametrize("wavelet,mode", [("haar", "zero"), ("db4", "periodization"), ("haar", "periodization")])
def test_tight_containers_take_padding_none(wavelet, mode):
    c = ptwt_amd.wavedec2(_x(2, 32, 48), wavelet, mode=mode, level=3)
    arr, _ = check(c, padding=None)
    assert arr.shape == (2, 32, 48)
    arr, _ = check(ptwt_amd.wavedec3(_x(2, 8, 16, 8), wavelet, mode=mode, level=2), padding=None)
    assert arr.shape == (2, 8, 16, 8)


def test_axes_0_2():
    x = _x(23, 3, 37)  # [H, B, W]
    c = ptwt_amd.wavedec2(x, "db2", mode="symmetric", level=2, axes=(0, 2))
    arr, slices = check(c, axes=(0, 2))
    assert arr.shape[1] == 3 and slices[1]["da"][1] == slice(None)


@pytest.mark.parametrize("lead", [(), (1,), (2, 3), (0,)], ids=["none", "one", "2x3", "empty"])
def test_leading_shapes(lead):
    x = _x(*lead, 23, 37)
    c = ptwt_amd.wavedec2(x, "db2", mode="symmetric", level=2) if 0 not in lead else (
        x[..., :7, :11], WaveletDetailTuple2d(*[x[..., :7, :11]] * 3), WaveletDetailTuple2d(*[x[..., :12, :19]] * 3))
    arr, _ = check(c, launches=0 if 0 in lead else 1)
    assert arr.shape[:len(lead)] == lead


def test_level_0():
    x = _x(3, 20)
    for c in (ptwt_amd.wavedec(x, "db2", level=0), ptwt_amd.wavedec2(x, "db2", level=0)):
        assert len(c) == 1
        (arr, slices), ids = events(lambda: ptwt_amd.coeffs_to_array(c, PAD))
        assert arr is c[0] and slices == [(slice(None), slice(None))] and ids == []
        (flat, rsl, shapes), ids = events(lambda: ptwt_amd.ravel_coeffs(c))
        assert flat is c[0] and ids == []
        for copy in (False, True):
            assert ptwt_amd.array_to_coeffs(arr, slices, "wavedec2", copy=copy)[0] is arr
            assert ptwt_amd.unravel_coeffs(flat, rsl, shapes, "wavedec", copy=copy)[0] is flat


def test_bands_sliced_with_a_step_along_the_batch():
    c = ptwt_amd.wavedec2(_x(5, 23, 37), "db4", mode="symmetric", level=2)
    stepped = (c[0][::2], *[WaveletDetailTuple2d(*[t[::2] for t in e]) for e in c[1:]])
    assert stepped[1].vertical.stride(0) == 2 * c[1].vertical.stride(0)
    check(stepped)
    c1 = ptwt_amd.wavedec(_x(6, 101), "db2", mode="symmetric", level=2)
    check([t[1::3] for t in c1], padding=None)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.complex64, torch.complex128, torch.float16, torch.bfloat16],
                         ids=["f32", "f64", "c64", "c128", "f16", "bf16"])
def test_all_six_dtypes(dtype):
    x = _x(2, 23, 37, dtype=dtype)
    if dtype in (torch.float16, torch.bfloat16):
        with ptwt_amd.half_storage():
            c = ptwt_amd.wavedec2(x, "db2", mode="symmetric", level=2)
            c1 = ptwt_amd.wavedec(x, "db2", mode="symmetric", level=2)
    else:
        c = ptwt_amd.wavedec2(x, "db2", mode="symmetric", level=2)
        c1 = ptwt_amd.wavedec(x, "db2", mode="symmetric", level=2)
    assert c[0].dtype == dtype
    arr, _ = check(c)
    assert arr.dtype == dtype
    check(c1, padding=None)


def test_level_4_wavedec3_takes_two_launches():
    c = ptwt_amd.wavedec3(_x(2, 16, 16, 16), "haar", level=4)
    assert 1 + 7 * 4 == 29 > C.max_tensors()
    arr, _ = check(c, padding=None, launches=2)
    assert arr.shape == (2, 16, 16, 16)


@pytest.mark.parametrize("w", [1, 2, 3])
def test_bands_narrower_than_one_vector(w):
    r = lambda *s: _x(*s, seed=w + sum(s))
    for dtype in (torch.float32, torch.float16):
        bands = lambda h, ww: WaveletDetailTuple2d(*[r(2, 4, h, ww).to(dtype)[:, k + 1] for k in range(3)])
        c = (r(2, 2, w).to(dtype), bands(2, w), bands(3, w + 1), bands(5, 2 * w + 1))
        arr, _ = check(c)
        assert arr.shape == (2, 12, 5 * w + 2)
    c1 = [r(3, w), r(3, 2, w)[:, 1], r(3, 2, w + 1)[:, 1]]
    check(c1, padding=None)


# ---- gradients -------------------------------------------------------------------------------------------------------------------------------
def _grad_case(dtype=torch.float32):
    c = ptwt_amd.wavedec2(_x(2, 23, 37, dtype=torch.complex64 if dtype.is_complex else torch.float32), "db2", mode="symmetric", level=2)
    leaves = [c[0].to(dtype).clone().requires_grad_(True)] + [t.to(dtype).clone().requires_grad_(True) for e in c[1:] for t in e]
    it = iter(leaves)
    return (next(it), *[WaveletDetailTuple2d(next(it), next(it), next(it)) for _ in c[1:]]), leaves


@pytest.mark.parametrize("dtype", [torch.float32, torch.complex64, torch.bfloat16], ids=["f32", "c64", "bf16"])
def test_gradients_are_the_slices_of_the_incoming_gradient(dtype):
    c, leaves = _grad_case(dtype)
    (arr, slices), ids = events(lambda: ptwt_amd.coeffs_to_array(c, PAD))
    assert ids == [59] and arr.requires_grad
    g = _x(*arr.shape, dtype=dtype, seed=5)
    grads = torch.autograd.grad(arr, leaves, g)
    want = R.from_array(g.cpu(), R.to_array(R.cpu(c))[1])
    flat_want = [want[0]] + [lv[k] for lv in want[1:] for k in ("da", "ad", "dd")]
    assert all(R.same_bits(a, b) for a, b in zip(grads, flat_want))
    flat, rsl, shapes = ptwt_amd.ravel_coeffs(c)
    g = _x(*flat.shape, dtype=dtype, seed=6)
    grads = torch.autograd.grad(flat, leaves, g)
    want = R.unravel(g.cpu(), rsl, shapes)
    flat_want = [want[0]] + [lv[k] for lv in want[1:] for k in ("da", "ad", "dd")]
    assert all(R.same_bits(a, b) for a, b in zip(grads, flat_want))


def test_gradients_of_the_copies_and_of_second_order():
    c, leaves = _grad_case()
    arr, slices = ptwt_amd.coeffs_to_array(c, PAD)
    w = _x(*arr.shape, seed=7)
    for fn in (lambda a: ptwt_amd.array_to_coeffs(a, slices, "wavedec2", copy=True),
               lambda a: ptwt_amd.unravel_coeffs(*ptwt_amd.ravel_coeffs(ptwt_amd.array_to_coeffs(a, slices, "wavedec2")), "wavedec2", copy=True)):
        a = arr.detach().clone().requires_grad_(True)
        back, ids = events(lambda: fn(a))
        assert 60 in ids
        gs = [_x(*t.shape, seed=8 + i) for i, t in enumerate([back[0]] + [t for e in back[1:] for t in e])]
        (ga,) = torch.autograd.grad([back[0]] + [t for e in back[1:] for t in e], a, gs)
        it = iter(g.cpu() for g in gs)
        want, _ = R.to_array((next(it), *[WaveletDetailTuple2d(next(it), next(it), next(it)) for _ in back[1:]]), 0.0)
        assert R.same_bits(ga, want)
    # create_graph: the gradient of (arr * arr * w).sum() is 2 arr w on the blocks; its gradient w.r.t. the leaves again 2 w on them
    loss = (arr * arr * w).sum()
    first = torch.autograd.grad(loss, leaves, create_graph=True)
    assert all(f.requires_grad for f in first)
    second = torch.autograd.grad(sum((f * f).sum() for f in first), leaves)
    wb = R.from_array(w.cpu(), slices)
    wl = [wb[0]] + [lv[k] for lv in wb[1:] for k in ("da", "ad", "dd")]
    for s, f, x, ww in zip(second, first, leaves, wl):
        assert R.same_bits(f, 2 * x.detach().cpu() * ww) and R.same_bits(s, 2 * (2 * x.detach().cpu() * ww) * (2 * ww))


# ---- capture -----------------------------------------------------------------------------------------------------------------------------------
def test_capture_replays_on_new_data():
    fn = lambda t: ptwt_amd.coeffs_to_array(ptwt_amd.wavedec2(t, "db2", level=2))[0]
    cap = ptwt_amd.capture(fn, _x(3, 40, 52))
    x = _x(3, 40, 52, seed=11)
    got = cap(x).clone()
    assert torch.equal(got, fn(x)) and not torch.equal(got, fn(_x(3, 40, 52)))
    flat = ptwt_amd.capture(lambda t: ptwt_amd.ravel_coeffs(ptwt_amd.wavedec2(t, "db2", level=2))[0], x)
    assert torch.equal(flat(x), ptwt_amd.ravel_coeffs(ptwt_amd.wavedec2(x, "db2", level=2))[0])


def test_composed_cells_take_the_composition(monkeypatch):
    monkeypatch.setattr(C, "COMPOSED_CELLS", ROUTED)
    assert ("coeffs_to_array", torch.float32, 1, False) in ROUTED
    c = ptwt_amd.wavedec(_x(2, 1001), "db4", mode="symmetric", level=3)  # (finest rows of 504 elements: not short)
    (arr, slices), ids = events(lambda: ptwt_amd.coeffs_to_array(c, PAD))
    assert ids == [] and R.same_bits(arr, R.to_array(R.cpu(c), PAD)[0])
    (flat, rsl, shapes), ids = events(lambda: ptwt_amd.ravel_coeffs(c))
    assert ids == [] and R.same_bits(flat, R.ravel(R.cpu(c))[0])
    for back, ids in (events(lambda: ptwt_amd.array_to_coeffs(arr, slices, "wavedec", copy=True)),
                      events(lambda: ptwt_amd.unravel_coeffs(flat, rsl, shapes, "wavedec", copy=True))):
        assert ids == [] and R.same_container(back, R.cpu(c)) and all(t.is_contiguous() for t in back)
