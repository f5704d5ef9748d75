"""coeffs_to_array / array_to_coeffs / ravel_coeffs / unravel_coeffs / wavedecn_shapes without a GPU: slices and shapes pinned by hand,
the reference (tests/_pack_ref.py) against a deliberately wrong layout, a CPU model of the kernels' box map — every destination element
written once — against the reference, the copy=False views, the shapes of the committed PyWavelets goldens, the API surface, the
host-only answers of the C ABI and every argument error that fires before a device is needed."""
import importlib
import itertools
import os
import re

import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine
from ptwt_amd.constants import WaveletDetailTuple2d
from tests import _golden as G
from tests import _pack_ref as R
from tests import _per_ref

C = importlib.import_module("ptwt_amd.coeff_array")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS3 = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")


def _gen(seed=0):
    g = torch.Generator().manual_seed(seed)
    return lambda *shape, dtype=torch.float32: torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)


def _views(r, lead, ext, nb, dtype=torch.float32):
    """``nb`` bands as the transforms hand them out: strided views of one level buffer [*lead, nb + 1, *ext]."""
    buf = r(*lead, nb + 1, *ext, dtype=dtype)
    return [buf.select(len(lead), k + 1) for k in range(nb)]


def dec1(lead=(3,), a=8, lens=(8, 9, 11), dtype=torch.float32, seed=1):
    r = _gen(seed)
    return [r(*lead, a, dtype=dtype)] + [_views(r, lead, (n,), 1, dtype)[0] for n in lens]


def dec2(lead=(2,), a=(3, 4), ext=((3, 4), (5, 7)), dtype=torch.float32, seed=2):
    r = _gen(seed)
    return (r(*lead, *a, dtype=dtype), *[WaveletDetailTuple2d(*_views(r, lead, e, 3, dtype)) for e in ext])


def dec3(lead=(2,), a=(2, 3, 2), ext=((2, 3, 2), (3, 5, 4)), seed=3, keys=KEYS3):
    r = _gen(seed)
    return (r(*lead, *a), *[dict(zip(keys, _views(r, lead, e, 7))) for e in ext])


def _s(*spans):
    return tuple(slice(None) if s is None else slice(*s) for s in spans)


# ---- slices and shapes by hand ---------------------------------------------------------------------------------------------------------
def test_layout_1d_16_samples_8_taps_three_padded_levels():
    c = dec1()
    assert [t.shape[-1] for t in c] == [8, 8, 9, 11]  # floor((n + 7) / 2) from 16: 11, 9, 8
    p = C._parse("t", c, None)
    shape, slices, regions, gaps = C._array_layout("t", p, True)  # 1-D is always tight
    assert shape == (3, 36) and gaps == [[], [], []]
    assert slices == [_s(None, (0, 8)), {"d": _s(None, (8, 16))}, {"d": _s(None, (16, 25))}, {"d": _s(None, (25, 36))}]
    lead, n, rsl, shapes = C._ravel_layout(p)
    assert (lead, n) == ((3,), 36)
    assert rsl == [slice(0, 8), {"d": slice(8, 16)}, {"d": slice(16, 25)}, {"d": slice(25, 36)}]
    assert shapes == [(8,), {"d": (8,)}, {"d": (9,)}, {"d": (11,)}]
    arr, rs = R.to_array(c)
    assert rs == slices and arr.shape == (3, 36) and R.same_bits(arr, R.ravel(c)[0])  # in 1-D the two layouts are one


def test_layout_2d_by_hand():
    c = dec2()  # approximation 3 x 4, levels 3 x 4 and 5 x 7: offsets (3, 4) and (6, 8), arr 11 x 15
    p = C._parse("t", c, None)
    shape, slices, regions, gaps = C._array_layout("t", p, False)
    assert shape == (2, 11, 15)
    assert slices[0] == _s(None, (0, 3), (0, 4))
    assert slices[1] == {"da": _s(None, (3, 6), (0, 4)), "ad": _s(None, (0, 3), (4, 8)), "dd": _s(None, (3, 6), (4, 8))}
    assert slices[2] == {"da": _s(None, (6, 11), (0, 7)), "ad": _s(None, (0, 5), (8, 15)), "dd": _s(None, (6, 11), (8, 15))}
    assert gaps[0] == [] and sorted(gaps[1]) == [[(0, 2), (5, 1), (8, 7)], [(0, 2), (6, 5), (7, 1)]]
    with pytest.raises(ValueError, match="padding=None asks for tight packing"):
        C._array_layout("t", p, True)
    assert R.to_array(c)[1] == slices
    lead, n, rsl, shapes = C._ravel_layout(p)
    assert (lead, n) == ((2,), 12 + 3 * 12 + 3 * 35)
    assert list(rsl[1]) == ["ad", "da", "dd"] and rsl[1] == {"ad": slice(12, 24), "da": slice(24, 36), "dd": slice(36, 48)}
    assert rsl[2] == {"ad": slice(48, 83), "da": slice(83, 118), "dd": slice(118, 153)}
    assert shapes == [(3, 4), {k: (3, 4) for k in ("ad", "da", "dd")}, {k: (5, 7) for k in ("ad", "da", "dd")}]
    assert R.ravel(c)[1:] == (rsl, shapes) and C.wavedecn_size(shapes) == R.size(shapes) == 153


def test_layout_axes_0_2_by_hand():
    r = _gen(4)
    hbw = lambda h, w: r(h, 5, w)  # [H, B, W], axes = (0, 2)
    c = (hbw(2, 3), WaveletDetailTuple2d(hbw(2, 3), hbw(2, 3), hbw(2, 3)), WaveletDetailTuple2d(hbw(4, 6), hbw(4, 6), hbw(4, 6)))
    p = C._parse("t", c, (0, 2))
    shape, slices, _, gaps = C._array_layout("t", p, True)  # tight: 2 + 2 = 4, 3 + 3 = 6
    assert p.axes == (0, 2) and shape == (8, 5, 12) and gaps == [[], []]
    assert slices[2] == {"da": _s((4, 8), None, (0, 6)), "ad": _s((0, 4), None, (6, 12)), "dd": _s((4, 8), None, (6, 12))}
    assert C._parse("t", c, (-3, -1)).axes == (0, 2)
    lead, n, rsl, shapes = C._ravel_layout(p)
    assert lead == (5,) and n == 6 * 4 + 24 * 3 and shapes[2]["dd"] == (4, 6)
    assert R.to_array(c, axes=(0, 2))[1] == slices and R.ravel(c, axes=(0, 2))[1:] == (rsl, shapes)


# ---- the reference tells layouts apart ------------------------------------------------------------------------------------------------------
def test_swapped_band_letters_fail_against_the_reference():
    c = dec2()
    right, _ = R.to_array(c, -7.5)
    flat = [c[0]] + [t for e in c[1:] for t in e]
    _, slices = R.to_array(c)
    composed = C._composed_to_array(flat, [slices[0]] + [s[k] for s in slices[1:] for k in s], right.shape, -7.5)
    assert R.same_bits(composed, right)
    wrong, _ = R.to_array(c, -7.5, swap_letters=True)  # 'da' where 'ad' belongs
    assert wrong.shape == right.shape and not R.same_bits(wrong, right)
    assert R.same_bits(wrong[:, :3, :4], right[:, :3, :4]) and R.same_bits(wrong[:, 3:6, 4:8], right[:, 3:6, 4:8])  # approximation and 'dd' agree
    assert R.same_bits(wrong[:, 3:6, :4], c[1].vertical) and R.same_bits(right[:, 3:6, :4], c[1].horizontal)


# ---- a CPU model of the kernels' box map -----------------------------------------------------------------------------------------------------
class BoxModel:
    """What a launch of kernel 59 / 60 does, box by box, on CPU tensors; counts the writers of every destination element."""

    def __init__(self, monkeypatch):
        self.launches, self.writers = [], {}
        monkeypatch.setattr(C, "_launch", self)

    def __call__(self, tag, kid, boxes, esz, padding, anchor, numel):
        assert 1 <= len(boxes) <= C.max_boxes()
        self.launches.append((tag, kid, len(boxes)))
        for b in boxes:
            ext = [d[0] for d in b.dims]
            assert len(ext) == C.BOX_DIMS and all(0 < n < 1 << 31 for n in ext) and esz == b.dst.element_size()
            dst_st = [d[1] for d in b.dims[:-1]] + [1]
            dst = b.dst.as_strided(ext, dst_st, b.dst.storage_offset() + b.dst_off)
            count = self.writers.setdefault(b.dst.untyped_storage().data_ptr(), torch.zeros(b.dst.untyped_storage().nbytes() // esz, dtype=torch.int32))
            count.as_strided(ext, dst_st, b.dst.storage_offset() + b.dst_off).add_(1)
            if b.src is None:
                assert kid == C.KID_TO_ARRAY
                dst.copy_(torch.frombuffer(bytearray(padding), dtype=b.dst.dtype)[0])
            else:
                dst.copy_(b.src.as_strided(ext, [d[2] for d in b.dims], b.src.storage_offset()))

    def written_once(self, t):
        count = self.writers[t.untyped_storage().data_ptr()]
        return bool((count.as_strided(t.shape, t.stride(), t.storage_offset()) == 1).all())


def _model_cases():
    r = _gen(9)
    cases = {
        "dec1": (dec1(), None),
        "dec1_nolead": (dec1(lead=()), None),
        "dec2": (dec2(), None),
        "dec2_lead23": (dec2(lead=(2, 3)), None),
        "dec2_f64": (dec2(dtype=torch.float64), None),
        "dec2_c128": (dec2(dtype=torch.complex128), None),
        "dec2_bf16": (dec2(dtype=torch.bfloat16), None),
        "dec2_narrow": (dec2(a=(1, 1), ext=((1, 1), (2, 1), (3, 2))), None),
        "dec3": (dec3(), None),
        "fs2_order": ((r(2, 3, 4), dict(zip(("da", "ad", "dd"), _views(r, (2,), (3, 4), 3)))), None),
        "level0": ([r(2, 5)], None),
    }
    hbw = lambda h, w: r(5, h, w).permute(1, 0, 2)  # [H, B, W] views whose batch axis is not where it lies in memory
    cases["axes02"] = ((hbw(2, 3), WaveletDetailTuple2d(hbw(2, 3), hbw(2, 3), hbw(2, 3)), WaveletDetailTuple2d(hbw(3, 5), hbw(3, 5), hbw(3, 5))), (0, 2))
    step = dec2(lead=(4,))
    cases["batch_step"] = (tuple(step[0][::2] if i == 0 else WaveletDetailTuple2d(*[t[::2] for t in e]) for i, e in enumerate(step)), None)
    haar4 = (r(2, 1, 1, 1), *[dict(zip(KEYS3, _views(r, (2,), (n, n, n), 7))) for n in (1, 2, 4, 8)])  # 29 tensors
    cases["dec3_level4"] = (haar4, None)
    return cases


@pytest.mark.parametrize("name", sorted(_model_cases()))
def test_box_model_against_the_reference(name, monkeypatch):
    coeffs, axes = _model_cases()[name]
    model = BoxModel(monkeypatch)
    p = C._parse("t", coeffs, axes)
    if p.kind == "approx":  # no box: the approximation is returned as it is
        assert p.d == 0 and not model.launches
        return
    ntens = 1 + sum(len(lv) for lv in p.levels)
    want_launches = 1 if ntens <= C.max_tensors() else 2
    # coeffs_to_array
    shape, slices, regions, gaps = C._array_layout("t", p, False)
    arr = C._to_array_launch(p, shape, regions, gaps, -7.5)
    want, wslices = R.to_array(coeffs, -7.5, axes)
    assert arr is not None and slices == wslices and R.same_bits(arr, want) and model.written_once(arr)
    assert [l[:2] for l in model.launches] == [("pack_to_array", 59)] * want_launches
    # ravel_coeffs
    model.launches.clear()
    lead, n, rsl, shapes = C._ravel_layout(p)
    flat = C._ravel_launch(p, lead, n, rsl, shapes)
    wflat, wsl, wsh = R.ravel(coeffs, axes)
    assert (rsl, shapes) == (wsl, wsh) and R.same_bits(flat, wflat) and model.written_once(flat)
    assert [l[:2] for l in model.launches] == [("pack_ravel", 59)] * want_launches
    assert R.same_bits(C._composed_ravel(C._flat(p, [list(s) for s in rsl[1:]]), p.axes), wflat)
    # the copy=True directions
    model.launches.clear()
    views = [arr[slices[0]]] + [arr[s[k]] for s in slices[1:] for k in s]
    outs = C._to_bands_launch(arr, views, [len(s) for s in slices[1:]])
    assert [l[:2] for l in model.launches] == [("pack_to_bands", 60)] * want_launches
    base = outs[0].untyped_storage().data_ptr()
    for o, v in zip(outs, views):
        assert R.same_bits(o, v) and o.is_contiguous() and model.written_once(o)
        assert o.untyped_storage().data_ptr() == base and (o.data_ptr() - base) % C.ALIGN_BYTES == 0
    rviews = [flat[..., rsl[0]].unflatten(-1, shapes[0])] + [flat[..., s[k]].unflatten(-1, sh[k]) for s, sh in zip(rsl[1:], shapes[1:]) for k in s]
    for o, v in zip(C._to_bands_launch(flat, rviews, [len(s) for s in rsl[1:]]), rviews):
        assert R.same_bits(o, v) and o.is_contiguous() and model.written_once(o)


def test_box_model_tight_and_zero_batch(monkeypatch):
    model = BoxModel(monkeypatch)
    c = dec2(a=(3, 4), ext=((3, 4), (6, 8)))
    p = C._parse("t", c, None)
    shape, slices, regions, gaps = C._array_layout("t", p, True)
    assert gaps == [[], []] and R.same_bits(C._to_array_launch(p, shape, regions, gaps, None), R.to_array(c, None)[0])
    assert model.launches == [("pack_to_array", 59, 7)]
    model.launches.clear()
    e = dec2(lead=(0,))
    p = C._parse("t", e, None)
    shape, slices, regions, gaps = C._array_layout("t", p, False)
    assert C._to_array_launch(p, shape, regions, gaps, 1.0).shape == (0, 11, 15) and model.launches == []
    lead, n, rsl, shapes = C._ravel_layout(p)
    assert C._ravel_launch(p, lead, n, rsl, shapes).shape == R.ravel(e)[0].shape == (0, 153) and model.launches == []
    assert C._composed_ravel(C._flat(p, [list(s) for s in rsl[1:]]), p.axes).shape == (0, 153)


def test_boxes_merge_and_refuse():
    assert C._merge([(2, 60, 200), (3, 20, 40), (4, 5, 11), (5, 1, 1)]) == [[2, 60, 200], [3, 20, 40], [4, 5, 11], [5, 1, 1]]
    assert C._merge([(2, 60, 200), (3, 20, 40), (4, 5, 10), (5, 1, 1)]) == [[1, 0, 0], [2, 60, 200], [12, 5, 10], [5, 1, 1]]
    assert C._merge([(2, 60, 60), (3, 20, 20), (4, 5, 5), (5, 1, 1)]) == [[1, 0, 0]] * 3 + [[120, 1, 1]]  # dense on both sides: one row
    assert C._merge([(2, 60, None), (3, 20, None), (4, 5, None), (2, 1, None)])[-2:] == [[24, 5, None], [2, 1, None]]  # a fill box
    assert C._merge([(3, 7, 1), (1, 1, 9)])[-2:] == [[3, 7, 1], [1, 1, 1]]  # a band one column wide: rows of one element
    assert C._merge([(2, 960, 7), (3, 320, 5), (4, 80, 3), (5, 16, 2), (6, 1, 1)]) is None  # five extents: composed


# ---- the copy=False views --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,make", [("wavedec", dec1), ("wavedec2", dec2), ("wavedecn", dec3)])
def test_views_alias_round_trip_and_carry_gradients(fmt, make):
    c = make()
    arr, slices = R.to_array(c, -7.5)
    back = ptwt_amd.array_to_coeffs(arr, slices, fmt)
    assert R.same_container(back, c) and type(back) is type(c)
    again, _ = R.to_array(back, -7.5)
    assert R.same_bits(again, arr)
    leaves = [back[0]] + [t for lv in R.levels(back)[1] for t in lv.values()]
    lo, hi = arr.data_ptr(), arr.data_ptr() + arr.numel() * arr.element_size()
    assert all(lo <= t.data_ptr() < hi and t.untyped_storage().data_ptr() == arr.untyped_storage().data_ptr() for t in leaves)
    flat, rsl, shapes = R.ravel(c)
    rback = ptwt_amd.unravel_coeffs(flat, rsl, shapes, fmt)
    assert R.same_bits(R.ravel(rback)[0], flat) and rback[1 if fmt != "wavedec" else 0] is not None
    want = R.unravel(flat, rsl, shapes)
    for a, b in [(rback[0], want[0])] + [(lv[k], w[k]) for lv, w in zip(R.levels(rback)[1], want[1:]) for k in w]:
        assert R.same_bits(a, b) and a.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
    x = arr.clone().requires_grad_(True)
    out = ptwt_amd.array_to_coeffs(x, slices, fmt)
    w = torch.arange(1.0, 1.0 + leaves[-1].numel()).reshape(leaves[-1].shape)
    last = list(R.levels(out)[1][-1].values())[-1]
    (g,) = torch.autograd.grad((last * w).sum() + 2 * out[0].sum(), x)
    want = torch.zeros_like(arr)
    want[list(slices[-1].values())[-1]] = w
    want[slices[0]] = 2
    assert torch.equal(g, want)


def test_formats_and_the_approximation_alone():
    a = torch.arange(6.0).reshape(2, 3)
    for fmt, kind in (("wavedec", list), ("wavedec2", tuple), ("wavedecn", tuple)):
        out = ptwt_amd.array_to_coeffs(a, [(slice(None), slice(None))], fmt)
        assert type(out) is kind and len(out) == 1 and out[0] is a
        out = ptwt_amd.unravel_coeffs(a, [slice(None)], [(2, 3)], fmt, copy=True)  # nothing to copy: no device needed
        assert type(out) is kind and out[0] is a
    arr, slices = ptwt_amd.coeffs_to_array([a])
    assert arr is a and slices == [(slice(None), slice(None))]
    flat, rsl, shapes = ptwt_amd.ravel_coeffs((a,))
    assert flat is a and rsl == [slice(None)] and shapes == [(2, 3)] and ptwt_amd.wavedecn_size(shapes) == 6
    arr, slices = R.to_array(dec2())
    with pytest.raises(ValueError, match="'wavedec' is a 1-D container, the slices describe a 2-D one"):
        ptwt_amd.array_to_coeffs(arr, slices, "wavedec")
    arr1, slices1 = R.to_array(dec1())
    with pytest.raises(ValueError, match="'wavedec2' is a 2-D container, the slices describe a 1-D one"):
        ptwt_amd.array_to_coeffs(arr1, slices1, "wavedec2")
    with pytest.raises(ValueError, match="'wavedec2' is a 2-D container, the slices describe a 3-D one"):
        ptwt_amd.unravel_coeffs(*R.ravel(dec3()), "wavedec2")
    with pytest.raises(ValueError, match="output_format is one of"):
        ptwt_amd.array_to_coeffs(arr, slices, "wavedec3")
    assert isinstance(ptwt_amd.array_to_coeffs(arr, slices, "wavedecn")[1], dict)
    assert list(ptwt_amd.array_to_coeffs(arr, slices)[1]) == ["da", "ad", "dd"]  # the key order of the slices


# ---- errors, before any device is needed ---------------------------------------------------------------------------------------------------
def test_argument_errors():
    for call in (ptwt_amd.coeffs_to_array, ptwt_amd.ravel_coeffs):
        c = list(dec2())
        with pytest.raises(ValueError, match="entry 1 of the container is None"):
            call([c[0], None, c[2]])
        with pytest.raises(ValueError, match="band 'ad' of entry 2 is None"):
            call([c[0], c[1], WaveletDetailTuple2d(c[2][0], None, c[2][2])])
        with pytest.raises(ValueError, match="approximation tensor, got None"):
            call([None, c[1]])
        d3 = list(dec3())
        with pytest.raises(ValueError, match=r"needs the 7 bands .* missing \['dad'\]"):
            call([d3[0], {k: v for k, v in d3[1].items() if k != "dad"}])
        with pytest.raises(ValueError, match="band 'ddd' of entry 1 is None"):
            call([d3[0], {**d3[1], "ddd": None}])
        with pytest.raises(ValueError, match="the bands of one level share their shape"):
            call([c[0], WaveletDetailTuple2d(c[1][0], c[1][1][:, :2], c[1][2])])
        with pytest.raises(ValueError, match="share dtype and device"):
            call([c[0], WaveletDetailTuple2d(c[1][0], c[1][1].double(), c[1][2])])
        with pytest.raises(ValueError, match="share dtype and device"):
            call([c[0], WaveletDetailTuple2d(c[1][0], c[1][1].to("meta"), c[1][2])])
        with pytest.raises(ValueError, match=r"share their leading shape \(2,\)"):
            call([c[0], WaveletDetailTuple2d(*[t[:1] for t in c[1]])])
        with pytest.raises(ValueError, match="dtype torch.int32 not supported"):
            call([torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, 4, dtype=torch.int32)])
        with pytest.raises(ValueError, match="axes must be distinct"):
            call(c, axes=(1, -2))
        with pytest.raises(ValueError, match="one entry per transformed axis"):
            call(c, axes=(1,))
        with pytest.raises(ValueError, match="expected a coefficient container"):
            call(c[0])
        with pytest.raises(RuntimeError, match="ROCm device"):  # valid arguments: only the device is missing
            call(c)
    with pytest.raises(ValueError, match="padding=None asks for tight packing"):
        ptwt_amd.coeffs_to_array(dec2(), None)
    over = dec2(a=(3, 4), ext=((3, 4), (7, 8)))  # 7 rows of 'ad' next to 6 rows before it
    with pytest.raises(ValueError, match="would overlap along transformed axis 0"):
        ptwt_amd.coeffs_to_array(over)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.ravel_coeffs(over)  # the flat layout has no blocks to overlap
    arr, slices = R.to_array(dec2())
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.array_to_coeffs(arr, slices, "wavedec2", copy=True)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ptwt_amd.unravel_coeffs(*R.ravel(dec2()), "wavedec2", copy=True)
    with pytest.raises(ValueError, match="shapes has the nesting and the keys of slices"):
        ptwt_amd.unravel_coeffs(R.ravel(dec2())[0], R.ravel(dec2())[1], [(3, 4)])
    with pytest.raises(ValueError, match="slice of step 1 on the last axis with the elements of its shape"):
        flat, rsl, shapes = R.ravel(dec1())
        ptwt_amd.unravel_coeffs(flat, rsl, [(9,)] + shapes[1:], "wavedec")


# ---- wavedecn_shapes against the committed goldens ---------------------------------------------------------------------------------------------
def _shapes_of(flat_named, d):
    """[shape, {key: shape}, ...] of goldens named as tests/_golden.flatten_coeffs names them."""
    names = {1: {"": "d"}, 2: {"h": "da", "v": "ad", "d": "dd"}}.get(d)
    out = [None]
    for name, shape in flat_named:
        if name == "a":
            out[0] = tuple(shape)
            continue
        lvl, _, band = name.partition("_")
        while len(out) < int(lvl) + 2:
            out.append({})
        out[int(lvl) + 1][names[band] if names else band] = tuple(shape)
    return out


def _same_shapes(got, want):
    return got[0] == want[0] and len(got) == len(want) and all(dict(g) == dict(w) for g, w in zip(got[1:], want[1:]))


def test_wavedecn_shapes_equal_the_goldens():
    checked = 0
    z, idx = G.load("pywt_wavedec1d.npz")
    for case in idx:
        want = _shapes_of([("a" if i == 0 else str(i - 1), z[f"{case['key']}_{i}"].shape) for i in range(case["ncoef"])], 1)
        x_shape = z[f"{case['key']}_x"].shape
        assert x_shape[-1] == case["n"]
        got = ptwt_amd.wavedecn_shapes(x_shape, case["wavelet"], case["mode"], case["level"], axes=-1)
        assert _same_shapes(got, want), case
        assert ptwt_amd.wavedecn_size(got) == sum(z[f"{case['key']}_{i}"].size for i in range(case["ncoef"]))
        checked += 1
    for fname, d in (("pywt_wavedec2d.npz", 2), ("pywt_wavedec3d.npz", 3)):
        z, idx = G.load(fname)
        for case in idx:
            pre = case["key"] + "_"
            named = [(k[len(pre):], z[k].shape) for k in z.files if k.startswith(pre) and k != pre + "x"]
            want = _shapes_of(named, d)
            x_shape = tuple(z[pre + "x"].shape)
            assert x_shape[-d:] == tuple(case["shape"])
            got = ptwt_amd.wavedecn_shapes(x_shape, case["wavelet"], case["mode"], case["level"], axes=tuple(range(-d, 0)))
            assert _same_shapes(got, want), case
            if len(x_shape) == d + 1 and x_shape[0] == 1:  # all axes of the plain shape: the same extents
                plain = ptwt_amd.wavedecn_shapes(x_shape[1:], case["wavelet"], case["mode"], case["level"])
                assert plain[0] == want[0][1:] and all(v == want[i][k][1:] for i in range(1, len(want)) for k, v in plain[i].items())
            checked += 1
    for case in _per_ref.goldens():
        d = case["ndim"]
        want = _shapes_of([(name, arr.shape) for name, arr in case["coeffs"].items()], d)
        got = ptwt_amd.wavedecn_shapes(tuple(case["shape"]), case["wavelet"], "periodization", case["level"])
        assert _same_shapes(got, want), (case["wavelet"], case["shape"], case["level"])
        checked += 1
    assert checked == 445 + 140 + 60 + 324


def test_wavedecn_shapes_level_default_and_errors():
    S = ptwt_amd.wavedecn_shapes
    assert len(S((64,), "db4")) == 1 + 3 and len(S((8, 64, 64), "db2", "zero", axes=(1, 2))) == 1 + 4  # dwtn_max_level
    assert S((5,), "db4", "symmetric") == [(5,)] and S((16,), "db4", "symmetric", 3) == [(8,), {"d": (8,)}, {"d": (9,)}, {"d": (11,)}]
    assert S((16,), "db4", "periodization", 3) == [(2,), {"d": (2,)}, {"d": (4,)}, {"d": (8,)}]
    assert S((7, 9), "haar", "smooth", 1) == [(4, 5), {"ad": (4, 5), "da": (4, 5), "dd": (4, 5)}]
    assert S((3, 16), "db4", "zero", 1, axes=-1) == [(3, 11), {"d": (3, 11)}]
    assert S((16,), "db4", "zero", -1) == [(16,)]  # the padded drivers' level loop takes no trip
    for mode in ("periodization", "smooth"):
        with pytest.raises(ValueError, match="Level value of -1 is too low"):
            S((16,), "db4", mode, -1)
    with pytest.raises(ValueError, match="Padding mode not supported"):
        S((16,), "db4", "mirror")
    with pytest.raises(RuntimeError, match="Padding size should be less"):
        S((16, 6), "db4", "reflect", 1)  # 6 samples reflected by 6
    with pytest.raises(ValueError, match="same axis twice"):
        S((16, 16), "db4", "zero", 1, axes=(0, -2))
    with pytest.raises(ValueError, match="out of range"):
        S((16, 16), "db4", "zero", 1, axes=(2,))


# ---- the surface -------------------------------------------------------------------------------------------------------------------------
def test_api_surface():
    names = ["coeffs_to_array", "array_to_coeffs", "ravel_coeffs", "unravel_coeffs", "wavedecn_shapes", "wavedecn_size"]
    assert C.__all__ == names
    for name in names:
        assert name in ptwt_amd.__all__ and getattr(ptwt_amd, name) is getattr(C, name)
    assert isinstance(C.COMPOSED_CELLS, set) and all(cell[0] in names[:4] for cell in C.COMPOSED_CELLS)
    assert (C.KID_TO_ARRAY, C.KID_TO_BANDS) == (59, 60)
    with open(os.path.join(ROOT, "include", "mifwt.h")) as f:
        header = f.read()
    for name, kid in (("MIFWT_KID_PACK_TO_ARRAY", 59), ("MIFWT_KID_PACK_TO_BANDS", 60)):
        assert re.search(rf"#define {name} {kid}\b", header), name
    assert re.search(r"\*\s+59 / 60\s", header)  # the id table
    lib = _engine.load_library()
    assert sorted(_engine.PACK_ENTRIES) == ["mifwt_pack_max_boxes", "mifwt_pack_max_tensors", "mifwt_pack_plan", "mifwt_pack_to_array",
                                            "mifwt_pack_to_bands"]
    for sym in _engine.PACK_ENTRIES:
        assert getattr(lib, sym) is not None and sym not in _engine._ENTRIES
        assert re.search(rf"\b{sym}\(", header), sym
    assert lib.mifwt_abi_version() == _engine.ABI_VERSION == 3
    assert "sparse_encode" in C.ravel_coeffs.__doc__ and "overwrites" in C.coeffs_to_array.__doc__


def _box(ext, src=1, dst=1):
    b = _engine.PackBox()
    b.extent[:] = ext
    b.src, b.dst = src, dst
    return b


def test_cabi_answers_without_a_device():
    lib = C._lib()
    assert C.max_tensors() == 24 and C.max_boxes() == 40
    assert C.max_boxes() >= 1 + 7 + 2 * 16  # a level-3 3-D container with gaps at two levels: 22 tensors and 18 fills
    arr = lambda *boxes: ((_engine.PackBox * len(boxes))(*boxes), len(boxes))
    plan = lambda esz, *boxes: lib.mifwt_pack_plan(esz, *arr(*boxes))
    # rows of fewer than 1024 slots share a unit; slots = (n + 2 vec - 2) / vec whatever the alignment
    assert plan(4, _box([1, 1, 10, 33])) == 1 and plan(4, _box([1, 2, 200, 33])) == -(-400 // (1024 // 9))
    assert plan(4, _box([1, 1, 3, 4 * 1023 - 5])) == 3 and plan(4, _box([1, 1, 3, 4 * 1023 - 2])) == 3  # 1023 and 1024 slots: a row a unit
    assert plan(2, _box([1, 1, 3, 1 << 20])) == 3 * 129 and plan(16, _box([1, 1, 1, 5000])) == 5 and plan(8, _box([2, 0, 3, 5])) == 0
    assert plan(4, _box([1, 1, 1, 5]), _box([1, 1, 0, 5]), _box([1, 1, 2000, 1])) == 1 + 0 + 2
    assert plan(3, _box([1, 1, 1, 5])) == -1 and plan(4, _box([1, 1, -1, 5])) == -1
    assert lib.mifwt_pack_plan(4, None, 1) == -1 and lib.mifwt_pack_plan(4, *arr(*[_box([1, 1, 1, 1])] * 41)) == -1
    assert plan(4, _box([1, 1, 1, 1 << 31])) == -2 and plan(4, _box([1 << 11, 1 << 10, 1 << 10, 1])) == -2
    # nothing is launched for a refused call
    pad = (_engine.ctypes.c_char * 16)()
    to_array = lambda esz, padding, *boxes: lib.mifwt_pack_to_array(esz, *arr(*boxes), padding, None)
    to_bands = lambda esz, *boxes: lib.mifwt_pack_to_bands(esz, *arr(*boxes), None)
    assert to_array(4, None, _box([1, 1, 1, 5])) == -1  # no padding element
    assert to_array(4, pad, _box([1, 1, 1, 5], dst=None)) == -1 and to_bands(4, _box([1, 1, 1, 5], src=None)) == -1  # kernel 60 fills nothing
    assert to_array(4, pad, _box([1, 1, 1, 5], src=2, dst=4)) == -1 and to_bands(8, _box([1, 1, 1, 5], src=8, dst=4)) == -1  # misaligned
    assert to_array(4, pad, _box([1, 0, 1, 5], src=None, dst=None)) == 0 and to_bands(2, _box([0, 1, 1, 5])) == 0  # nothing to write
    assert to_array(5, pad, _box([1, 1, 1, 5])) == -1 and to_bands(4, _box([1, 1, 1, 1 << 31])) == -2


#: the guards of ``box_units`` / ``build_args`` (csrc/mifwt_pack.hip) as ``mifwt_pack_plan`` answers them: (what, element size, boxes,
#: the answer: units, or -2 = MIFWT_ERR_UNSUPPORTED) — the last accepted value and the first refused one
PACK_GUARDS = [
    ("row of 2^31 - 1", 2, [[1, 1, 1, (1 << 31) - 1]], None), ("row of 2^31", 2, [[1, 1, 1, 1 << 31]], -2),
    ("2^31 - 1 rows of 2", 2, [[1, 1, (1 << 31) - 1, 2]], -(-((1 << 31) - 1) // 512)), ("2^31 rows of 2", 2, [[2, 1, 1 << 30, 2]], -2),
    ("2^31 rows on one axis", 2, [[1, 1, 1 << 31, 2]], -2), ("2^31 + 8 rows of 2", 2, [[(1 << 31) + 8, 1, 1, 2]], -2),
    ("2^31 - 2 units", 4, [[1, 1, 715827882, 8192]], (1 << 31) - 2), ("2^31 + 1 units", 4, [[1, 1, 715827883, 8192]], -2),
    ("2^31 - 2 units in two boxes", 4, [[1, 1, 715827881, 8192], [1, 1, 1, 8192]], (1 << 31) - 2),
    ("2^31 units in two boxes", 4, [[1, 1, 715827882, 8192], [1, 1, 2000, 1]], -2),
]


@pytest.mark.parametrize("what,esz,boxes,want", PACK_GUARDS, ids=[g[0] for g in PACK_GUARDS])
def test_guards_of_the_pack_plan(what, esz, boxes, want):
    lib = C._lib()
    arr = (_engine.PackBox * len(boxes))(*[_box(ext) for ext in boxes])
    got = lib.mifwt_pack_plan(esz, arr, len(boxes))
    if want is None:  # one row of 2^31 - 1 float16: slots = (n + 14) / 8, units of about 1024 slots with none empty
        vpr = ((1 << 31) - 1 + 14) // 8
        upr = -(-vpr // 1024)
        want = -(-vpr // -(-vpr // upr))
    assert got == want, (what, got)
