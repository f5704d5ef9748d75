"""A coefficient container as ONE tensor and back — PyWavelets' ``coeffs_to_array`` / ``array_to_coeffs``, ``ravel_coeffs`` /
``unravel_coeffs``, ``wavedecn_shapes`` and ``wavedecn_size`` (C ABI ``mifwt_pack_*``, include/mifwt.h; kernel csrc/mifwt_pack.hip, ids
59 / 60).

    coeffs = ptwt_amd.wavedec2(x, "db4", level=3)
    arr, slices = ptwt_amd.coeffs_to_array(coeffs, padding=0.0)      # the "wavelet image" of the batch: one launch, padding included
    back = ptwt_amd.array_to_coeffs(arr, slices, "wavedec2")         # views of arr; copy=True: fresh dense tensors, one launch
    y = ptwt_amd.waverec2(back, "db4")

CONTAINERS AND AXES.  The number of transformed axes ``d`` is read off the container: a list or tuple of tensors gives ``d = 1`` (band
key ``"d"``), ``WaveletDetailTuple2d`` entries give ``d = 2`` (``horizontal = "da"``, ``vertical = "ad"``, ``diagonal = "dd"``), dict
entries give ``d = len(key)`` with their own keys.  Letter ``i`` of a key belongs to transformed axis ``i``.  ``axes=None`` means the last
``d`` axes, otherwise ``axes`` is ``d`` distinct axes as given to the transform; all other axes are LEADING axes and are carried through.

THE ARRAY LAYOUT is PyWavelets'.  Per transformed axis ``i``, with ``a_i`` the approximation's extent and ``D_l,i`` the extent of the
bands of level ``l`` (coarsest first): ``o_1,i = a_i``, ``o_{l+1},i = o_l,i + D_l,i``; ``arr`` has extent ``a_i + sum_l D_l,i``.  The
approximation occupies ``[0, a_i)``; the band with key ``k`` of level ``l`` occupies ``[0, D_l,i)`` along an axis whose letter is ``a``
and ``[o_l,i, o_l,i + D_l,i)`` along an axis whose letter is ``d``; everything else holds ``padding``.  DEVIATION from PyWavelets: where
blocks would overlap (``D_l,i > o_l,i`` on an ``a`` axis; impossible for a container a transform of this library produced, since
``o_{l+1} >= 2 D_{l+1} >= D_l``) PyWavelets silently overwrites, this module raises ``ValueError``.

THE FLAT LAYOUT (``ravel_coeffs``): ``[*lead, n]`` — the approximation, then level by level, coarsest first, within a level the bands in
SORTED key order (``ad, da, dd``), each band row-major over its transformed axes in axis order.  For 2-D containers this order differs
from the flat index of ``sparse_encode``, which follows container order (``da, ad, dd``).

LAUNCHES.  The host cuts the destination into boxes — the approximation, every band, and the gaps between them — that tile it, and one
launch (id 59) copies the bands through their own strides and fills the gaps: every element of ``arr`` is written once, every band
element read once, no fill pass, no ``.contiguous()``.  ``copy=True`` of the two inverse calls carves fresh dense tensors out of ONE
backing allocation (every start rounded up to 256 bytes) and writes them with one launch of the same table run the other way (id 60).
One launch takes :func:`max_tensors` tensors (24) of whole levels; a larger container (a level-4 3-D container has 29) takes one launch
per range of levels, each owning the nested region ``[0, o + D)`` minus ``[0, o)`` of its levels.  The copy is templated on the element
size: float32, float64, complex64, complex128 and (always, not only inside ``half_storage()``) float16 and bfloat16.  Nothing is read
back and nothing synchronises: the calls can be captured (``ptwt_amd.capture``).  A box of more than four extents after merging, an
extent beyond the kernels' index range (2^31 elements per row, 2^31 rows per box) and the cells of ``COMPOSED_CELLS`` (by call, dtype, ``d`` and short rows) are composed from
torch operations (:func:`_composed_to_array`, :func:`_composed_to_bands`), which are also the emulation tools/pack_bench.py compares
the kernels with.

GRADIENTS need no kernel: the two directions are each other's adjoint.  ``coeffs_to_array`` / ``ravel_coeffs`` hand every tensor the
view ``g[slices]`` (reshaped), the ``copy=True`` calls scatter the incoming gradients into zeros by slice assignment, ``copy=False`` is
differentiable by construction.  The backwards are differentiable torch operations, so gradients of any order exist, for complex and
16-bit data alike.
"""
from __future__ import annotations

import ctypes
import itertools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _engine
from . import _fwt
from . import _wavelets
from .constants import WaveletDetailTuple2d

__all__ = ["coeffs_to_array", "array_to_coeffs", "ravel_coeffs", "unravel_coeffs", "wavedecn_shapes", "wavedecn_size"]

KID_TO_ARRAY, KID_TO_BANDS = 59, 60
DTYPES = (torch.float32, torch.float64, torch.complex64, torch.complex128, torch.float16, torch.bfloat16)
FORMATS = ("wavedec", "wavedec2", "wavedecn")
ALIGN_BYTES = 256  # start of every tensor in the backing allocation of a copy=True call
BOX_DIMS = 4       # extents of a box of the kernels (three outer ones and the row)
#: rows of fewer elements than this are SHORT: the last term of a cell
SHORT_ROW = 64
#: (call, dtype, d, short) cells that are composed from torch operations instead of the kernels; ``short`` says whether the innermost
#: extent of the finest level's bands (the longest rows a launch copies) is below SHORT_ROW.  A cell belongs there only where tools/pack_bench.py (which measures with
#: this set emptied) has shown the fused median behind the composed one by more than the spread of its windows, at every size and
#: packing measured for the cell (README, EXPERIMENTS part M).  Measured behind: all four calls on the 1-D float32 container (ten long
#: dense rows: torch's own copies lead by 20 - 45 %), three of the four on the 2-D float64 container (1 - 12 %), array_to_coeffs on the
#: 3-D float32 container (6 %), and all four on 4096 images of 33 x 33 float32 (rows of 5 - 20 elements: 1.6 - 5 x).  SHORT_ROW lies
#: between the rows measured behind (20) and ahead (129 and up); the line itself was not measured.  One mixed cell stays with the
#: kernels: coeffs_to_array on 2-D float64 leads with gaps (1.32 x) and trails when tight (1 %).
COMPOSED_CELLS: set = {
    ("coeffs_to_array", torch.float32, 1, False), ("ravel_coeffs", torch.float32, 1, False), ("array_to_coeffs", torch.float32, 1, False),
    ("unravel_coeffs", torch.float32, 1, False),
    ("ravel_coeffs", torch.float64, 2, False), ("array_to_coeffs", torch.float64, 2, False), ("unravel_coeffs", torch.float64, 2, False),
    ("array_to_coeffs", torch.float32, 3, False),
    ("coeffs_to_array", torch.float32, 2, True), ("ravel_coeffs", torch.float32, 2, True), ("array_to_coeffs", torch.float32, 2, True),
    ("unravel_coeffs", torch.float32, 2, True),
}
_KEYS_2D = ("da", "ad", "dd")  # WaveletDetailTuple2d(horizontal, vertical, diagonal)

_entries = None


def _lib():
    global _entries
    if _entries is None:
        _entries = _engine.private_entries(_engine.PACK_ENTRIES)
    return _entries


def max_tensors() -> int:
    """Tensors of a container one launch takes (``mifwt_pack_max_tensors``)."""
    return int(_lib().mifwt_pack_max_tensors())


def max_boxes() -> int:
    """Boxes — tensors and the gaps between them — one launch takes (``mifwt_pack_max_boxes``)."""
    return int(_lib().mifwt_pack_max_boxes())


# ---- containers --------------------------------------------------------------------------------------------------------------------
class _Parsed:
    """A container read once: ``d``, the approximation, per level a dict key -> tensor in container order, the container's kind, the
    transformed axes (non-negative), the rank."""

    __slots__ = ("d", "approx", "levels", "kind", "axes", "rank")


def _entry_bands(who: str, e, pos: int) -> Tuple[str, Dict[str, torch.Tensor]]:
    if e is None:
        raise ValueError(f"{who}: entry {pos} of the container is None: every band is needed")
    if isinstance(e, torch.Tensor):
        return "wavedec", {"d": e}
    if isinstance(e, dict):
        if not e or not all(isinstance(k, str) and k and set(k) <= {"a", "d"} for k in e):
            raise ValueError(f"{who}: the keys of a detail dict are strings of 'a' and 'd', got {list(e)}")
        d = len(next(iter(e)))
        want = ["".join(p) for p in itertools.product("ad", repeat=d)][1:]
        missing = [k for k in want if k not in e]
        if missing or len(e) != len(want):
            raise ValueError(f"{who}: entry {pos} needs the {len(want)} bands {want}, missing {missing}, got {list(e)}")
        bands = dict(e)
        kind = "wavedecn"
    elif isinstance(e, tuple) and len(e) == 3:
        bands = dict(zip(_KEYS_2D, e))
        kind = "wavedec2"
    else:
        raise ValueError(f"{who}: entry {pos} is a tensor, a WaveletDetailTuple2d or a dict of tensors, not {type(e).__name__}")
    for k, t in bands.items():
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who}: band {k!r} of entry {pos} is {'None' if t is None else type(t).__name__}: every band is needed")
    return kind, bands


def _parse(who: str, coeffs, axes) -> _Parsed:
    if not isinstance(coeffs, (list, tuple)) or len(coeffs) == 0:
        raise ValueError(f"{who}: expected a coefficient container (a non-empty list or tuple), got {type(coeffs).__name__}")
    if not isinstance(coeffs[0], torch.Tensor):
        raise ValueError(f"{who}: the first entry of a container is the approximation tensor, got "
                         f"{'None' if coeffs[0] is None else type(coeffs[0]).__name__}")
    p = _Parsed()
    p.approx = coeffs[0]
    p.levels = []
    p.kind = None
    for pos, e in enumerate(coeffs[1:], 1):
        kind, bands = _entry_bands(who, e, pos)
        if p.kind is not None and (kind != p.kind or len(next(iter(bands))) != p.d):
            raise ValueError(f"{who}: the entries of a container are of one kind")
        p.kind, p.d = kind, len(next(iter(bands)))
        p.levels.append(bands)
    a = p.approx
    p.rank = a.dim()
    if a.dtype not in DTYPES:
        raise ValueError(f"{who}: dtype {a.dtype} not supported (float32, float64, complex64, complex128, float16, bfloat16)")
    if p.kind is None:  # the approximation alone
        p.d, p.kind, p.axes = 0, "approx", ()
        return p
    if p.rank < p.d:
        raise ValueError(f"{who}: a {p.d}-D container needs tensors of at least {p.d} axes, got {p.rank}")
    if axes is None:
        p.axes = tuple(range(p.rank - p.d, p.rank))
    else:
        axes = (axes,) if isinstance(axes, int) else tuple(axes)
        if len(axes) != p.d:
            raise ValueError(f"{who}: axes has one entry per transformed axis: {len(axes)} for a {p.d}-D container")
        if any(not -p.rank <= ax < p.rank for ax in axes):
            raise ValueError(f"{who}: axes {axes} out of range for tensors of {p.rank} axes")
        p.axes = tuple(ax % p.rank for ax in axes)
        if len(set(p.axes)) != p.d:
            raise ValueError(f"{who}: axes must be distinct, got {axes}")
    lead = [s for ax, s in enumerate(a.shape) if ax not in p.axes]
    for pos, bands in enumerate(p.levels, 1):
        first = next(iter(bands.values()))
        for k, t in bands.items():
            if t.dtype != a.dtype or t.device != a.device:
                raise ValueError(f"{who}: the tensors of a container share dtype and device: band {k!r} of entry {pos} is {t.dtype} on "
                                 f"{t.device}, the approximation {a.dtype} on {a.device}")
            if t.dim() != p.rank or [s for ax, s in enumerate(t.shape) if ax not in p.axes] != lead:
                raise ValueError(f"{who}: the tensors of a container share their leading shape {tuple(lead)}: band {k!r} of entry {pos} "
                                 f"has shape {tuple(t.shape)}")
            if t.shape != first.shape:
                raise ValueError(f"{who}: the bands of one level share their shape: entry {pos} holds {tuple(first.shape)} and "
                                 f"{tuple(t.shape)}")
    return p


def _container(fmt: str, approx: torch.Tensor, levels: Sequence[Dict[str, torch.Tensor]]):
    """The container of ``fmt`` over the approximation and per-level dicts: the types the transforms return."""
    if fmt == "wavedec":
        return [approx] + [lv["d"] for lv in levels]
    if fmt == "wavedec2":
        return (approx, *[WaveletDetailTuple2d(lv["da"], lv["ad"], lv["dd"]) for lv in levels])
    return (approx, *[dict(lv) for lv in levels])


def _check_format(who: str, fmt: str, d: int, keys: Sequence[Sequence[str]]) -> None:
    if fmt not in FORMATS:
        raise ValueError(f"{who}: output_format is one of {FORMATS}, got {fmt!r}")
    want = {"wavedec": 1, "wavedec2": 2}.get(fmt)
    if want is not None and keys and (d != want or any(sorted(k) != sorted(_KEYS_2D if want == 2 else ("d",)) for k in keys)):
        raise ValueError(f"{who}: output_format {fmt!r} is a {want}-D container, the slices describe a {d}-D one with the keys "
                         f"{[list(k) for k in keys]}")


# ---- the two layouts (host only) ---------------------------------------------------------------------------------------------------
def _array_layout(who: str, p: _Parsed, tight: bool):
    """(shape of ``arr``, slices, regions, gaps): a region is, per axis of ``arr``, ``(start, extent)``; ``regions`` has the
    approximation's first, then per level a dict; ``gaps`` per level the boxes of padding of its shell.  Raises for overlapping blocks
    and, with ``tight``, for any gap."""
    a = p.approx
    d, axes = p.d, p.axes
    ext = [[a.shape[ax] for ax in axes]] + [[next(iter(lv.values())).shape[ax] for ax in axes] for lv in p.levels]
    o = [list(ext[0])]
    for lvl in ext[1:]:
        o.append([o[-1][i] + lvl[i] for i in range(d)])
    # o[l - 1][i] = o_l,i for l >= 1; o[-1] is the extent of arr
    shape = list(a.shape)
    for i, ax in enumerate(axes):
        shape[ax] = o[-1][i]
    full = [(0, s) for s in shape]

    def region(spans):
        r = list(full)
        for i, ax in enumerate(axes):
            r[ax] = spans[i]
        return r

    regions: list = [region([(0, n) for n in ext[0]])]
    gaps: list = []
    for l, lv in enumerate(p.levels, 1):
        D, ol = ext[l], o[l - 1]
        if d >= 2:
            for i in range(d):
                if D[i] > ol[i]:
                    raise ValueError(f"{who}: the blocks of level entry {l} would overlap along transformed axis {i}: its bands have extent "
                                     f"{D[i]}, the blocks before them end at {ol[i]} (PyWavelets overwrites here; no transform of this "
                                     "library produces such a container)")
                if tight and D[i] != ol[i]:
                    raise ValueError(f"{who}: padding=None asks for tight packing, but level entry {l} leaves a gap along transformed "
                                     f"axis {i}: extent {D[i]} against {ol[i]} before it")
        regs, gap = {}, []
        for k in lv:
            regs[k] = region([(ol[i], D[i]) if k[i] == "d" else (0, D[i]) for i in range(d)])
            # the cell of the key minus its band, cut along its 'a' axes in order: before j inside the band, j in the gap, after j whole
            a_axes = [i for i in range(d) if k[i] == "a"]
            for n, j in enumerate(a_axes):
                if ol[j] == D[j]:
                    continue
                spans = [(ol[i], D[i]) if k[i] == "d" else None for i in range(d)]
                for m, i in enumerate(a_axes):
                    spans[i] = (0, D[i]) if m < n else (D[i], ol[i] - D[i]) if m == n else (0, ol[i])
                gap.append(region(spans))
        regions.append(regs)
        gaps.append(gap)
    as_slices = lambda r: tuple(slice(None) if ax not in axes else slice(s, s + n) for ax, (s, n) in enumerate(r))
    slices: list = [as_slices(regions[0])] + [{k: as_slices(r) for k, r in regs.items()} for regs in regions[1:]]
    return tuple(shape), slices, regions, gaps


def _ravel_layout(p: _Parsed):
    """(lead shape, n, slices, shapes, per level the sorted keys)."""
    lead = tuple(s for ax, s in enumerate(p.approx.shape) if ax not in p.axes)
    tshape = lambda t: tuple(t.shape[ax] for ax in p.axes)
    shapes: list = [tshape(p.approx)]
    n = math.prod(shapes[0])
    slices: list = [slice(0, n)]
    for lv in p.levels:
        sl, sh = {}, {}
        for k in sorted(lv):
            sh[k] = tshape(lv[k])
            m = math.prod(sh[k])
            sl[k] = slice(n, n + m)
            n += m
        slices.append(sl)
        shapes.append(sh)
    return lead, n, slices, shapes


def _last(t: torch.Tensor, axes: Sequence[int]) -> torch.Tensor:
    """``t`` with the transformed axes moved to the end, in order (a view)."""
    if tuple(axes) == tuple(range(t.dim() - len(axes), t.dim())):
        return t
    return t.permute([ax for ax in range(t.dim()) if ax not in axes] + list(axes))


def _unlast(t: torch.Tensor, axes: Sequence[int]) -> torch.Tensor:
    """The inverse of :func:`_last`."""
    if tuple(axes) == tuple(range(t.dim() - len(axes), t.dim())):
        return t
    perm = [ax for ax in range(t.dim()) if ax not in axes] + list(axes)
    inv = [0] * len(perm)
    for i, q in enumerate(perm):
        inv[q] = i
    return t.permute(inv)


# ---- composed from torch operations -------------------------------------------------------------------------------------------------
def _composed_to_array(tensors: Sequence[torch.Tensor], slices: Sequence, shape, padding) -> torch.Tensor:
    """``arr`` from ``torch.full`` (``padding=None``, blocks that tile the array: ``torch.empty``) and one slice assignment per tensor
    (``slices`` flat, one index per tensor): the route beyond the kernel's envelope and the emulation the benchmark compares it with."""
    t0 = tensors[0]
    if padding is None:
        arr = torch.empty(tuple(shape), dtype=t0.dtype, device=t0.device)
    else:
        arr = torch.full(tuple(shape), padding, dtype=t0.dtype, device=t0.device)
    for t, sl in zip(tensors, slices):
        arr[sl] = t
    return arr


def _composed_ravel(tensors: Sequence[torch.Tensor], axes: Sequence[int]) -> torch.Tensor:
    """The flat form from a ``reshape`` of every tensor and one ``cat``."""
    lead = _last(tensors[0], axes).shape[: tensors[0].dim() - len(axes)]
    return torch.cat([_last(t, axes).reshape(*lead, math.prod(t.shape[ax] for ax in axes)) for t in tensors], dim=-1)


def _composed_to_bands(views: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """Fresh dense tensors of views of the array, one copy each."""
    return [v.clone(memory_format=torch.contiguous_format) for v in views]


# ---- the box table ------------------------------------------------------------------------------------------------------------------
def _merge(dims: Sequence[Tuple[int, int, Optional[int]]]):
    """``dims`` — (extent, destination stride, source stride or None) per axis, outermost first — as at most BOX_DIMS of them with a dense
    destination row, or None.  Axes of extent 1 go; neighbours merge where both sides step over them as one."""
    out: list = []
    for n, ds, ss in dims:
        if n == 1:
            continue
        if out and out[-1][1] == n * ds and (ss is None or out[-1][2] == n * ss):
            out[-1] = [out[-1][0] * n, ds, ss]
        else:
            out.append([n, ds, ss])
    if not out or out[-1][1] != 1:
        out.append([1, 1, None if not dims or dims[0][2] is None else 1])
    if len(out) > BOX_DIMS:
        return None
    return [[1, 0, None if out[0][2] is None else 0]] * (BOX_DIMS - len(out)) + out


class _Box:
    """One box of a launch: the merged dims, the destination tensor and the box's offset in it (in elements), the source view whose
    first element is the box's (None: filled)."""

    __slots__ = ("dims", "dst", "dst_off", "src")

    def __init__(self, dims, dst_off, src, dst=None):
        self.dims, self.dst, self.dst_off, self.src = dims, dst, dst_off, src


def _partition(groups: Sequence[Sequence[_Box]], ntens: Sequence[int]) -> List[List[_Box]]:
    """The launches of a call: ``groups`` of boxes (the approximation, then one group per level) with ``ntens`` tensors each, packed
    greedily into launches of whole groups within :func:`max_tensors` and :func:`max_boxes`; empty boxes go."""
    cap_t, cap_b = max_tensors(), max_boxes()
    launches: list = [[]]
    used = 0
    for g, nt in zip(groups, ntens):
        g = [b for b in g if all(d[0] > 0 for d in b.dims)]
        if launches[-1] and (used + nt > cap_t or len(launches[-1]) + len(g) > cap_b):
            launches.append([])
            used = 0
        # (a level of its own beyond the capacity, as in five dimensions: cut anywhere, a box has one writer wherever it runs)
        for c0 in range(0, len(g), cap_b):
            if c0:
                launches.append([])
            launches[-1].extend(g[c0:c0 + cap_b])
        used += nt
    return [boxes for boxes in launches if boxes]


def _launch(tag: str, kid: int, boxes: Sequence[_Box], esz: int, padding: bytes, anchor: torch.Tensor, numel: int) -> None:
    """One launch of kernel 59 / 60 over ``boxes`` (tests/test_pack_host.py replaces this with a CPU model of the kernel's map)."""
    arr = (_engine.PackBox * len(boxes))()
    for s, b in zip(arr, boxes):
        s.dst = b.dst.data_ptr() + b.dst_off * esz
        s.src = None if b.src is None else b.src.data_ptr()
        s.extent[:] = [d[0] for d in b.dims]
        s.src_stride[:] = [0 if d[2] is None else d[2] for d in b.dims]
        s.dst_stride[:] = [d[1] for d in b.dims[:-1]]
    if kid == KID_TO_ARRAY:
        pad = (ctypes.c_char * 16).from_buffer_copy(padding + bytes(16 - len(padding)))
        _engine._run(tag, kid, (numel,), anchor, _lib().mifwt_pack_to_array, (esz, arr, len(boxes), pad))
    else:
        _engine._run(tag, kid, (numel,), anchor, _lib().mifwt_pack_to_bands, (esz, arr, len(boxes)))


def _run_boxes(tag: str, kid: int, groups, ntens: Sequence[int], esz: int, padding: bytes, anchor: torch.Tensor, numel: int) -> None:
    for boxes in _partition(groups, ntens):
        _launch(tag, kid, boxes, esz, padding, anchor, numel)


def _within(esz: int, groups) -> bool:
    """Whether every box is inside the kernels' index range (``mifwt_pack_plan`` answers without a device)."""
    cap = max_boxes()
    boxes = [b for g in groups for b in g]
    for c0 in range(0, len(boxes), cap):
        part = boxes[c0:c0 + cap]
        arr = (_engine.PackBox * len(part))()
        for s, b in zip(arr, part):
            s.extent[:] = [d[0] for d in b.dims]
        if _lib().mifwt_pack_plan(esz, arr, len(part)) < 0:
            return False
    return True


def _padding_bytes(padding, dtype) -> bytes:
    return torch.tensor([0.0 if padding is None else padding], dtype=dtype).view(torch.uint8).numpy().tobytes()


def _region_dims(region, dst_strides, src_strides):
    return _merge([(n, ds, None if src_strides is None else src_strides[ax]) for ax, ((_, n), ds) in enumerate(zip(region, dst_strides))])


def _dense_strides(shape) -> List[int]:
    st, run = [], 1
    for n in reversed(shape):
        st.insert(0, run)
        run *= n
    return st


def _to_array_launch(p: _Parsed, shape, regions, gaps, padding) -> Optional[torch.Tensor]:
    """``arr`` through kernel 59, or None where the composed route serves the call."""
    a = p.approx
    st = _dense_strides(shape)
    off = lambda r: sum(s * q for (s, _), q in zip(r, st))
    groups: list = [[_Box(_region_dims(regions[0], st, a.stride()), off(regions[0]), a)]]
    ntens = [1]
    for lv, regs, gap in zip(p.levels, regions[1:], gaps):
        g = [_Box(_region_dims(regs[k], st, t.stride()), off(regs[k]), t) for k, t in lv.items()]
        g += [_Box(_region_dims(r, st, None), off(r), None) for r in gap]
        groups.append(g)
        ntens.append(len(lv))
    esz = a.element_size()
    if any(b.dims is None for g in groups for b in g) or not _within(esz, groups):
        return None
    arr = torch.empty(shape, dtype=a.dtype, device=a.device)
    for g in groups:
        for b in g:
            b.dst = arr
    if arr.numel():
        _run_boxes("pack_to_array", KID_TO_ARRAY, groups, ntens, esz, _padding_bytes(padding, a.dtype), arr, arr.numel())
    return arr


def _ravel_launch(p: _Parsed, lead, n: int, slices, shapes) -> Optional[torch.Tensor]:
    a = p.approx
    out_shape = tuple(lead) + (n,)
    lst = _dense_strides(out_shape)[:-1]

    def box(t, sl, tshape):
        tl = _last(t, p.axes)
        dims = [(s, q, tl.stride(i)) for i, (s, q) in enumerate(zip(lead, lst))]
        dims += [(s, q, tl.stride(len(lead) + i)) for i, (s, q) in enumerate(zip(tshape, _dense_strides(tshape)))]
        return _Box(_merge(dims), sl.start, t)

    groups: list = [[box(a, slices[0], shapes[0])]]
    for lv, sl, sh in zip(p.levels, slices[1:], shapes[1:]):
        groups.append([box(lv[k], sl[k], sh[k]) for k in sl])
    esz = a.element_size()
    if any(b.dims is None for g in groups for b in g) or not _within(esz, groups):
        return None
    arr = torch.empty(out_shape, dtype=a.dtype, device=a.device)
    for g in groups:
        for b in g:
            b.dst = arr
    if arr.numel():
        _run_boxes("pack_ravel", KID_TO_ARRAY, groups, [len(g) for g in groups], esz, _padding_bytes(0.0, a.dtype), arr, arr.numel())
    return arr


def _carve(shapes: Sequence[Tuple[int, ...]], dtype, device) -> List[torch.Tensor]:
    """Uninitialised contiguous tensors of ``shapes`` carved out of ONE allocation, every start rounded up to ALIGN_BYTES."""
    step = ALIGN_BYTES // torch.empty(0, dtype=dtype).element_size()
    offs, total = [], 0
    for shape in shapes:
        total = -(-total // step) * step
        offs.append(total)
        total += math.prod(shape)
    base = torch.empty(total, dtype=dtype, device=device)
    return [base[o:o + math.prod(shape)].view(shape) for o, shape in zip(offs, shapes)]


def _to_bands_launch(arr: torch.Tensor, views: Sequence[torch.Tensor], group_sizes: Sequence[int]) -> Optional[List[torch.Tensor]]:
    """Fresh dense copies of ``views`` (views of ``arr``; the approximation's, then ``group_sizes`` per level) through kernel 60, or None
    where the composed route serves the call."""
    outs = _carve([tuple(v.shape) for v in views], arr.dtype, arr.device)
    boxes = []
    for v, o in zip(views, outs):
        dims = _merge([(n, ds, ss) for n, ds, ss in zip(v.shape, o.stride(), v.stride())])
        boxes.append(_Box(dims, 0, v, o))
    it = iter(boxes)
    groups = [[next(it) for _ in range(size)] for size in (1, *group_sizes)]
    esz = arr.element_size()
    if any(b.dims is None for b in boxes) or not _within(esz, groups):
        return None
    if sum(v.numel() for v in views):
        _run_boxes("pack_to_bands", KID_TO_BANDS, groups, [len(g) for g in groups], esz, b"", arr, sum(v.numel() for v in views))
    return outs


# ---- autograd -------------------------------------------------------------------------------------------------------------------------
class _Gather(torch.autograd.Function):
    """The tensors of a container -> ``arr`` (either layout).  The gradient of a tensor is its view of the incoming gradient: ``take``
    maps ``g`` to the list of those views with differentiable torch operations, so the backward can be recorded itself."""

    @staticmethod
    def forward(ctx, run, take, *tensors):
        ctx.take = take
        return run([t.detach() for t in tensors])

    @staticmethod
    def backward(ctx, g):
        return (None, None, *[v if need else None for v, need in zip(ctx.take(g), ctx.needs_input_grad[2:])])


class _Scatter(torch.autograd.Function):
    """``arr`` -> fresh dense tensors (copy=True).  The gradient of ``arr``: the incoming gradients assigned to their slices of zeros;
    ``put`` does that with differentiable torch operations."""

    @staticmethod
    def forward(ctx, run, put, arr):
        ctx.put, ctx.like = put, (tuple(arr.shape), arr.dtype, arr.device)
        return tuple(run(arr.detach()))

    @staticmethod
    def backward(ctx, *gs):
        return None, None, ctx.put(gs, ctx.like)


def _wants_grad(tensors) -> bool:
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


def _flat(p: _Parsed, keys: Optional[Sequence[Sequence[str]]] = None) -> List[torch.Tensor]:
    return [p.approx] + [lv[k] for lv, ks in zip(p.levels, keys or p.levels) for k in ks]


# ---- the public functions ---------------------------------------------------------------------------------------------------------------
def coeffs_to_array(coeffs, padding=0.0, *, axes=None):
    """``pywt.coeffs_to_array``: the container as one fresh dense tensor ``arr`` in the layout of the module docstring, and ``slices`` —
    ``[tuple, {key: tuple}, ...]``, every tuple covering ALL axes of ``arr`` (``slice(None)`` on the leading ones), so
    ``arr[slices[1]["da"]]`` is the band.  One launch for the whole container, ``padding`` included; ``padding=None`` asks for tight
    packing and raises unless the blocks tile the array.  A container that holds only the approximation gives that tensor itself.

    ``ValueError`` for a ``None`` or missing band, bands of one level that differ in shape, tensors that differ in dtype, device or
    leading shape, another dtype than the six of the module docstring, blocks that would overlap (PyWavelets overwrites there), and for
    ``padding=None`` with a gap; ``RuntimeError`` for CPU tensors."""
    who = "coeffs_to_array"
    p = _parse(who, coeffs, axes)
    if p.kind == "approx":
        return p.approx, [tuple(slice(None) for _ in range(p.rank))]
    shape, slices, regions, gaps = _array_layout(who, p, padding is None)
    tensors = _flat(p)
    flat_slices = [slices[0]] + [sl[k] for sl in slices[1:] for k in sl]
    for t in tensors:
        _engine._require_gpu(t)

    def run(ts):
        q = p
        if ts is not tensors:
            q = _reparse(p, ts)
        out = None if _cell(who, p) in COMPOSED_CELLS else _to_array_launch(q, shape, regions, gaps, padding)
        return out if out is not None else _composed_to_array(ts, flat_slices, shape, padding)

    if _wants_grad(tensors):
        arr = _Gather.apply(run, lambda g: [g[sl] for sl in flat_slices], *tensors)
    else:
        arr = run(tensors)
    return arr, slices


def _cell(who: str, p: _Parsed):
    """The cell of COMPOSED_CELLS a call on the container ``p`` belongs to."""
    finest = next(iter(p.levels[-1].values()))
    return who, p.approx.dtype, p.d, finest.shape[-1] < SHORT_ROW


def _reparse(p: _Parsed, tensors: Sequence[torch.Tensor], keys=None) -> _Parsed:
    """``p`` over other tensors of the same geometry (the detached ones of a recorded call), given in the order of ``keys`` per level
    (None: container order)."""
    q = _Parsed()
    q.d, q.kind, q.axes, q.rank = p.d, p.kind, p.axes, p.rank
    it = iter(tensors)
    q.approx = next(it)
    q.levels = [{k: next(it) for k in ks} for ks in (keys or p.levels)]
    return q


def _check_slices(who: str, arr, slices) -> Tuple[int, List[List[str]]]:
    if not isinstance(arr, torch.Tensor):
        raise ValueError(f"{who}: arr is a tensor, got {type(arr).__name__}")
    if not isinstance(slices, (list, tuple)) or len(slices) == 0 or not all(isinstance(s, dict) and s for s in slices[1:]):
        raise ValueError(f"{who}: slices is what coeffs_to_array / ravel_coeffs returned: one entry for the approximation, then a dict per level")
    keys = [list(s) for s in slices[1:]]
    d = len(keys[0][0]) if keys else 0
    if any(len(k) != d for ks in keys for k in ks):
        raise ValueError(f"{who}: the keys of the slices have one length")
    return d, keys


def array_to_coeffs(arr, slices, output_format: str = "wavedecn", *, copy: bool = False):
    """``pywt.array_to_coeffs``: the container of ``output_format`` — ``"wavedec"`` the list of tensors, ``"wavedec2"`` the tensor plus
    ``WaveletDetailTuple2d``s, ``"wavedecn"`` the tensor plus dicts (in the key order of ``slices``) — over the blocks of ``arr``.
    ``copy=False`` (PyWavelets' behaviour): the bands are views of ``arr``; no kernel, any device, differentiable by construction.
    ``copy=True``: fresh dense tensors carved out of ONE backing allocation with 256-byte aligned starts, written by one launch.
    ``ValueError`` for an unknown format or one whose number of axes is not that of the slices."""
    who = "array_to_coeffs"
    d, keys = _check_slices(who, arr, slices)
    _check_format(who, output_format, d, keys)
    if not keys:
        return _container(output_format, arr, [])
    flat = [slices[0]] + [s[k] for s in slices[1:] for k in s]
    for sl in flat:
        if not isinstance(sl, tuple) or any(not isinstance(s, slice) or s.step not in (None, 1) for s in sl):
            raise ValueError(f"{who}: every entry of slices is a tuple of slices of step 1, got {sl!r}")
    views = [arr[sl] for sl in flat]
    if copy:
        views = _copied(who, arr, views, [len(k) for k in keys], d,
                        lambda gs, like: _assigned(like, [(sl, g) for sl, g in zip(flat, gs) if g is not None]))
    it = iter(views)
    approx = next(it)
    return _container(output_format, approx, [{k: next(it) for k in ks} for ks in keys])


def _assigned(like, parts) -> torch.Tensor:
    """Zeros of the (shape, dtype, device) ``like`` with ``g`` assigned to ``[index]`` for every (index, g): differentiable w.r.t. every
    ``g``."""
    out = torch.zeros(like[0], dtype=like[1], device=like[2])
    for index, g in parts:
        out[index] = g
    return out


def _copied(who: str, arr: torch.Tensor, views, group_sizes, d: int, put) -> List[torch.Tensor]:
    _engine._require_gpu(arr)
    if arr.dtype not in DTYPES:
        raise ValueError(f"{who}: dtype {arr.dtype} not supported (float32, float64, complex64, complex128, float16, bfloat16)")
    shapes = [tuple(v.shape) for v in views]
    index = [(v.storage_offset() - arr.storage_offset(), tuple(v.stride())) for v in views]

    def run(a):
        vs = views if a is arr else [a.as_strided(s, st, a.storage_offset() + o) for s, (o, st) in zip(shapes, index)]
        outs = None if (who, arr.dtype, d, views[-1].shape[-1] < SHORT_ROW) in COMPOSED_CELLS else _to_bands_launch(a, vs, group_sizes)
        return outs if outs is not None else _composed_to_bands(vs)

    if _wants_grad([arr]):
        return list(_Scatter.apply(run, put, arr))
    return run(arr)


def ravel_coeffs(coeffs, *, axes=None):
    """``pywt.ravel_coeffs``: ``(arr, slices, shapes)`` with ``arr`` ``[*lead, n]`` — the approximation, then level by level, coarsest
    first, within a level the bands in SORTED key order (``ad, da, dd``), each band row-major over its transformed axes in axis order —
    ``slices`` ``[slice, {key: slice}, ...]`` on the last axis and ``shapes`` the transformed extents in the same nesting.  One launch.
    For 2-D containers this order differs from the flat index of :func:`ptwt_amd.sparse_encode`, which follows container order
    (``da, ad, dd``).  A container that holds only the approximation gives that tensor itself, ``[slice(None)]`` and its shape.
    Errors as for :func:`coeffs_to_array`."""
    who = "ravel_coeffs"
    p = _parse(who, coeffs, axes)
    if p.kind == "approx":
        return p.approx, [slice(None)], [tuple(p.approx.shape)]
    lead, n, slices, shapes = _ravel_layout(p)
    keys = [list(sl) for sl in slices[1:]]
    tensors = _flat(p, keys)
    flat_slices = [slices[0]] + [sl[k] for sl in slices[1:] for k in sl]
    flat_shapes = [shapes[0]] + [sh[k] for sh in shapes[1:] for k in sh]
    for t in tensors:
        _engine._require_gpu(t)

    def run(ts):
        q = p if ts is tensors else _reparse(p, ts, keys)
        out = None if _cell(who, p) in COMPOSED_CELLS else _ravel_launch(q, lead, n, slices, shapes)
        return out if out is not None else _composed_ravel(ts, p.axes)

    def take(g):
        return [_unlast(g[..., sl].unflatten(-1, sh), p.axes) for sl, sh in zip(flat_slices, flat_shapes)]

    arr = _Gather.apply(run, take, *tensors) if _wants_grad(tensors) else run(tensors)
    return arr, slices, shapes


def unravel_coeffs(arr, slices, shapes, output_format: str = "wavedecn", *, copy: bool = False):
    """``pywt.unravel_coeffs``, the inverse of :func:`ravel_coeffs`: the container of ``output_format`` over the tensors
    ``arr[..., slice]`` reshaped to ``[*lead, *shape]`` — the transformed axes LAST, whatever ``axes`` the ravel was given.  ``copy`` as
    for :func:`array_to_coeffs`: views of ``arr`` by default, with ``copy=True`` fresh dense tensors out of one backing allocation
    written by one launch."""
    who = "unravel_coeffs"
    d, keys = _check_slices(who, arr, slices)
    _check_format(who, output_format, d, keys)
    if not keys:
        return _container(output_format, arr, [])
    if not isinstance(shapes, (list, tuple)) or len(shapes) != len(slices) or any(not isinstance(sh, dict) or list(sh) != list(sl)
                                                                                for sh, sl in zip(shapes[1:], slices[1:])):
        raise ValueError(f"{who}: shapes has the nesting and the keys of slices")
    flat = [slices[0]] + [s[k] for s in slices[1:] for k in s]
    flat_shapes = [tuple(shapes[0])] + [tuple(sh[k]) for sh in shapes[1:] for k in sh]
    for sl, sh in zip(flat, flat_shapes):
        if not isinstance(sl, slice) or sl.step not in (None, 1) or len(range(*sl.indices(arr.shape[-1]))) != math.prod(sh):
            raise ValueError(f"{who}: every entry of slices is a slice of step 1 on the last axis with the elements of its shape, got "
                             f"{sl!r} for {sh}")
    views = [arr[..., sl].unflatten(-1, sh) for sl, sh in zip(flat, flat_shapes)]
    if copy:
        def put(gs, like):
            return _assigned(like, [((Ellipsis, sl), g.flatten(-len(sh))) for sl, sh, g in zip(flat, flat_shapes, gs) if g is not None])

        views = _copied(who, arr, views, [len(k) for k in keys], d, put)
    it = iter(views)
    approx = next(it)
    return _container(output_format, approx, [{k: next(it) for k in ks} for ks in keys])


# ---- shapes without a transform (host only) -----------------------------------------------------------------------------------------
def wavedecn_shapes(shape, wavelet, mode="reflect", level: Optional[int] = None, axes=None):
    """``pywt.wavedecn_shapes``: the shapes ``wavedec`` / ``wavedec2`` / ``wavedec3`` (and ``fswavedec*``) return for an input of
    ``shape`` as ``[shape, {key: shape}, ...]``, coarsest level first, keys in sorted order (``"d"`` in 1-D) — from the arithmetic of
    the level drivers, without a transform or a device: ``floor((n + L - 1) / 2)`` coefficients per axis and level in the padded modes,
    ``ceil(n / 2)`` in ``"periodization"``.  ``axes=None``: every axis of ``shape``; otherwise the other axes are carried through.
    ``mode`` defaults to ``"reflect"``, the default of ``wavedec`` and ``wavedec2`` (``wavedec3``'s is ``"zero"``: the shapes of the
    padded modes are the same).  ``level=None`` is the transforms' default, ``dwtn_max_level``; the errors are the transforms':
    ``ValueError`` for an unknown mode, for repeated axes, for a negative level in ``"periodization"`` and the value-map modes,
    ``RuntimeError`` where ``reflect`` / ``periodic`` padding does not fit a level."""
    shape = tuple(int(s) for s in shape)
    if axes is None:
        axes = tuple(range(len(shape)))
    axes = (axes,) if isinstance(axes, int) else tuple(axes)
    d = len(axes)
    if d == 0 or any(not -len(shape) <= ax < len(shape) for ax in axes):
        raise ValueError(f"wavedecn_shapes: axes {axes} out of range for a shape of {len(shape)} axes")
    axes = tuple(ax % len(shape) for ax in axes)
    if len(set(axes)) != d:
        raise ValueError("Cant transform the same axis twice.")
    flen = _wavelets.filter_length(wavelet)
    per = isinstance(mode, str) and mode == _fwt.PERIODIZATION
    ext = isinstance(mode, str) and mode in _fwt.EXT_MODES
    if not (per or ext):
        _fwt._mode_id(mode)
    ns = [shape[ax] for ax in axes]
    if level is None:
        level = _wavelets.dwtn_max_level(ns, flen)
    elif level < 0 and (per or ext):
        raise ValueError(f"Level value of {level} is too low. Minimum level is 0.")
    if not (per or ext):
        _fwt._check_pad_levels(ns, flen, mode, level)
    keys = ["".join(k) for k in itertools.product("ad", repeat=d)][1:]

    def full(ext_):
        out = list(shape)
        for ax, n in zip(axes, ext_):
            out[ax] = n
        return tuple(out)

    levels: list = []
    for _ in range(level):
        ns = [(n + 1) // 2 if per else (n + flen - 1) // 2 for n in ns]
        levels.insert(0, {k: full(ns) for k in keys})
    return [full(ns)] + levels


def wavedecn_size(shapes) -> int:
    """``pywt.wavedecn_size``: the number of coefficients of a container with ``shapes`` (what :func:`wavedecn_shapes` or
    :func:`ravel_coeffs` returned)."""
    if not isinstance(shapes, (list, tuple)) or len(shapes) == 0:
        raise ValueError("wavedecn_size: shapes is what wavedecn_shapes returned")
    total = math.prod(shapes[0])
    for lv in shapes[1:]:
        total += sum(math.prod(s) for s in (lv.values() if isinstance(lv, dict) else [lv]))
    return int(total)
