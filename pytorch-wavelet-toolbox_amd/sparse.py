"""The k kept coefficients of every image, compacted — ``(values, indices)`` and back (C ABI ``mifwt_compact_*``, include/mifwt.h; kernels
csrc/mifwt_compact.hip, ids 56 .. 58).

    coeffs = ptwt_amd.wavedec2(x, "db4", level=3)
    s = ptwt_amd.sparse_encode(coeffs, 0.05)          # the largest 5 % of the detail coefficients of every image: values + positions
    del coeffs                                        # s holds no reference to the dense details
    y = ptwt_amd.waverec2(ptwt_amd.sparse_decode(s), "db4")

``coeffs``, ``keep`` and ``approx`` mean what they mean in :func:`ptwt_amd.keep_threshold` / :func:`ptwt_amd.sparsify`: the pooled tensors
of one leading index (one image) form ONE pool of ``n`` elements.  The FLAT INDEX of a pooled element is its position in that pool: the
pooled tensors in container order, tensor ``t`` at ``[off_t, off_t + n_t)``, inside it the row-major index of the element within its image.

Selection rule, per image, for ``k`` clipped to ``[0, min(n, K)]``: with ``v = keep_threshold`` of the image, every element with
``|x| > v`` is kept, and of the elements with ``|x| == v`` the first ``k - #{|x| > v}`` in flat-index order — compared on the bit pattern
with the sign cleared.  Exactly ``k`` elements per image; with ``k = 0`` none.  NaN inputs are unspecified.

:class:`SparseCoeffs` holds ``values`` ``[*lead, K]`` (the ORIGINAL values: hard selection, no shrinkage), ``indices`` ``[*lead, K]`` (int32,
ascending flat indices), ``counts`` ``[*lead]`` (int32, the clipped ``k``), slots ``j >= counts`` holding value 0 and index -1, ``approx``
(the approximation where it stayed out of the pool: the same object, dense) and a host-side ``layout``.  The capacity ``K`` is ``k`` for a
Python ``keep`` (or ``capacity >= k``) and the required ``capacity`` for a tensor ``keep``, which is read on the device.

Everything is written on the device and enqueued on the caller's stream: nothing is copied to the host, nothing synchronises, a call can
be captured (``ptwt_amd.capture``).  No atomics: two runs give the same bits.  After the selection (sparsify.py) a pool of at most
``estimators.lds_capacity`` elements per image in at most :func:`max_segments` tensors is compacted by one workgroup per image from LDS
(id 56); anything else by a count launch, a scan launch and a write launch over the unit table of the streaming selection (id 57).
``FORCE_STREAM`` sends every size down the streaming selection and compaction.  ``sparse_decode`` is one fill of ONE backing allocation
(every tensor's start rounded up to 256 bytes) and one scatter launch (id 58) per :func:`max_segments` tensors.  Beyond the kernels'
envelope (the collapsed form of ``thresholding._form``) and while a backward is itself recorded, the calls are composed from torch
operations (:func:`_composed_encode` / :func:`_composed_decode`).  float32 and float64 data only, fewer than 2^31 pooled elements per image.
"""
from __future__ import annotations

import ctypes
import importlib
import itertools
import math
import numbers
from typing import List, Optional, Sequence, Tuple

import torch

from . import _engine
from . import estimators as _est
from . import thresholding as _thr

# (the package attribute ``sparsify`` is the function: the module is reached through the import system)
_sp = importlib.import_module(__package__ + ".sparsify")

__all__ = ["SparseCoeffs", "sparse_encode", "sparse_decode"]

KID_COMPACT_LDS, KID_COMPACT_STREAM, KID_COMPACT_MOVE = 56, 57, 58
#: test / tool switch: the streaming selection (id 55) and compaction (id 57) at every size
FORCE_STREAM = False
#: (dtype, pooled elements per leading index) cells inside the LDS route's envelope that take the streaming route all the same, and cells
#: that are composed from torch operations instead of the kernels: a cell belongs there only where tools/sparse_bench.py has shown the
#: default's median behind by more than the spread of its windows.  Empty: the LDS route led the streaming one, and both led the
#: composition, in every cell measured (EXPERIMENTS part L).
STREAM_CELLS: set = set()
COMPOSED_CELLS: set = set()
_INDEX_LIMIT = 1 << 31
ALIGN_BYTES = 256  # start of every tensor in the backing allocation of a decode

_entries = None


def _lib():
    global _entries
    if _entries is None:
        _entries = _engine.private_entries(_engine.COMPACT_ENTRIES)
    return _entries


def max_segments() -> int:
    """Tensors one count / write / scatter launch takes (``mifwt_compact_max_segments``)."""
    return int(_lib().mifwt_compact_max_segments())


# ---- the compacted form -------------------------------------------------------------------------------------------------------------
class _Frozen:
    __slots__ = ()

    def __init__(self, **fields):
        for name, value in fields.items():
            object.__setattr__(self, name, value)

    def __setattr__(self, name, value):
        raise AttributeError(f"{type(self).__name__} is immutable")

    def __delattr__(self, name):
        raise AttributeError(f"{type(self).__name__} is immutable")


class Layout(_Frozen):
    """Host-side description of an encoded container: ``skeleton`` (the container with every pooled tensor replaced by its number and an
    approximation that stayed out of the pool by ``None``), ``dtype``, ``device``, ``lead`` (the leading shape), ``entries`` (per pooled
    tensor its shape and the flat index of its first element), ``n`` (pooled elements per image) and ``capacity``.  No tensor."""

    __slots__ = ("skeleton", "dtype", "device", "lead", "entries", "n", "capacity")

    def __repr__(self):
        return f"Layout(tensors={len(self.entries)}, lead={self.lead}, n={self.n}, capacity={self.capacity}, dtype={self.dtype})"


class SparseCoeffs(_Frozen):
    """What :func:`sparse_encode` returns: ``values`` [*lead, K], ``indices`` [*lead, K] (int32, ascending flat indices, -1 in the padding),
    ``counts`` [*lead] (int32), ``approx`` (the dense approximation where it stayed out of the pool, else None), ``layout``."""

    __slots__ = ("values", "indices", "counts", "approx", "layout")

    def __repr__(self):
        return f"SparseCoeffs(values={tuple(self.values.shape)}, {self.layout!r})"


def _skeleton(coeffs, whole: bool):
    if isinstance(coeffs, torch.Tensor):
        return 0
    numbers_ = itertools.count()
    return type(coeffs)([None if i == 0 and not whole else _thr._rebuild(e, numbers_) for i, e in enumerate(coeffs)])


def _filled(obj, outs: Sequence[torch.Tensor], approx):
    """The container of a skeleton over the tensors ``outs``."""
    if obj is None:
        return approx
    if isinstance(obj, int):
        return outs[obj]
    if isinstance(obj, dict):
        return {k: _filled(v, outs, approx) for k, v in obj.items()}
    if isinstance(obj, tuple) and hasattr(obj, "_fields"):
        return type(obj)(*[_filled(v, outs, approx) for v in obj])
    return type(obj)(_filled(v, outs, approx) for v in obj)


def _capacity(capacity, n: int) -> int:
    if isinstance(capacity, bool) or not isinstance(capacity, numbers.Integral) or not 0 <= capacity <= n:
        raise ValueError(f"sparse_encode: capacity is an int in [0, {n}] (the pooled coefficients per image), got {capacity!r}")
    return int(capacity)


# ---- composed from torch operations -------------------------------------------------------------------------------------------------
def _live(indices: torch.Tensor, counts: torch.Tensor, n: int) -> torch.Tensor:
    """[images, K] which slots name an element: below the image's count, index inside the pool."""
    j = torch.arange(indices.shape[1], device=indices.device)
    return (j.unsqueeze(0) < counts.reshape(-1, 1)) & (indices >= 0) & (indices < n)


def _composed_encode(tensors: Sequence[torch.Tensor], lead: int, k: int, dk: Optional[torch.Tensor], cap: int):
    """(values [images, K], indices, counts) of the pooled ``tensors`` from torch operations — ``cat``, a stable descending ``sort`` of the
    magnitudes (every greater element, then the earliest ties), a ``sort`` of the chosen positions, a ``gather``: the route beyond the
    kernels' limits, of a recorded backward, and the emulation the benchmark compares the kernels with.  Differentiable w.r.t. the data.
    ``dk``: the flat int64 tensor of ``sparsify._keep`` instead of ``k``."""
    images = math.prod(tensors[0].shape[:lead])
    flat = torch.cat([t.reshape(images, -1) for t in tensors], 1)
    n = flat.shape[1]
    order = flat.detach().abs().sort(dim=1, descending=True, stable=True).indices[:, :cap]
    kk = torch.full((images,), k, dtype=torch.int64, device=flat.device) if dk is None else dk.clamp(0, min(n, cap)).expand(images)
    live = torch.arange(cap, device=flat.device).unsqueeze(0) < kk.unsqueeze(1)
    idx = torch.where(live, order, n).sort(1).values  # (ascending; the padding, n, goes last: `live` holds before and after)
    values = torch.where(live, flat.gather(1, idx.clamp(max=n - 1)), torch.zeros((), dtype=flat.dtype, device=flat.device))
    return values, torch.where(live, idx, -1).to(torch.int32), kk.to(torch.int32)


def _composed_decode(values: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor, shapes: Sequence[Tuple[int, ...]], n: int):
    """The dense tensors of ``shapes`` (together ``n`` elements per image) from torch operations: ``zeros`` and a ``scatter``.
    Differentiable w.r.t. ``values``."""
    cap = values.shape[-1]
    v, idx = values.reshape(-1, cap), indices.reshape(-1, cap).long()
    images = v.shape[0]
    live = _live(idx, counts, n)
    zero = torch.zeros((), dtype=v.dtype, device=v.device)
    flat = torch.zeros((images, n + 1), dtype=v.dtype, device=v.device).scatter(1, torch.where(live, idx, n), torch.where(live, v, zero))
    outs, off = [], 0
    for shape in shapes:
        m = math.prod(shape) // images if images else 0
        outs.append(flat[:, off:off + m].reshape(shape))
        off += m
    return outs


def _composed_gather(tensors: Sequence[torch.Tensor], indices: torch.Tensor, counts: torch.Tensor, n: int) -> torch.Tensor:
    """values [images, K] = the elements of the dense ``tensors`` at ``indices``, 0 in the padding; differentiable w.r.t. ``tensors``."""
    cap = indices.shape[-1]
    idx = indices.reshape(-1, cap).long()
    flat = torch.cat([t.reshape(idx.shape[0], -1) for t in tensors], 1)
    return torch.where(_live(idx, counts, n), flat.gather(1, idx.clamp(0, n - 1)), torch.zeros((), dtype=flat.dtype, device=flat.device))


# ---- launches -----------------------------------------------------------------------------------------------------------------------
def _empty_result(images: int, cap: int, dtype, device):
    return (torch.zeros((images, cap), dtype=dtype, device=device), torch.full((images, cap), -1, dtype=torch.int32, device=device),
            torch.zeros((images,), dtype=torch.int32, device=device))


def _encode_flat(xs: Sequence[torch.Tensor], lead: int, n: int, k: int, dk: Optional[torch.Tensor], cap: int):
    """(values [images, K], indices [images, K], counts [images]) of the pooled tensors ``xs`` (detached): the selection, then the
    compaction.  ``dk``: the flat int64 tensor of ``sparsify._keep`` instead of ``k``."""
    t0 = xs[0]
    images = math.prod(t0.shape[:lead])
    if images == 0 or n == 0 or cap == 0:  # shapes and dtypes only: no launch
        return _empty_result(images, cap, t0.dtype, t0.device)
    if dk is not None:
        dk = dk.clamp(0, cap)  # (on the device: the selection and the compaction read the same clipped k)
    live = [t.detach() for t in xs if t.numel()]
    bands = [_est._band(t, lead) for t in live]
    cell = (t0.dtype, n)
    if any(b is None for b in bands) or cell in COMPOSED_CELLS:
        with torch.no_grad():
            return _composed_encode(live, lead, k, dk, cap)
    dt = _engine._DTYPE_IDS[t0.dtype]
    arr = (_engine.EstimBand * len(bands))()
    for b, band in zip(arr, bands):
        _est._fill(b, band)
    force = int(bool(FORCE_STREAM) or cell in STREAM_CELLS)
    sel, lib = _sp._lib(), _lib()
    route = int(sel.mifwt_select_route(dt, arr, len(bands), images, force))
    croute = int(lib.mifwt_compact_route(dt, arr, len(bands), images, force))
    if route <= 0 or croute <= 0:
        _engine._check(min(route, croute) if min(route, croute) < 0 else -1)
    anchor = bands[0][0]
    ksrc = (k, dk.data_ptr() if dk is not None else None, int(dk is not None and dk.numel() > 1))
    v = torch.empty(images, dtype=t0.dtype, device=t0.device)
    _engine._run("select_kth", route, (images, n), anchor, sel.mifwt_select_kth, (dt, arr, len(bands), images, *ksrc, route, v.data_ptr(), None),
                 ws_bytes=int(sel.mifwt_select_workspace(dt, arr, len(bands), images, route)))
    values = torch.empty((images, cap), dtype=t0.dtype, device=t0.device)
    indices = torch.empty((images, cap), dtype=torch.int32, device=t0.device)
    counts = torch.empty((images,), dtype=torch.int32, device=t0.device)
    _engine._run("compact_encode", croute, (images, n), anchor, lib.mifwt_compact_encode,
                 (dt, arr, len(bands), images, *ksrc, cap, croute, v.data_ptr(), values.data_ptr(), indices.data_ptr(), counts.data_ptr()),
                 ws_bytes=int(lib.mifwt_compact_workspace(dt, arr, len(bands), images, croute)))
    return values, indices, counts


def _carve(shapes: Sequence[Tuple[int, ...]], dtype, device) -> List[torch.Tensor]:
    """Zero-filled contiguous tensors of ``shapes`` carved out of ONE allocation, every start rounded up to ALIGN_BYTES: one fill."""
    step = ALIGN_BYTES // torch.empty(0, dtype=dtype).element_size()
    offs, total = [], 0
    for shape in shapes:
        total = -(-total // step) * step
        offs.append(total)
        total += math.prod(shape)
    base = torch.zeros(total, dtype=dtype, device=device)
    return [base[o:o + math.prod(shape)].view(shape) for o, shape in zip(offs, shapes)]


def _move(gather: bool, dense: Sequence[torch.Tensor], values: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor) -> None:
    """Scatter ``values`` into / gather them from the contiguous tensors ``dense`` ([images, ...] each) at ``indices`` (kernel 58)."""
    images, cap = values.shape
    dense = [t for t in dense if t.numel()]
    ptrs = (ctypes.c_void_p * len(dense))(*[t.data_ptr() for t in dense])
    sizes = (ctypes.c_int64 * len(dense))(*[t.numel() // images for t in dense])
    _engine._run("compact_gather" if gather else "compact_scatter", KID_COMPACT_MOVE, (images, cap), values, _lib().mifwt_compact_move,
                 (_engine._DTYPE_IDS[values.dtype], int(gather), ptrs, sizes, len(dense), images, cap, values.data_ptr(), indices.data_ptr(),
                  counts.data_ptr()))


def _scatter(values: torch.Tensor, indices: torch.Tensor, counts: torch.Tensor, shapes: Sequence[Tuple[int, ...]], n: int):
    """Fresh dense tensors of ``shapes``: zeros except ``values`` at ``indices`` — one fill, one scatter launch per ``max_segments``."""
    cap = values.shape[-1]
    outs = _carve(shapes, values.dtype, values.device)
    images = math.prod(values.shape[:-1])
    if images and n and cap:
        _move(False, outs, values.detach().reshape(images, cap).contiguous(), indices.reshape(images, cap).contiguous(),
              counts.reshape(images).contiguous())
    return outs


def _gather(dense: Sequence[torch.Tensor], indices: torch.Tensor, counts: torch.Tensor, n: int) -> torch.Tensor:
    """values [images, K] of the dense tensors at ``indices``, 0 in the padding (kernel 58)."""
    images, cap = indices.shape
    values = torch.zeros((images, cap), dtype=dense[0].dtype, device=dense[0].device)
    if images and n and cap:
        _move(True, [t.detach().contiguous() for t in dense], values, indices, counts)
    return values


# ---- autograd -------------------------------------------------------------------------------------------------------------------------
class _Encode(torch.autograd.Function):
    """The pooled tensors -> (values, indices, counts).  ``grad_x`` is the scatter of ``grad_values``; indices and counts are constants."""

    @staticmethod
    def forward(ctx, cfg, *xs):
        lead, n, k, dk, cap = cfg
        values, indices, counts = _encode_flat(xs, lead, n, k, dk, cap)
        ctx.shapes, ctx.n = [tuple(x.shape) for x in xs], n
        ctx.save_for_backward(indices, counts)
        ctx.mark_non_differentiable(indices, counts)
        return values, indices, counts

    @staticmethod
    def backward(ctx, gv, _gi, _gc):
        indices, counts = ctx.saved_tensors
        if gv is None:
            return (None,) * (1 + len(ctx.shapes))
        if torch.is_grad_enabled():  # the backward itself is being recorded: the composed route, differentiated by autograd
            gx = _composed_decode(gv, indices, counts, ctx.shapes, ctx.n)
        else:
            gx = _scatter(gv, indices, counts, ctx.shapes, ctx.n)
        return (None, *[g if need else None for g, need in zip(gx, ctx.needs_input_grad[1:])])


class _Decode(torch.autograd.Function):
    """values -> the dense tensors.  ``grad_values`` is the gather of the incoming gradients at ``indices``, 0 in the padding."""

    @staticmethod
    def forward(ctx, cfg, values, indices, counts):
        shapes, n = cfg
        ctx.cfg = cfg
        ctx.save_for_backward(indices, counts)
        return tuple(_scatter(values, indices, counts, shapes, n))

    @staticmethod
    def backward(ctx, *gouts):
        shapes, n = ctx.cfg
        indices, counts = ctx.saved_tensors
        if all(g is None for g in gouts):
            return None, None, None, None
        like = next(g for g in gouts if g is not None)
        gs = [torch.zeros(shape, dtype=like.dtype, device=like.device) if g is None else g for g, shape in zip(gouts, shapes)]
        cap = indices.shape[-1]
        flat_idx, flat_counts = indices.reshape(-1, cap), counts.reshape(-1)
        if torch.is_grad_enabled():
            gv = _composed_gather(gs, flat_idx, flat_counts, n)
        else:
            gv = _gather(gs, flat_idx.contiguous(), flat_counts.contiguous(), n)
        return None, gv.reshape(indices.shape), None, None


def _arguments(coeffs, keep, approx: bool, capacity):
    """Everything the host decides before a device is needed: (all tensors, the pooled ones, leading axes, leading shape, n, k, the flat
    keep tensor or None, K)."""
    leaves, pooled, lead, shape, n = _sp._pool(coeffs, approx, None)
    if n >= _INDEX_LIMIT:
        raise ValueError(f"sparse_encode: the indices are int32: fewer than 2^31 pooled coefficients per image, got {n}")
    k, dk = _sp._keep(keep, n, shape, leaves[0].device)
    if dk is not None:
        if capacity is None:
            raise ValueError("sparse_encode: a tensor keep is read on the device: capacity (slots per image, an int in [0, n]) is required")
        cap = _capacity(capacity, n)
    else:
        cap = k if capacity is None else _capacity(capacity, n)
        if cap < k:
            raise ValueError(f"sparse_encode: capacity {cap} is below k = {k}")
    return leaves, [leaves[i] for i in pooled], lead, shape, n, k, dk, cap


def _layout(coeffs, xs: Sequence[torch.Tensor], lead: int, whole: bool, cap: int) -> Layout:
    """The :class:`Layout` of ``coeffs`` whose pooled tensors are ``xs``."""
    first = xs[0] if xs else _thr._flatten(coeffs)[0][0]
    entries, off = [], 0
    for t in xs:
        entries.append((tuple(t.shape), off))
        off += math.prod(t.shape[lead:])
    return Layout(skeleton=_skeleton(coeffs, whole), dtype=first.dtype, device=first.device, lead=tuple(first.shape[:lead]),
                  entries=tuple(entries), n=off, capacity=cap)


# ---- the public functions ---------------------------------------------------------------------------------------------------------------
def sparse_encode(coeffs, keep, *, approx: bool = False, capacity: Optional[int] = None) -> SparseCoeffs:
    """The ``k`` largest coefficients of every image of a tensor or coefficient container as :class:`SparseCoeffs`: their original values
    and their ascending flat indices in the image's pool (module docstring), exactly ``k`` per image — at a tied k-th magnitude the
    earliest ties in flat-index order.  ``coeffs``, ``keep``, ``approx`` and the errors as for :func:`ptwt_amd.keep_threshold`.

    The capacity ``K`` (slots per image) is ``k`` for an ``int`` / ``float`` ``keep``, or ``capacity >= k``; a tensor ``keep`` needs
    ``capacity`` (an int in [0, n]) and is read on the device, clipped to ``[0, min(n, capacity)]`` there.  Slots ``j >= counts`` hold
    value 0 and index -1.  ``K == 0``, an empty pool and a zero-size leading axis give empty / padded tensors without a launch.  The
    result keeps no reference to the pooled tensors.  Differentiable w.r.t. the data (the gradient of ``values`` scattered back);
    indices and counts are constants.  ``ValueError`` also for a missing or out-of-range ``capacity`` and for a pool of 2^31 or more
    elements per image (the indices are int32)."""
    leaves, xs, lead, shape, n, k, dk, cap = _arguments(coeffs, keep, approx, capacity)
    for t in leaves:
        _engine._require_gpu(t)
    whole = isinstance(coeffs, torch.Tensor) or approx
    first = leaves[0]
    layout = _layout(coeffs, xs, lead, whole, cap)
    if not xs:
        values, indices, counts = _empty_result(math.prod(shape), cap, first.dtype, first.device)
    elif torch.is_grad_enabled() and any(x.requires_grad for x in xs):
        values, indices, counts = _Encode.apply((lead, n, k, dk, cap), *xs)
    else:
        values, indices, counts = _encode_flat(xs, lead, n, k, dk, cap)
    return SparseCoeffs(values=values.reshape(shape + (cap,)), indices=indices.reshape(shape + (cap,)), counts=counts.reshape(shape),
                        approx=None if whole else coeffs[0], layout=layout)


def sparse_decode(s: SparseCoeffs):
    """The container :func:`sparse_encode` compacted — same types, keys and named tuples — over fresh contiguous tensors that hold zeros
    except the kept values; ``s.approx`` is returned as the same object.  All pooled outputs are carved out of ONE backing allocation,
    every start rounded up to 256 bytes: one fill and one scatter launch per :func:`max_segments` tensors.  Equal to
    ``sparsify(coeffs, keep, "hard")`` bit for bit wherever the k-th magnitude is not tied.  Differentiable w.r.t. ``s.values``."""
    if not isinstance(s, SparseCoeffs):
        raise TypeError(f"sparse_decode: expected SparseCoeffs, got {type(s).__name__}")
    lay = s.layout
    want = tuple(lay.lead) + (lay.capacity,)
    if tuple(s.values.shape) != want or tuple(s.indices.shape) != want or tuple(s.counts.shape) != tuple(lay.lead):
        raise ValueError(f"sparse_decode: values and indices have the shape {want} and counts {tuple(lay.lead)} of the layout")
    if s.values.dtype != lay.dtype or s.indices.dtype != torch.int32 or s.counts.dtype != torch.int32:
        raise ValueError(f"sparse_decode: values are {lay.dtype}, indices and counts int32")
    for t in (s.values, s.indices, s.counts):
        _engine._require_gpu(t)
    shapes = [shape for shape, _ in lay.entries]
    if torch.is_grad_enabled() and s.values.requires_grad:
        outs = _Decode.apply((shapes, lay.n), s.values, s.indices, s.counts)
    else:
        outs = _scatter(s.values, s.indices, s.counts, shapes, lay.n)
    return _filled(lay.skeleton, outs, s.approx)
