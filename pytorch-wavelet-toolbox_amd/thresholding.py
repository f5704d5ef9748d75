"""Coefficient thresholding — ``pywt.threshold`` and ``pywt.threshold_firm`` on tensors and on whole coefficient containers, one HIP
launch per container (C ABI ``mifwt_thresh_*``, include/mifwt.h; kernels csrc/mifwt_thresh.hip, ids 48 / 49).

    coeffs = ptwt_amd.wavedec2(x, "db4", level=3)
    shrunk = ptwt_amd.threshold(coeffs, [None, 0.3, 0.2, 0.1], "soft")      # per level, the approximation spared
    y = ptwt_amd.waverec2(shrunk, "db4")

The definitions are PyWavelets'.  With ``m = |x|`` (complex data: the magnitude of the complex number):

    soft      x max(1 - v / m, 0), which is sign(x) (m - v) for m > v and 0 otherwise
    hard      x where m >= v, else ``substitute``
    garrote   x max(1 - v^2 / m^2, 0)
    greater   x where x >= v, else ``substitute``     (real data only)
    less      x where x <= v, else ``substitute``     (real data only)
    firm      0 for m <= v_lo;  x v_hi (1 - v_lo / m) / (v_hi - v_lo) for v_lo < m <= v_hi;  x for m > v_hi

``soft`` and ``garrote`` return ``substitute`` where ``m < v``, but only when ``substitute != 0``.  ``x = 0`` gives 0: numpy's ``0 / 0``
NaN at ``v = 0`` is deliberately NOT reproduced.  ``v_hi == v_lo`` is hard thresholding at that value with substitute 0; nothing is
divided.  The arithmetic is float32 for float32, complex64 and (inside ``half_storage()``) float16 / bfloat16 data, whose result is
rounded once, and float64 for float64 and complex128; number thresholds are rounded to that type first.

A threshold is a number, a one-element tensor on the data's device, or a LEADING-FORM tensor: ``value.shape == t.shape[:value.dim()]``
with ``value.dim() < t.dim()``, one threshold per leading index (per image, say), which fits every tensor of a container because they
share their leading axes.  (This is an extension; numpy's trailing broadcasting would read such a shape differently.)  For a container
it may also be a sequence with one entry — a number, a tensor, or ``None`` — per container entry; ``None`` returns that entry's tensors
as they are, the same objects.  A single value on a container applies to EVERY tensor, the approximation included, which is what
mapping ``pywt.threshold`` over the container does.  Threshold tensors are read on the device when the kernel runs: nothing is copied
to the host, nothing synchronises, a call can be captured (``ptwt_amd.capture``) and sees the values the tensor holds at replay time.
Tensor thresholds are therefore not checked for sign or order.

Size: a kernel row holds at most 2^30 elements and a tensor fewer than 2^31 rows.  A dense tensor beyond 2^30 elements, whose axes
would merge into one longer row, is cut back into equal rows that respect the thresholds' leading axes (``_split_row``); only a tensor
with no such cut — a single axis of a length above 2^30 without a divisor in [n / 2^30, 2^16], or one that already needs all three
extents — is composed from torch operations (:func:`_composed`) instead.

Gradients: first order w.r.t. real data and threshold tensors runs on the backward kernel (``d/dx`` and, per threshold index, the sum of
``g dT/dv``: float32 runs of at most 16 terms per thread, float64 from there on, no atomics).  ``hard`` / ``greater`` / ``less`` give the
thresholds a zero gradient; ``substitute`` gets none.  While the backward itself is recorded (``create_graph=True``), and for complex
data that requires grad, the call is composed from torch operations with the same closed forms (:func:`_composed`), so gradients of any
order exist there.
"""
from __future__ import annotations

import ctypes
import functools
import numbers
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _engine
from .constants import supported_dtypes

__all__ = ["threshold", "threshold_firm"]

KID_FWD, KID_BWD = 48, 49
#: ``mode`` of the C ABI (MIFWT_THRESH_*)
MODES = {"soft": 0, "hard": 1, "garrote": 2, "greater": 3, "less": 4}
FIRM = 5
_HAS_VGRAD = (0, 2, FIRM)
_COMPLEX = {torch.complex64: torch.float32, torch.complex128: torch.float64}


class Seg(ctypes.Structure):
    """``mifwt_thresh_seg``."""

    _fields_ = [
        ("x", ctypes.c_void_p),
        ("y", ctypes.c_void_p),
        ("g", ctypes.c_void_p),
        ("extent", ctypes.c_int64 * 3),
        ("x_stride", ctypes.c_int64 * 3),
        ("y_stride", ctypes.c_int64 * 3),
        ("g_stride", ctypes.c_int64 * 3),
        ("value", ctypes.c_double * 2),
        ("dvalue", ctypes.c_void_p * 2),
        ("rows_per_value", ctypes.c_int64 * 2),
        ("gvalue", ctypes.c_void_p * 2),
    ]


_seg_p = ctypes.POINTER(Seg)
THRESH_ENTRIES: dict = {
    "mifwt_thresh_max_segments": (ctypes.c_int, []),
    "mifwt_thresh_plan": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int, _seg_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
    "mifwt_thresh_fwd": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, _seg_p, ctypes.c_int, ctypes.c_void_p]),
    "mifwt_thresh_bwd": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _seg_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
}
_entries = None


def _lib():
    global _entries
    if _entries is None:
        _entries = _engine.private_entries(THRESH_ENTRIES)
    return _entries


def max_segments() -> int:
    """Tensors one launch takes (``mifwt_thresh_max_segments``)."""
    return int(_lib().mifwt_thresh_max_segments())


_plans: dict = {}
_engine._routing_caches.append(_plans)


# ---- containers ------------------------------------------------------------------------------------------------------------------
def _walk(obj, entry: int, leaves: List[torch.Tensor], owner: List[int]) -> None:
    """(A module-level function, not a closure of :func:`_flatten`: a nested function that calls itself is a reference cycle, and one
    that also closes over ``leaves`` kept every input tensor of a call alive until the cyclic collector ran — a batch of 8 GiB stayed
    allocated after ``threshold`` had returned and its caller had dropped it.)"""
    if isinstance(obj, torch.Tensor):
        leaves.append(obj)
        owner.append(entry)
    elif isinstance(obj, dict):
        for v in obj.values():
            _walk(v, entry, leaves, owner)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _walk(v, entry, leaves, owner)
    else:
        raise TypeError(f"threshold: a coefficient container holds tensors, tuples and dicts of tensors, not {type(obj).__name__}")


def _flatten(data) -> Tuple[List[torch.Tensor], List[int], int]:
    """(the tensors of a container in order, the container entry each belongs to, the number of entries); a tensor is one entry."""
    leaves: List[torch.Tensor] = []
    owner: List[int] = []
    if isinstance(data, torch.Tensor):
        _walk(data, 0, leaves, owner)
        return leaves, owner, 1
    if not isinstance(data, (list, tuple)):
        raise TypeError(f"threshold: expected a tensor or a coefficient container, got {type(data).__name__}")
    for i, e in enumerate(data):
        _walk(e, i, leaves, owner)
    return leaves, owner, len(data)


def _rebuild(data, outs):
    """The container of ``data`` — same types, keys and order — over the tensors of the iterator ``outs``."""
    if isinstance(data, torch.Tensor):
        return next(outs)
    if isinstance(data, dict):
        return {k: _rebuild(v, outs) for k, v in data.items()}
    if isinstance(data, tuple) and hasattr(data, "_fields"):
        return type(data)(*[_rebuild(v, outs) for v in data])
    return type(data)(_rebuild(v, outs) for v in data)


# ---- thresholds ------------------------------------------------------------------------------------------------------------------
def _arith(dtype: torch.dtype) -> torch.dtype:
    return torch.float64 if dtype in (torch.float64, torch.complex128) else torch.float32


def _check_value(name: str, v, leaves: Sequence[torch.Tensor]):
    """One threshold of one container entry: a number (checked, returned as float) or a tensor (its form checked against every tensor of
    the entry)."""
    if isinstance(v, torch.Tensor):
        if v.is_complex() or v.dtype == torch.bool:
            raise ValueError(f"threshold: {name} must be real, got a {v.dtype} tensor")
        for t in leaves:
            if v.device != t.device:
                raise ValueError(f"threshold: a tensor {name} must live on the data's device ({t.device}), got {v.device}")
            if v.numel() != 1 and not (v.dim() < t.dim() and tuple(v.shape) == tuple(t.shape[: v.dim()])):
                raise ValueError(f"threshold: a tensor {name} has one element or the LEADING shape of the data: {tuple(v.shape)} is no "
                                 f"leading part of {tuple(t.shape)}")
        return v
    if isinstance(v, numbers.Real) and not isinstance(v, bool):
        v = float(v)
        if not v >= 0.0:
            raise ValueError(f"threshold: {name} must be non-negative, got {v}")
        return v
    raise ValueError(f"threshold: {name} must be a number or a tensor, got {type(v).__name__}")


def _per_entry(name: str, value, is_container: bool, nentries: int) -> list:
    if is_container and isinstance(value, (list, tuple)):
        if len(value) != nentries:
            raise ValueError(f"threshold: a sequence {name} has one entry per container entry: {len(value)} for {nentries}")
        return list(value)
    if value is None:
        raise ValueError(f"threshold: {name} is None (None is an entry of a per-entry sequence)")
    return [value] * nentries


def _round(v: float, arith: torch.dtype) -> float:
    return float(np.float32(v)) if arith == torch.float32 else v


def _lead(v, t: torch.Tensor) -> int:
    """Leading axes of ``t`` a tensor threshold indexes (0: one value)."""
    return 0 if not isinstance(v, torch.Tensor) or v.numel() == 1 else v.dim()


# ---- geometry --------------------------------------------------------------------------------------------------------------------
#: what ``seg_geometry`` of csrc/mifwt_thresh.hip takes: rows of at most 2^30 elements, an inner row extent of at most 2^30, fewer
#: than 2^31 rows
ROW_LIMIT = 1 << 30
_ROWS_LIMIT = 1 << 31


#: how many rows :func:`_split_row` tries: the search is host work, a modulo per candidate.  Rows get shorter as their number grows and
#: the kernel does not mind, but a length whose smallest divisor from ``ceil(n / ROW_LIMIT)`` on lies beyond this (3 x a prime above
#: 2^30) is treated as having none and takes the composed route, whose temporaries are several times the tensor.
SPLIT_SEARCH = 1 << 16


def _split_row(n: int):
    """A dense row of ``n > ROW_LIMIT`` elements as ``(a, b)``: ``a`` rows of ``b <= ROW_LIMIT`` elements with the longest such ``b``
    (the smallest divisor ``a`` of ``n`` from ``ceil(n / ROW_LIMIT)`` on, up to SPLIT_SEARCH rows), or None where ``n`` has none."""
    a = -(-n // ROW_LIMIT)
    while a <= SPLIT_SEARCH:
        if n % a == 0:
            return a, n // a
        a += 1
    return None


def _kernel_takes(t: torch.Tensor, leads: Tuple[int, int]) -> bool:
    """Whether the kernels take ``t``.  Anything of at most ROW_LIMIT elements is inside their envelope in every form; beyond that it is
    what :func:`_form` says (a row that could not be cut back — a prime length, no free extent — is not)."""
    return t.numel() <= ROW_LIMIT or _form(tuple(t.shape), tuple(t.stride()), tuple(leads)) is not None


def _collapse(shape, stride, barriers):
    """``shape`` / ``stride`` as at most three extents with element strides, outermost first, the innermost with unit stride.  A
    ``barrier`` b says that a threshold indexes the first b axes: no extent merges axes from both of its sides, and the innermost
    extent lies behind every barrier.  A merged innermost extent of more than ROW_LIMIT elements (a dense tensor of several GiB) is cut
    back into rows the kernels take where an extent is free for them (:func:`_split_row`).  Returns (extents, strides, rows per
    threshold index for each barrier), or None where the tensor has no such form (it is then read from a contiguous copy)."""
    nd = len(shape)
    dims: list = []  # [size, stride, first axis]
    for ax in range(nd):
        if shape[ax] == 1:
            continue
        if dims and dims[-1][1] == shape[ax] * stride[ax] and not any(dims[-1][2] < b <= ax for b in barriers):
            dims[-1][0] *= shape[ax]
            dims[-1][1] = stride[ax]
        else:
            dims.append([shape[ax], stride[ax], ax])
    if not dims or any(dims[-1][2] < b for b in barriers):
        dims.append([1, 1, nd])
    if dims[-1][0] > ROW_LIMIT and dims[-1][1] == 1 and len(dims) < 3:
        # a merged row longer than the kernels take: cut back into `a` dense rows of `b` elements (behind every barrier, as the row was)
        cut = _split_row(dims[-1][0])
        if cut is not None:
            dims[-1:] = [[cut[0], cut[1], dims[-1][2]], [cut[1], 1, dims[-1][2]]]
    if (dims[-1][0] > 1 and dims[-1][1] != 1) or len(dims) > 3:
        return None
    ext = [1] * (3 - len(dims)) + [d[0] for d in dims]
    st = [0] * (3 - len(dims)) + [d[1] for d in dims[:-1]] + [1]
    rows_per = []
    for b in barriers:
        rp = 1
        for d in dims[:-1]:
            if d[2] >= b:
                rp *= d[0]
        rows_per.append(rp)
    return ext, st, rows_per


@functools.lru_cache(maxsize=1024)
def _form(shape: Tuple[int, ...], stride: Tuple[int, ...], leads: Tuple[int, int]):
    """The collapsed form of a tensor of ``shape`` / ``stride`` for thresholds that index ``leads`` leading axes (0: one value): (whether
    it is read from a contiguous copy, extents, strides, rows per threshold index (0: one value) for each of the two thresholds) — or
    None where that form is outside the kernels' envelope (ROW_LIMIT, _ROWS_LIMIT).  Pure and cached: the one place that decides both."""
    barriers = sorted({b for b in leads if b > 0})
    g, copy = _collapse(shape, stride, barriers), False
    if g is None:
        dense, run = [], 1
        for n in reversed(shape):
            dense.insert(0, run)
            run *= n
        g, copy = _collapse(shape, tuple(dense), barriers), True
    ext, st, rp = g
    if ext[2] > ROW_LIMIT or ext[1] > ROW_LIMIT or ext[0] * ext[1] >= _ROWS_LIMIT:
        return None
    rows = dict(zip(barriers, rp))
    return copy, tuple(ext), tuple(st), tuple(rows[b] if b > 0 else 0 for b in leads)


def _geometry(t: torch.Tensor, leads: Tuple[int, int]):
    """:func:`_form` of ``t`` with the tensor to read in front — ``t`` or a contiguous copy —, or None outside the envelope."""
    form = _form(tuple(t.shape), tuple(t.stride()), tuple(leads))
    if form is None:
        return None
    return (t.contiguous() if form[0] else t, *form[1:])


def _dense_strides(ext):
    return [ext[1] * ext[2], ext[2], 1]


def _distinct(t: torch.Tensor) -> bool:
    """Whether the elements of ``t`` are distinct memory locations (what an output may mirror)."""
    reach = 1
    for s, n in sorted((s, n) for n, s in zip(t.shape, t.stride()) if n > 1):
        if s < reach:
            return False
        reach += s * (n - 1)
    return True


def _alloc_ops(srcs: Sequence[torch.Tensor]) -> list:
    """How to allocate fresh outputs for ``srcs``: ("dense", i) or ("mirror", [i..], elements of the buffer, [(shape, stride, offset)..]).
    Tensors that are views of one buffer (the bands of a level) get views of ONE new buffer with the same offsets and strides, so every
    output row is misaligned exactly as its input row — the kernel's 16-byte path needs that — and the next transform finds the layout
    it wrote itself.  A view that covers little of its buffer, or whose elements overlap, gets a dense tensor."""
    ops: list = []
    groups: dict = {}
    for i, t in enumerate(srcs):
        if t.is_contiguous():
            ops.append(("dense", i))
        else:
            groups.setdefault(t.untyped_storage().data_ptr(), []).append(i)
    for idx in groups.values():
        t0 = srcs[idx[0]]
        elems = t0.untyped_storage().nbytes() // t0.element_size()
        covered = sum(srcs[i].numel() for i in idx)
        offsets = {srcs[i].storage_offset() for i in idx}
        if 2 * covered >= elems and len(offsets) == len(idx) and all(_distinct(srcs[i]) for i in idx):
            ops.append(("mirror", idx, elems, [(srcs[i].shape, srcs[i].stride(), srcs[i].storage_offset()) for i in idx]))
        else:
            ops.extend(("dense", i) for i in idx)
    return ops


def _alloc_run(ops, srcs: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    outs: List[Optional[torch.Tensor]] = [None] * len(srcs)
    dtype, device = srcs[0].dtype, srcs[0].device
    for op in ops:
        if op[0] == "dense":
            outs[op[1]] = torch.empty(srcs[op[1]].shape, dtype=dtype, device=device)
        else:
            base = torch.empty(op[2], dtype=dtype, device=device)
            off = base.storage_offset()
            for i, (shape, stride, offset) in zip(op[1], op[3]):
                outs[i] = base.as_strided(shape, stride, off + offset)
    return outs  # type: ignore[return-value]


class _Plan:
    """What one launch needs that depends on geometry alone: the descriptor table as bytes (pointers and values blank), its array type,
    the number of units (the backward's workspace) and of elements."""

    __slots__ = ("arr_t", "template", "units", "numel", "c0", "n")

    def __init__(self, dt: int, is_complex: bool, table, c0: int):
        n = len(table)
        self.c0, self.n = c0, n
        self.arr_t = Seg * n
        arr = self.arr_t()
        self.numel = 0
        for s, (ext, xs, ys, gs, rp, on_dev) in zip(arr, table):
            s.extent[:] = ext
            s.x_stride[:] = xs
            s.y_stride[:] = ys
            s.g_stride[:] = gs
            s.rows_per_value[:] = rp
            for k in range(2):
                s.dvalue[k] = 1 if on_dev[k] else None  # (a placeholder that says "device threshold" to mifwt_thresh_plan)
            self.numel += ext[0] * ext[1] * ext[2]
        units = _lib().mifwt_thresh_plan(dt, int(is_complex), arr, n, None)
        if units < 0:
            _engine._check(int(units))
        self.units = int(units)
        self.template = bytes(arr)


class _Recipe:
    """A call's host work that depends on geometry alone (shapes, strides, offsets, which tensors share a buffer, the thresholds' forms):
    which tensors are read from contiguous copies, how the outputs are allocated, the descriptor tables of its launches."""

    __slots__ = ("copy_x", "copy_g", "ops", "plans")


def _signature(xs, los, his, gs):
    """The cache key of a call's recipe."""
    buffers: dict = {}
    sig = []
    for i, x in enumerate(xs):
        lo, hi = los[i], his[i] if his is not None else 0.0
        place = None if x.is_contiguous() else (x.storage_offset(), buffers.setdefault(x.untyped_storage().data_ptr(), len(buffers)),
                                                x.untyped_storage().nbytes())
        sig.append((x.shape, x.stride(), place, None if gs is None else gs[i].stride(),
                    lo.shape if isinstance(lo, torch.Tensor) else None, hi.shape if isinstance(hi, torch.Tensor) else None))
    return (xs[0].dtype, his is None, tuple(sig))


def _build_recipe(xs, los, his, gs) -> _Recipe:
    dtype = xs[0].dtype
    is_complex = dtype in _COMPLEX
    dt = _engine._DTYPE_IDS[_COMPLEX.get(dtype, dtype)]
    cap = max_segments()
    r = _Recipe()
    r.copy_x, r.copy_g = [], []
    reads, geos = [], []
    for i, x in enumerate(xs):
        xr, ext, st, rp = _geometry(x, (_lead(los[i], x), _lead(his[i], x) if his is not None else 0))
        if xr is not x:
            r.copy_x.append(i)
        reads.append(xr)
        geos.append((ext, st, rp))
    r.ops = _alloc_ops(reads)
    outs = _alloc_run(r.ops, reads)
    r.plans = []
    for c0 in range(0, len(xs), cap):
        table = []
        for i in range(c0, min(c0 + cap, len(xs))):
            ext, st, rp = geos[i]
            ys = _dense_strides(ext) if outs[i].is_contiguous() else st  # (an output is dense or mirrors its input)
            gst = [0, 0, 1]
            if gs is not None:
                g = gs[i]
                gst = _dense_strides(ext)
                if not g.is_contiguous():
                    leads = (_lead(los[i], g), _lead(his[i], g) if his is not None else 0)
                    cg = _collapse(tuple(g.shape), tuple(g.stride()), sorted({b for b in leads if b > 0}))
                    if cg is not None and tuple(cg[0]) == tuple(ext):
                        gst = cg[1]
                    else:
                        r.copy_g.append(i)
            on_dev = (isinstance(los[i], torch.Tensor), his is not None and isinstance(his[i], torch.Tensor))
            table.append((tuple(ext), tuple(st), tuple(ys), tuple(gst), tuple(rp), on_dev))
        r.plans.append(_Plan(dt, is_complex, table, c0))
    return r


# ---- the two launches (no autograd) -----------------------------------------------------------------------------------------------
def _dev64(v: torch.Tensor) -> torch.Tensor:
    """A threshold tensor as the kernels read it: float64, contiguous, flat (a device-side cast, asynchronous, as ``_engine.DevTaps``)."""
    v = v.detach().reshape(-1)
    if v.dtype != torch.float64 or not v.is_contiguous():
        v = v.to(torch.float64).contiguous()
    return v


def _launches(xs: Sequence[torch.Tensor], los, his, mode: int, sub: float, gs: Optional[Sequence[torch.Tensor]] = None,
              want: Optional[dict] = None) -> List[torch.Tensor]:
    """Forward (``gs`` None) or backward of the tensors ``xs`` (non-empty, one dtype, one device) with the thresholds ``los`` / ``his``
    (per tensor a float or a tensor; ``his`` None outside firm): ``ceil(len(xs) / max_segments())`` launches.  Returns the outputs; the
    backward appends to ``want[id(v)]``, for every threshold tensor ``v`` named there, the float64 sums of ``g dT/dv`` of each launch."""
    dtype = xs[0].dtype
    is_complex = dtype in _COMPLEX
    dt = _engine._DTYPE_IDS[_COMPLEX.get(dtype, dtype)]
    arith = _arith(dtype)
    bwd = gs is not None
    recipe = _engine._plan(_signature(xs, los, his, gs), lambda: _build_recipe(xs, los, his, gs), _plans)
    reads = xs
    if recipe.copy_x:
        reads = list(xs)
        for i in recipe.copy_x:
            reads[i] = xs[i].contiguous()
    if bwd and recipe.copy_g:
        gs = list(gs)
        for i in recipe.copy_g:
            gs[i] = gs[i].contiguous()
    outs = _alloc_run(recipe.ops, reads)
    dev_cache: dict = {}
    for plan in recipe.plans:
        arr = plan.arr_t.from_buffer_copy(plan.template)  # (per call: a cached plan never owns an array that a call writes)
        dests: dict = {}
        for j, s in enumerate(arr):
            i = plan.c0 + j
            s.x = reads[i].data_ptr()
            s.y = outs[i].data_ptr()
            if bwd:
                s.g = gs[i].data_ptr()
            for k, v in enumerate((los[i], his[i] if his is not None else 0.0)):
                if isinstance(v, torch.Tensor):
                    d64 = dev_cache.get(id(v))
                    if d64 is None:
                        d64 = dev_cache[id(v)] = _dev64(v)
                    s.dvalue[k] = d64.data_ptr()
                    if bwd and mode in _HAS_VGRAD and id(v) in want:
                        d = dests.get(id(v))
                        if d is None:
                            d = dests[id(v)] = torch.empty(v.numel(), dtype=torch.float64, device=v.device)
                        s.gvalue[k] = d.data_ptr()
                elif v != 0.0:
                    s.value[k] = _round(v, arith)
        if bwd:
            _engine._run("thresh_bwd", KID_BWD, (plan.numel,), reads[plan.c0], _lib().mifwt_thresh_bwd, (dt, mode, arr, plan.n),
                         ws_bytes=16 * plan.units if dests else 0)
            for vid, d in dests.items():
                want[vid].append(d)
        else:
            _engine._run("thresh_fwd", KID_FWD, (plan.numel,), reads[plan.c0], _lib().mifwt_thresh_fwd,
                         (dt, int(is_complex), mode, sub, arr, plan.n))
    return outs


# ---- the composed route: torch operations, the same closed forms -------------------------------------------------------------------
def _bcast(v, t: torch.Tensor, arith: torch.dtype):
    if not isinstance(v, torch.Tensor):
        return torch.tensor(_round(v, arith), dtype=arith, device=t.device)
    v = v.to(arith)
    return v.reshape(()) if v.numel() == 1 else v.reshape(tuple(v.shape) + (1,) * (t.dim() - v.dim()))


def _composed(x: torch.Tensor, lo, hi, mode: int, sub: float) -> torch.Tensor:
    """``T(x)`` from torch operations, in the arithmetic type of ``x``, differentiable to any order w.r.t. ``x`` and tensor thresholds:
    the route of calls whose backward is recorded itself and of complex data that requires grad, and the emulation the benchmark
    (tools/thresh_bench.py) compares the kernels with.  Real ``soft`` is the usual ``sign(x) * relu(|x| - v)``."""
    arith = _arith(x.dtype)
    xa = x if x.dtype in (torch.float32, torch.float64) or x.is_complex() else x.to(arith)
    v = _bcast(lo, x, arith)
    m = xa.abs()
    zero = torch.zeros((), dtype=xa.dtype, device=x.device)
    subs = torch.full((), sub, dtype=xa.dtype, device=x.device)
    if mode == 0:
        if xa.is_complex():
            y = torch.where(m > v, xa * (1 - v / torch.where(m > v, m, torch.ones_like(m))), zero)
        else:
            y = torch.sign(xa) * torch.relu(m - v)
        if sub != 0.0:
            y = torch.where(m < v, subs, y)
    elif mode == 1:
        y = torch.where(m >= v, xa, subs)
    elif mode == 2:
        ms = torch.where(m > v, m, torch.ones_like(m))
        y = torch.where(m > v, xa * (1 - (v * v) / (ms * ms)), zero)
        if sub != 0.0:
            y = torch.where(m < v, subs, y)
    elif mode == 3:
        y = torch.where(xa >= v, xa, subs)
    elif mode == 4:
        y = torch.where(xa <= v, xa, subs)
    else:
        h = _bcast(hi, x, arith)
        mid = (m > v) & (m <= h)
        ms = torch.where(mid, m, torch.ones_like(m))
        d = torch.where(h > v, h - v, torch.ones_like(h))
        y = torch.where(m > h, xa, torch.where(mid, xa * (h * (1 - v / ms) / d), zero))
    return y if y.dtype == x.dtype else y.to(x.dtype)


# ---- autograd ----------------------------------------------------------------------------------------------------------------------
class _Thresh(torch.autograd.Function):
    """The tensors of a call as one differentiable node: ``cfg`` = (mode, substitute, per tensor the low and the high threshold as a
    float or an index into the threshold tensors, number of data tensors), then the data tensors, then the threshold tensors."""

    @staticmethod
    def forward(ctx, cfg, *tensors):
        mode, sub, lo_spec, hi_spec, nx = cfg
        xs, vs = tensors[:nx], tensors[nx:]
        los = [vs[s] if isinstance(s, int) else s for s in lo_spec]
        his = None if hi_spec is None else [vs[s] if isinstance(s, int) else s for s in hi_spec]
        ctx.cfg = cfg
        ctx.save_for_backward(*tensors)  # (the input itself: no mask is kept)
        return tuple(_launches(xs, los, his, mode, sub))

    @staticmethod
    def backward(ctx, *gouts):
        mode, sub, lo_spec, hi_spec, nx = ctx.cfg
        tensors = ctx.saved_tensors
        xs, vs = tensors[:nx], tensors[nx:]
        los = [vs[s] if isinstance(s, int) else s for s in lo_spec]
        his = None if hi_spec is None else [vs[s] if isinstance(s, int) else s for s in hi_spec]
        live = [i for i, g in enumerate(gouts) if g is not None]
        grads: List[Optional[torch.Tensor]] = [None] * len(tensors)
        if not live:
            return (None, *grads)
        if torch.is_grad_enabled():
            # the backward itself is being recorded: the composed route, differentiated by autograd
            with torch.enable_grad():
                ys = [_composed(xs[i], los[i], None if his is None else his[i], mode, sub) for i in live]
                need = [j for j, t in enumerate(tensors) if t.requires_grad and ctx.needs_input_grad[j + 1]]
                got = torch.autograd.grad(ys, [tensors[j] for j in need], [gouts[i] for i in live], create_graph=True, allow_unused=True)
            for j, g in zip(need, got):
                grads[j] = g
            return (None, *grads)
        want = {id(v): [] for j, v in enumerate(vs) if ctx.needs_input_grad[1 + nx + j]}
        gx = _launches([xs[i] for i in live], [los[i] for i in live], None if his is None else [his[i] for i in live], mode, sub,
                       gs=[gouts[i] for i in live], want=want)
        for i, g in zip(live, gx):
            if ctx.needs_input_grad[1 + i]:
                grads[i] = g
        for j, v in enumerate(vs):
            parts = want.get(id(v))
            if parts is None:
                continue
            if not parts:  # (hard / greater / less, or a threshold none of the live tensors uses)
                grads[nx + j] = torch.zeros_like(v)
                continue
            total = parts[0] if len(parts) == 1 else torch.stack(parts).sum(0)
            grads[nx + j] = total.to(device=v.device, dtype=v.dtype).reshape(v.shape)  # (cast like the threshold, as _fwt._like does for taps)
        return (None, *grads)


# ---- the public functions ------------------------------------------------------------------------------------------------------------
def _apply(data, lo, hi, mode: int, sub: float):
    is_container = not isinstance(data, torch.Tensor)
    leaves, owner, nentries = _flatten(data)
    los_e = _per_entry("value" if hi is None else "value_low", lo, is_container, nentries)
    his_e = None if hi is None else _per_entry("value_high", hi, is_container, nentries)
    by_entry: List[List[torch.Tensor]] = [[] for _ in range(nentries)]
    for t, e in zip(leaves, owner):
        by_entry[e].append(t)
    for e in range(nentries):
        if los_e[e] is None or (his_e is not None and his_e[e] is None):
            if his_e is not None and (los_e[e] is None) != (his_e[e] is None):
                raise ValueError("threshold_firm: value_low and value_high must be None for the same container entries")
            continue
        los_e[e] = _check_value("value" if hi is None else "value_low", los_e[e], by_entry[e])
        if his_e is not None:
            his_e[e] = _check_value("value_high", his_e[e], by_entry[e])
            if not isinstance(los_e[e], torch.Tensor) and not isinstance(his_e[e], torch.Tensor) and his_e[e] < los_e[e]:
                raise ValueError(f"threshold_firm: value_high must not be below value_low, got {his_e[e]} < {los_e[e]}")
    allowed = supported_dtypes() | set(_COMPLEX)
    for t in leaves:
        if t.dtype not in allowed:
            raise ValueError(f"Input dtype {t.dtype} not supported")
        if t.is_complex() and mode in (3, 4):
            raise ValueError("threshold: modes 'greater' and 'less' are defined for real data only")
    for t in leaves:
        _engine._require_gpu(t)
    # the tensors that run: not spared by a None entry, not empty; a tensor beyond the kernels' envelope whose rows cannot be cut back
    # into it (module docstring) is composed here and now; the others are grouped by (dtype, device), a launch sequence each
    outs: List[Optional[torch.Tensor]] = list(leaves)
    work: dict = {}
    for i, (t, e) in enumerate(zip(leaves, owner)):
        if los_e[e] is None:
            continue
        if t.numel() == 0:
            outs[i] = torch.empty(t.shape, dtype=t.dtype, device=t.device)
            continue
        lo_t, hi_t = los_e[e], None if his_e is None else his_e[e]
        if not _kernel_takes(t, (_lead(lo_t, t), _lead(hi_t, t) if his_e is not None else 0)):
            outs[i] = _composed(t, lo_t, hi_t, mode, sub)
            continue
        work.setdefault((t.dtype, t.device), []).append(i)
    for (dtype, _), idx in work.items():
        xs = [leaves[i] for i in idx]
        los = [los_e[owner[i]] for i in idx]
        his = None if his_e is None else [his_e[owner[i]] for i in idx]
        vts: List[torch.Tensor] = []
        for v in los + (his or []):
            if isinstance(v, torch.Tensor) and not any(v is u for u in vts):
                vts.append(v)
        grad = torch.is_grad_enabled() and (any(x.requires_grad for x in xs) or any(v.requires_grad for v in vts))
        if not grad:
            ys = _launches(xs, los, his, mode, sub)
        elif dtype in _COMPLEX:
            ys = [_composed(x, los[j], None if his is None else his[j], mode, sub) for j, x in enumerate(xs)]
        else:
            def spec(vals):
                return tuple(next(k for k, u in enumerate(vts) if u is v) if isinstance(v, torch.Tensor) else v for v in vals)

            cfg = (mode, sub, spec(los), None if his is None else spec(his), len(xs))
            ys = _Thresh.apply(cfg, *xs, *vts)
        for i, y in zip(idx, ys):
            outs[i] = y
    return _rebuild(data, iter(outs))


def threshold(data, value, mode: str = "soft", substitute: float = 0.0):
    """``pywt.threshold`` on a tensor or a coefficient container (module docstring): ``mode`` is ``"soft"``, ``"hard"``, ``"garrote"``,
    ``"greater"`` or ``"less"``; ``value`` a number, a one-element or leading-form tensor, or — for a container — a sequence of those
    and ``None`` with one entry per container entry.  Returns the same container type with the same keys, order and named-tuple types
    over fresh tensors (entries spared by ``None`` keep their objects).  ``x = 0`` gives 0 also at ``value = 0``: numpy's ``0 / 0`` NaN is
    deliberately not reproduced.

    ``ValueError`` for an unknown mode, a negative number threshold, a tensor threshold of another shape, a sequence of the wrong length,
    ``greater`` / ``less`` on complex data, float16 / bfloat16 outside ``half_storage()``; ``RuntimeError`` for a CPU tensor."""
    if mode not in MODES:
        raise ValueError(f"threshold: unknown mode {mode!r}; the modes are {', '.join(MODES)}")
    return _apply(data, value, None, MODES[mode], float(substitute))


def threshold_firm(data, value_low, value_high):
    """``pywt.threshold_firm`` on a tensor or a coefficient container: 0 up to ``value_low``, the identity above ``value_high``, the
    straight line ``x v_hi (1 - v_lo / |x|) / (v_hi - v_lo)`` between; ``value_high == value_low`` is hard thresholding there (nothing is
    divided).  Thresholds and containers as for :func:`threshold`; ``ValueError`` for numbers with ``value_high < value_low``."""
    return _apply(data, value_low, value_high, FIRM, 0.0)
