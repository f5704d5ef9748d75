"""Host path of the VALUE-MAP extension levels (``mode="smooth" | "antisymmetric" | "antireflect"``; C ABI ``mifwt_ext_*``,
include/mifwt.h; kernels csrc/mifwt_ext.hip).

Two maps, taps as host floats in PyWavelets order, ``M = floor((n + L - 1) / 2)`` per axis,

    level_fwd(x, dec_lo, dec_hi, mode)           x [B, n..]               -> buffer [B, 2^d, M..]
    level_adj(g, dec_lo, dec_hi, mode, extent)   g [B, 2^d, M..]          -> g_x [B, n..]          the transpose of level_fwd

each ONE fused launch (kernel ids 42 / 43) for one or two transformed axes, float32 / float64, even ``L <= 20`` and unit innermost
strides.  Everything else runs the axis passes (ids 44 / 45), one launch per axis and plane as in ``_per``: longer filters, permuted
axes.  Three transformed axes: the fused 2-D launch over the last two axes with depth folded into the batch plus ONE axis pass along
depth, in both maps.  A call allocates its outputs and enqueues launches, nothing else: no host round trip, capturable.

The inverse of a level is the padded synthesis, which has no mode (``_fwt.synthesis``).  The two autograd Functions call each other —
the adjoint is linear and its backward is the level again — so data gradients of any order exist.
"""
from __future__ import annotations

import ctypes
from typing import Sequence, Set, Tuple

import numpy as np
import torch

from . import _engine

KID_FWD, KID_ADJ, KID_AXIS_FWD, KID_AXIS_ADJ = 42, 43, 44, 45
#: ``ext_mode`` of the C ABI (MIFWT_EXT_*)
MODES = {"smooth": 0, "antisymmetric": 1, "antireflect": 2}

# Tests and tools/ext_bench.py set this to run a level through the axis passes although the fused kernels would take it.
FORCE_AXIS = False
# (direction, dtype, L, ndim) cells of the fused envelope that go to the axis passes all the same (direction 0 analysis, 1 adjoint): a
# cell belongs here only where `tools/ext_bench.py` has shown the fused median behind the axis one by more than the spread of its
# windows.  Empty: nothing has been measured to lose.
AXIS_PASS_CELLS: Set[Tuple[int, torch.dtype, int, int]] = set()

_entries = None


def _lib():
    """The entry points of these levels (``_engine.EXT_ENTRIES``), bound on first use."""
    global _entries
    if _entries is None:
        _entries = _engine.private_entries(_engine.EXT_ENTRIES)
    return _entries


_desc, _unit_last = _engine._desc, _engine._unit_last
_plans: dict = {}
_engine._routing_caches.append(_plans)


def _launch(direction: int, kid: int, extent, anchor: torch.Tensor, entry, *args) -> None:
    _engine._run(("ext_fwd", "ext_adj")[direction], kid, extent, anchor, entry, args)


def _route(direction: int, key, mode: int, dtype: torch.dtype, flen: int, ndim: int, desc):
    """(reference to the level descriptor, whether the fused kernel takes the level); the descriptor ``desc()`` builds and the
    library's answer (``mifwt_ext_supported``) are cached under ``key``, which names EVERYTHING the descriptor holds: the direction,
    the caller's number of axes, extents and every stride set, signal and band side."""
    def build():
        d = desc()
        ok = _lib().mifwt_ext_supported(ctypes.byref(d), mode, direction)
        if ok < 0:
            _engine._check(ok)
        return d, ctypes.byref(d), bool(ok)

    _, ref, fused = _engine._plan(key, build, _plans)
    return ref, fused and not FORCE_AXIS and (direction, dtype, flen, ndim) not in AXIS_PASS_CELLS


def _setup(t: torch.Tensor, ndim: int) -> int:
    """The refusals of every level, and the dtype id of the axis passes."""
    _engine._require_gpu(t)
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"Input dtype {t.dtype} not supported by the smooth / antisymmetric / antireflect transforms (float32 / float64)")
    if not 1 <= ndim <= 3:
        raise NotImplementedError("smooth / antisymmetric / antireflect levels exist for one, two and three transformed axes")
    return _engine._DTYPE_IDS[t.dtype]


def _mode(mode) -> int:
    return MODES[mode] if isinstance(mode, str) else int(mode)


def _axis_strides(t: torch.Tensor):
    return _engine._arr(ctypes.c_int64, 3)(*t.stride())


def _oai(t: torch.Tensor, axis: int) -> torch.Tensor:
    """A [B, d0(, d1(, d2))] tensor as the [outer, n, inner] view whose middle axis is ``axis`` (1 .. 3)."""
    return t.reshape(int(np.prod(t.shape[:axis])), t.shape[axis], int(np.prod(t.shape[axis + 1:])))


def _axis_fwd(src, o_lo, o_hi, mode: int, dt: int, flen: int, lo, hi) -> None:
    """One analysis axis launch over [outer, n, inner] -> [outer, m, inner] views."""
    outer, n, inner = src.shape
    _launch(0, KID_AXIS_FWD, (n,), src, _lib().mifwt_ext_axis_fwd, mode, dt, flen, outer, n, inner, src.data_ptr(), _axis_strides(src),
            o_lo.data_ptr(), _axis_strides(o_lo), o_hi.data_ptr(), _axis_strides(o_hi), lo, hi)


def _axis_adj(g_lo, g_hi, dst, mode: int, dt: int, flen: int, lo, hi) -> None:
    """One adjoint axis launch over [outer, m, inner] -> [outer, n, inner] views."""
    outer, n, inner = dst.shape
    _launch(1, KID_AXIS_ADJ, (n,), g_lo, _lib().mifwt_ext_axis_adj, mode, dt, flen, outer, n, inner, g_lo.data_ptr(), _axis_strides(g_lo),
            g_hi.data_ptr(), _axis_strides(g_hi), dst.data_ptr(), _axis_strides(dst), lo, hi)


# ---- the two level maps (no autograd) ---------------------------------------------------------------------------------------------
def _fused_fwd(x: torch.Tensor, planes: Sequence[torch.Tensor], ref, mode: int, lo, hi) -> None:
    _launch(0, KID_FWD, tuple(x.shape[1:]), x, _lib().mifwt_ext_fwd, ref, mode, x.data_ptr(), planes[0].data_ptr(),
            _engine._ptr_array(planes[1:]), lo, hi)


def _fused_adj(planes: Sequence[torch.Tensor], y: torch.Tensor, ref, mode: int, lo, hi) -> None:
    _launch(1, KID_ADJ, tuple(y.shape[1:]), y, _lib().mifwt_ext_adj, ref, mode, planes[0].data_ptr(), _engine._ptr_array(planes[1:]),
            y.data_ptr(), lo, hi)


def level_fwd(x: torch.Tensor, dec_lo: Sequence[float], dec_hi: Sequence[float], mode) -> torch.Tensor:
    """x [B, n0(, n1(, n2))] -> buffer [B, 2^d, M0(, M1(, M2))], plane s = band s (bit (d-1-a) of s set <=> high-pass along axis a).
    (Three axes: the buffer is a view whose planes are dense tensors of their own.)"""
    ndim = x.dim() - 1
    dt = _setup(x, ndim)
    mode = _mode(mode)
    flen = len(dec_lo)
    sig = [int(n) for n in x.shape[1:]]
    coef = [(n + flen - 1) // 2 for n in sig]
    b = int(x.shape[0])
    lo, hi = _engine._taps_array(dec_lo), _engine._taps_array(dec_hi)
    if ndim == 3:
        xc = _unit_last(x)
        x2 = xc.reshape(b * sig[0], sig[1], sig[2])  # (a view of a dense volume)
        tmp = torch.empty((4, b * sig[0], coef[1], coef[2]), dtype=x.dtype, device=x.device)
        st = tmp.stride()[1:]
        ref, fused = _route(0, (0, 3, mode, x2.shape, x2.stride(), tuple(st), x.dtype, flen), mode, x.dtype, flen, 3,
                            lambda: _desc(2, x.dtype, 0, flen, b * sig[0], sig[1:], x2.stride(), coef[1:], st, st))
        if fused:
            out = torch.empty((8, b, *coef), dtype=x.dtype, device=x.device)
            if out.numel():
                _fused_fwd(x2, list(tmp.unbind(0)), ref, mode, lo, hi)
                plane = coef[1] * coef[2]
                _axis_fwd(tmp.view(4 * b, sig[0], plane), out[:4].view(4 * b, coef[0], plane), out[4:].view(4 * b, coef[0], plane),
                          mode, dt, flen, lo, hi)
            return out.transpose(0, 1)
        x = xc
    else:
        buf = torch.empty((b, 1 << ndim, *coef), dtype=x.dtype, device=x.device)
        if buf.numel() == 0:
            return buf
        st = [buf.stride(0), *buf.stride()[2:]]
        ref, fused = _route(0, (0, ndim, mode, x.shape, x.stride(), tuple(st), x.dtype, flen), mode, x.dtype, flen, ndim,
                            lambda: _desc(ndim, x.dtype, 0, flen, b, sig, x.stride(), coef, st, st))
        if fused:
            _fused_fwd(x, list(buf.unbind(1)), ref, mode, lo, hi)
            return buf
    # One pass per axis, last axis first: 1 (+ 2 (+ 4)) launches.  Stage k holds 2^k planes; the pass over plane p writes its low band to
    # plane p and its high band to plane p + 2^k; the planes of the last stage are the bands of `buf`.
    if ndim == 3:
        buf = torch.empty((b, 8, *coef), dtype=x.dtype, device=x.device)
        if buf.numel() == 0:
            return buf
    cur = [x]  # (a plane that is no [outer, n, inner] view as it stands — permuted axes — is copied by the reshape of its pass)
    for axis in range(ndim, 0, -1):
        npl = len(cur)
        if axis == 1:
            out = [buf[:, s] for s in range(2 * npl)]
        else:
            out = torch.empty((2 * npl, b, *sig[:axis - 1], *coef[axis - 1:]), dtype=x.dtype, device=x.device)
        for pl in range(npl):
            _axis_fwd(_oai(cur[pl], axis), _oai(out[pl], axis), _oai(out[npl + pl], axis), mode, dt, flen, lo, hi)
        cur = out
    return buf


def level_adj(g: torch.Tensor, dec_lo: Sequence[float], dec_hi: Sequence[float], mode, extent: Sequence[int]) -> torch.Tensor:
    """g [B, 2^d, M0(, M1(, M2))] (band order as above) -> g_x [B, n0(, n1(, n2))]: the transpose of :func:`level_fwd` at ``extent``."""
    ndim = g.dim() - 2
    dt = _setup(g, ndim)
    mode = _mode(mode)
    flen = len(dec_lo)
    sig = [int(n) for n in extent]
    coef = [(n + flen - 1) // 2 for n in sig]
    b = int(g.shape[0])
    if len(sig) != ndim or tuple(g.shape[1:]) != (1 << ndim, *coef):
        raise ValueError(f"a level of extent {tuple(sig)} and {flen} taps has no coefficient buffer of shape {tuple(g.shape)}")
    lo, hi = _engine._taps_array(dec_lo), _engine._taps_array(dec_hi)
    y = torch.empty((b, *sig), dtype=g.dtype, device=g.device)
    if y.numel() == 0:
        return y
    if ndim == 3:
        tmp = torch.empty((4, b * sig[0], coef[1], coef[2]), dtype=g.dtype, device=g.device)
        st = tmp.stride()[1:]
        y2 = y.view(b * sig[0], sig[1], sig[2])
        ref, fused = _route(1, (1, 3, mode, y2.shape, y2.stride(), tuple(coef), tuple(st), g.dtype, flen), mode, g.dtype, flen, 3,
                            lambda: _desc(2, g.dtype, 0, flen, b * sig[0], sig[1:], y2.stride(), coef[1:], st, st))
        if fused:
            gt = g.transpose(0, 1).contiguous()  # [8, B, M0, M1, M2]
            plane = coef[1] * coef[2]
            _axis_adj(gt[:4].view(4 * b, coef[0], plane), gt[4:].view(4 * b, coef[0], plane), tmp.view(4 * b, sig[0], plane), mode, dt, flen,
                      lo, hi)
            _fused_adj(list(tmp.unbind(0)), y2, ref, mode, lo, hi)
            return y
    else:
        gu = _unit_last(g)
        st = [gu.stride(0), *gu.stride()[2:]]
        ref, fused = _route(1, (1, ndim, mode, gu.shape, tuple(sig), y.stride(), tuple(st), g.dtype, flen), mode, g.dtype, flen, ndim,
                            lambda: _desc(ndim, g.dtype, 0, flen, b, sig, y.stride(), coef, st, st))
        if fused:
            _fused_adj(list(gu.unbind(1)), y, ref, mode, lo, hi)
            return y
    # The mirror of the analysis passes, first axis first: (4 +) (2 +) 1 launches.  The pass that leaves 2^k planes takes the low band
    # from plane p and the high band from plane p + 2^k; the last one writes `y`.
    cur = list(g.unbind(1))
    for axis in range(1, ndim + 1):
        npl = len(cur) // 2
        out = [y] if axis == ndim else torch.empty((npl, b, *sig[:axis], *coef[axis:]), dtype=g.dtype, device=g.device)
        for pl in range(npl):
            _axis_adj(_oai(cur[pl], axis), _oai(cur[npl + pl], axis), _oai(out[pl], axis), mode, dt, flen, lo, hi)
        cur = out
    return y


# ---- autograd: the level's backward is its adjoint, the adjoint's backward the level ------------------------------------------------------
class _Fwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dec_lo, dec_hi, mode):
        ctx.meta = (dec_lo, dec_hi, mode, tuple(x.shape[1:]))
        return level_fwd(x, dec_lo, dec_hi, mode)

    @staticmethod
    def backward(ctx, g):
        dec_lo, dec_hi, mode, sig = ctx.meta
        return _Adj.apply(g, dec_lo, dec_hi, mode, sig), None, None, None


class _Adj(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, dec_lo, dec_hi, mode, extent):
        ctx.meta = (dec_lo, dec_hi, mode)
        return level_adj(g, dec_lo, dec_hi, mode, extent)

    @staticmethod
    def backward(ctx, g_y):
        dec_lo, dec_hi, mode = ctx.meta
        return _Fwd.apply(g_y, dec_lo, dec_hi, mode), None, None, None, None


def fwd(x: torch.Tensor, dec_lo, dec_hi, mode) -> torch.Tensor:
    if torch.is_grad_enabled() and x.requires_grad:
        return _Fwd.apply(x, tuple(dec_lo), tuple(dec_hi), _mode(mode))
    return level_fwd(x, dec_lo, dec_hi, mode)


def adj(g: torch.Tensor, dec_lo, dec_hi, mode, extent: Sequence[int]) -> torch.Tensor:
    if torch.is_grad_enabled() and g.requires_grad:
        return _Adj.apply(g, tuple(dec_lo), tuple(dec_hi), _mode(mode), tuple(int(n) for n in extent))
    return level_adj(g, dec_lo, dec_hi, mode, extent)
