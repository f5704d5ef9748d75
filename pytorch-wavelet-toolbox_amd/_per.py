"""Host path of the PERIODIZED levels (``mode="periodization"``; C ABI ``mifwt_per_*``, include/mifwt.h; kernels csrc/mifwt_per.hip).

Two level maps, taps as host floats in PyWavelets order,

    level_fwd(x, dec_lo, dec_hi)                 x [B, n..]              -> buffer [B, 2^d, M..]     M = ceil(n / 2)
    level_inv(bands, rec_lo, rec_hi, out_extent) bands [B, M..] each     -> y [B, n..]               n in {2 M, 2 M - 1}

each ONE fused launch (kernel ids 38 / 39) for one or two transformed axes, float32 / float64, even ``L <= 20`` and unit innermost
strides.  Everything else runs the axis passes (ids 40 / 41), one launch per axis and plane as in ``_bwt``: longer filters, permuted
axes.  Three transformed axes: the fused 2-D launch over the last two axes with depth folded into the batch plus the axis pass along
depth — analysis two launches (the planes are laid out so that ONE axis launch takes the four of them), synthesis four axis launches
(one per pair of bands, which arrive as separate tensors) and the fused one.  A call allocates its outputs and enqueues launches,
nothing else: no host round trip, capturable.  On an axis shorter than the filter the taps that meet the same sample are summed on
the host, in double, before the launch (``_taps``).

Adjoints (include/mifwt.h): the transpose of an analysis level is the synthesis level with the reversed dec taps over the even extents,
after which the gradient of the virtual sample of an odd extent is added to its source, the last real sample; the transpose of a
synthesis level is the analysis level with the reversed rec taps (a cropped sample has gradient zero).  The two autograd Functions call
each other: data gradients of any order.
"""
from __future__ import annotations

import ctypes
import math
from typing import Sequence, Set, Tuple

import numpy as np
import torch

from . import _engine

KID_FWD, KID_INV, KID_AXIS_FWD, KID_AXIS_INV = 38, 39, 40, 41

# Tests and tools/per_bench.py set this to run a level through the axis passes although the fused kernel would take it.
FORCE_AXIS = False
# (direction, dtype, L, ndim) cells of the fused envelope that go to the axis passes all the same (direction 0 analysis, 1 synthesis): a
# cell belongs here only where `tools/per_bench.py` has shown the fused median behind the axis one by more than the spread of its
# windows.  Empty: nothing has been measured to lose.
AXIS_PASS_CELLS: Set[Tuple[int, torch.dtype, int, int]] = set()

_entries = None


def _lib():
    """The periodized entry points (``_engine.PER_ENTRIES``), bound on first use."""
    global _entries
    if _entries is None:
        _entries = _engine.private_entries(_engine.PER_ENTRIES)
    return _entries


_desc, _unit_last = _engine._desc, _engine._unit_last
_plans: dict = {}
_engine._routing_caches.append(_plans)


def _launch(direction: int, kid: int, extent, anchor: torch.Tensor, entry, *args) -> None:
    _engine._run(("per_fwd", "per_inv")[direction], kid, extent, anchor, entry, args)


def _route(direction: int, key, dtype: torch.dtype, flen: int, ndim: int, desc):
    """(reference to the level descriptor, whether the fused kernel takes the level); the descriptor ``desc()`` builds and the
    library's answer (``mifwt_per_supported``) are cached under ``key``, which therefore names EVERYTHING the descriptor holds: the
    direction, the caller's number of axes, extents and every stride set, signal and band side (the planes of a 3-D level's inner
    2-D launch and the planes of a 2-D level buffer of the same extents have different strides)."""
    def build():
        d = desc()
        ok = _lib().mifwt_per_supported(ctypes.byref(d), direction)
        if ok < 0:
            _engine._check(ok)
        return d, ctypes.byref(d), bool(ok)

    _, ref, fused = _engine._plan(key, build, _plans)
    return ref, fused and not FORCE_AXIS and (direction, dtype, flen, ndim) not in AXIS_PASS_CELLS


def _setup(t: torch.Tensor, ndim: int) -> int:
    """The refusals of every level, and the dtype id of the axis passes."""
    _engine._require_gpu(t)
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"Input dtype {t.dtype} not supported by the periodized transforms (float32 / float64)")
    if not 1 <= ndim <= 3:
        raise NotImplementedError("periodized levels exist for one, two and three transformed axes")
    return _engine._DTYPE_IDS[t.dtype]


def _axis_strides(t: torch.Tensor):
    return _engine._arr(ctypes.c_int64, 3)(*t.stride())


def _oai(t: torch.Tensor, axis: int) -> torch.Tensor:
    """A [B, d0(, d1(, d2))] tensor as the [outer, n, inner] view whose middle axis is ``axis`` (1 .. 3)."""
    return t.reshape(int(np.prod(t.shape[:axis])), t.shape[axis], int(np.prod(t.shape[axis + 1:])))


def _axis_fwd(src, o_lo, o_hi, dt: int, flen: int, lo, hi) -> None:
    """One analysis axis launch over [outer, n, inner] views."""
    outer, n, inner = src.shape
    _launch(0, KID_AXIS_FWD, (n,), src, _lib().mifwt_per_axis_fwd, dt, flen, outer, n, inner, src.data_ptr(), _axis_strides(src),
            o_lo.data_ptr(), _axis_strides(o_lo), o_hi.data_ptr(), _axis_strides(o_hi), lo, hi)


def _axis_inv(c_lo, c_hi, dst, dt: int, flen: int, lo, hi) -> None:
    """One synthesis axis launch over [outer, m, inner] -> [outer, n, inner] views."""
    outer, n, inner = dst.shape
    _launch(1, KID_AXIS_INV, (n,), c_lo, _lib().mifwt_per_axis_inv, dt, flen, outer, n, inner, c_lo.data_ptr(), _axis_strides(c_lo),
            c_hi.data_ptr(), _axis_strides(c_hi), dst.data_ptr(), _axis_strides(dst), lo, hi)


# ---- taps that alias ------------------------------------------------------------------------------------------------------------------
# On an axis whose period 2 M is shorter than the filter, taps j and j + 2 M meet the same sample (analysis) or add into the same
# sample (synthesis): a level then multiplies one value by several taps of alternating sign and sums the products in the data's
# precision.  The host sums such taps first, in double, and hands the kernels a filter of the same length whose first 2 M taps hold the
# sums and whose other taps are zero: the same map (every index is taken modulo 2 M), fewer roundings — in float32 the deep levels of
# short rows lose up to a digit otherwise (`stationary_transform._merge_aliased` does the same for the stationary kernels).  A launch
# has ONE bank for all its axes, so a fused 2-D launch folds only where both periods are equal; axis launches always can.
_folded: dict = {}


def _taps(lo: Sequence[float], hi: Sequence[float], periods: Sequence[int]):
    """The two tap arrays of a launch over axes of the given periods (2 M each), aliasing taps summed where the launch allows."""
    p = int(periods[0])
    if p >= len(lo) or any(int(q) != p for q in periods):
        return _engine._taps_array(lo), _engine._taps_array(hi)
    key = (tuple(lo), tuple(hi), p)
    hit = _folded.get(key)
    if hit is None:
        if len(_folded) > 512:
            _folded.clear()
        fold = lambda f: tuple(math.fsum(f[r::p]) if r < p else 0.0 for r in range(len(f)))  # noqa: E731
        hit = _folded[key] = (_engine._taps_array(fold(key[0])), _engine._taps_array(fold(key[1])))
    return hit


# ---- the two level maps (no autograd) ---------------------------------------------------------------------------------------------
def _fused_fwd(x: torch.Tensor, planes: Sequence[torch.Tensor], ref, lo, hi) -> None:
    _launch(0, KID_FWD, tuple(x.shape[1:]), x, _lib().mifwt_per_fwd, ref, x.data_ptr(), planes[0].data_ptr(), _engine._ptr_array(planes[1:]),
            lo, hi)


def level_fwd(x: torch.Tensor, dec_lo: Sequence[float], dec_hi: Sequence[float]) -> torch.Tensor:
    """x [B, n0(, n1(, n2))] -> buffer [B, 2^d, M0(, M1(, M2))], plane s = band s (bit (d-1-a) of s set <=> high-pass along axis a).
    (Three axes: the buffer is a view whose planes are dense tensors of their own.)"""
    ndim = x.dim() - 1
    dt = _setup(x, ndim)
    sig = [int(n) for n in x.shape[1:]]
    coef = [(n + 1) // 2 for n in sig]
    flen = len(dec_lo)
    b = int(x.shape[0])
    per = [2 * m for m in coef]
    if ndim == 3:
        xc = _unit_last(x)
        x2 = xc.reshape(b * sig[0], sig[1], sig[2])  # (a view of a dense volume)
        tmp = torch.empty((4, b * sig[0], coef[1], coef[2]), dtype=x.dtype, device=x.device)
        st = tmp.stride()[1:]
        ref, fused = _route(0, (0, 3, x2.shape, x2.stride(), tuple(st), x.dtype, flen), x.dtype, flen, 3,
                            lambda: _desc(2, x.dtype, 0, flen, b * sig[0], sig[1:], x2.stride(), coef[1:], st, st))
        if fused:
            out = torch.empty((8, b, *coef), dtype=x.dtype, device=x.device)
            if out.numel():
                _fused_fwd(x2, list(tmp.unbind(0)), ref, *_taps(dec_lo, dec_hi, per[1:]))
                plane = coef[1] * coef[2]
                src = tmp.view(4 * b, sig[0], plane)
                _axis_fwd(src, out[:4].view(4 * b, coef[0], plane), out[4:].view(4 * b, coef[0], plane), dt, flen, *_taps(dec_lo, dec_hi, per[:1]))
            return out.transpose(0, 1)
        x = xc
    else:
        buf = torch.empty((b, 1 << ndim, *coef), dtype=x.dtype, device=x.device)
        if buf.numel() == 0:
            return buf
        st = [buf.stride(0), *buf.stride()[2:]]
        ref, fused = _route(0, (0, ndim, x.shape, x.stride(), tuple(st), x.dtype, flen), x.dtype, flen, ndim,
                            lambda: _desc(ndim, x.dtype, 0, flen, b, sig, x.stride(), coef, st, st))
        if fused:
            _fused_fwd(x, list(buf.unbind(1)), ref, *_taps(dec_lo, dec_hi, per))
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
        lo, hi = _taps(dec_lo, dec_hi, per[axis - 1:axis])
        for pl in range(npl):
            _axis_fwd(_oai(cur[pl], axis), _oai(out[pl], axis), _oai(out[npl + pl], axis), dt, flen, lo, hi)
        cur = out
    return buf


def level_inv(bands: Sequence[torch.Tensor], rec_lo: Sequence[float], rec_hi: Sequence[float], out_extent: Sequence[int]) -> torch.Tensor:
    """bands (2^d tensors [B, M0(, M1(, M2))], band order as above) -> y [B, n0(, n1(, n2))], n in {2 M, 2 M - 1} per axis."""
    a0 = bands[0]
    ndim = a0.dim() - 1
    dt = _setup(a0, ndim)
    if len(bands) != 1 << ndim or any(t.shape != a0.shape for t in bands):
        raise ValueError("All coefficients on each level must have the same shape")
    coef = [int(m) for m in a0.shape[1:]]
    sig = [int(n) for n in out_extent]
    if any(n not in (2 * m, 2 * m - 1) or n < 1 for n, m in zip(sig, coef)):
        raise ValueError(f"a periodized level of {tuple(coef)} coefficients has no output of extent {tuple(sig)}")
    flen = len(rec_lo)
    b = int(a0.shape[0])
    per = [2 * m for m in coef]
    y = torch.empty((b, *sig), dtype=a0.dtype, device=a0.device)
    if y.numel() == 0:
        return y
    if ndim == 3:
        tmp = torch.empty((4, b * sig[0], coef[1], coef[2]), dtype=a0.dtype, device=a0.device)
        st = tmp.stride()[1:]
        y2 = y.view(b * sig[0], sig[1], sig[2])
        ref, fused = _route(1, (1, 3, y2.shape, y2.stride(), tuple(coef), tuple(st), a0.dtype, flen), a0.dtype, flen, 3,
                            lambda: _desc(2, a0.dtype, 0, flen, b * sig[0], sig[1:], y2.stride(), coef[1:], st, st))
        if fused:
            cb = [t.contiguous() for t in bands]
            plane = coef[1] * coef[2]
            lo, hi = _taps(rec_lo, rec_hi, per[:1])
            for s in range(4):
                _axis_inv(cb[s].view(b, coef[0], plane), cb[4 + s].view(b, coef[0], plane), tmp[s].view(b, sig[0], plane), dt, flen, lo, hi)
            _launch(1, KID_INV, tuple(sig[1:]), a0, _lib().mifwt_per_inv, ref, tmp[0].data_ptr(), _engine._ptr_array(list(tmp[1:].unbind(0))),
                    y.data_ptr(), *_taps(rec_lo, rec_hi, per[1:]))
            return y
    elif flen <= 20:
        ub = [bands[0], *_engine._share_strides(bands[1:])[0]]
        ref, fused = _route(1, (1, ndim, a0.shape, tuple(sig), y.stride(), ub[0].stride(), ub[1].stride(), a0.dtype, flen), a0.dtype, flen, ndim,
                            lambda: _desc(ndim, a0.dtype, 0, flen, b, sig, y.stride(), coef, ub[0].stride(), ub[1].stride()))
        if fused:
            _launch(1, KID_INV, tuple(sig), a0, _lib().mifwt_per_inv, ref, ub[0].data_ptr(), _engine._ptr_array(ub[1:]), y.data_ptr(),
                    *_taps(rec_lo, rec_hi, per))
            return y
    # The mirror of the analysis passes, first axis first: (4 +) (2 +) 1 launches.  The pass that leaves 2^k planes takes the low band
    # from plane p and the high band from plane p + 2^k; the last one writes `y`.
    cur = list(bands)
    for axis in range(1, ndim + 1):
        npl = len(cur) // 2
        out = [y] if axis == ndim else torch.empty((npl, b, *sig[:axis], *coef[axis:]), dtype=a0.dtype, device=a0.device)
        lo, hi = _taps(rec_lo, rec_hi, per[axis - 1:axis])
        for pl in range(npl):
            _axis_inv(_oai(cur[pl], axis), _oai(cur[npl + pl], axis), _oai(out[pl], axis), dt, flen, lo, hi)
        cur = out
    return y


# ---- autograd: each map's backward is the other map with the reversed taps ------------------------------------------------------------
def _fold_virtual(t: torch.Tensor, dim: int, n: int) -> torch.Tensor:
    """Gradient of repeating the last sample of an odd extent ``n`` along ``dim``: drop entry n, add it onto entry n - 1."""
    if t.shape[dim] == n:
        return t
    return torch.cat([t.narrow(dim, 0, n - 1), t.narrow(dim, n - 1, 1) + t.narrow(dim, n, 1)], dim)


class _Fwd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dec_lo, dec_hi):
        ctx.meta = (dec_lo, dec_hi, tuple(x.shape[1:]))
        return level_fwd(x, dec_lo, dec_hi)

    @staticmethod
    def backward(ctx, g):
        dec_lo, dec_hi, sig = ctx.meta
        full = tuple(n + (n & 1) for n in sig)
        g_x = _Inv.apply(tuple(dec_lo[::-1]), tuple(dec_hi[::-1]), full, *[g[:, s] for s in range(g.shape[1])])
        for a, n in enumerate(sig):
            g_x = _fold_virtual(g_x, 1 + a, n)
        return g_x, None, None


class _Inv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rec_lo, rec_hi, out_extent, *bands):
        ctx.meta = (rec_lo, rec_hi, tuple(bands[0].shape[1:]))
        return level_inv(bands, rec_lo, rec_hi, out_extent)

    @staticmethod
    def backward(ctx, g_y):
        rec_lo, rec_hi, coef = ctx.meta
        pad = []
        for a in reversed(range(len(coef))):  # (a cropped sample took no part in the output: its gradient is zero)
            pad += [0, 2 * coef[a] - g_y.shape[1 + a]]
        if any(pad):
            g_y = torch.nn.functional.pad(g_y, pad)
        g = _Fwd.apply(g_y, tuple(rec_lo[::-1]), tuple(rec_hi[::-1]))
        return (None, None, None, *[g[:, s] for s in range(g.shape[1])])


def fwd(x: torch.Tensor, dec_lo, dec_hi) -> torch.Tensor:
    if torch.is_grad_enabled() and x.requires_grad:
        return _Fwd.apply(x, tuple(dec_lo), tuple(dec_hi))
    return level_fwd(x, dec_lo, dec_hi)


def inv(bands: Sequence[torch.Tensor], rec_lo, rec_hi, out_extent: Sequence[int]) -> torch.Tensor:
    if torch.is_grad_enabled() and any(t.requires_grad for t in bands):
        return _Inv.apply(tuple(rec_lo), tuple(rec_hi), tuple(int(n) for n in out_extent), *bands)
    return level_inv(bands, rec_lo, rec_hi, out_extent)
