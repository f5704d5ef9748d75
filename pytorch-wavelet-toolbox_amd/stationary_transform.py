"""Stationary (undecimated) wavelet transform: ``swt`` / ``iswt`` (API of reference src/ptwt/stationary_transform.py), their 2-D
forms ``swt2`` / ``iswt2`` (``pywt.swt2`` / ``pywt.iswt2``; the reference has none) and their 3-D forms ``swt3`` / ``iswt3``
(``pywt.swtn`` / ``pywt.iswtn`` over three axes).

Equivalent to ``pywt.swt(..., trim_approx=True, norm=False)`` like the reference.  Each level is one HIP kernel
(C ABI ``mifwt_swt_fwd`` / ``mifwt_swt_inv``): stride-1 filter bank with dilation ``2^level`` and the periodic
extension as an index map — the reference's ``_circular_pad`` + ``F.conv1d(dilation)`` + ``split`` (:95-107) and
``stack`` + ``_circular_pad`` + grouped ``F.conv_transpose1d`` + ``mean`` (:142-156).  Differentiable w.r.t. the data
(each level kernel is the other's adjoint with reversed taps).

A 2-D level is the 1-D level along both axes of a plane.  It runs as ONE fused launch (C ABI ``mifwt_swt2_fwd`` / ``mifwt_swt2_inv``,
csrc/mifwt_swt2.hip: 1 plane in and 4 out, no intermediate plane, no transposed copy) where ``mifwt_swt2_supported`` says so, and
otherwise — filters longer than 20 taps, learnable filter banks — on the COMPOSED route: the 1-D level ops along the last axis, then
along the other one on permuted copies.  ``FORCE_COMPOSED`` selects that route for every call (cross-checks, timing baseline).

A 3-D level is the 1-D level along the three axes of a volume: ONE fused launch (``mifwt_swt3_fwd`` / ``mifwt_swt3_inv``,
csrc/mifwt_swt3.hip: 1 volume in and 8 out, no intermediate volume) where ``mifwt_swt3_supported`` says so — even lengths up to 10 —
and otherwise (longer filters, learnable banks, ``FORCE_COMPOSED``, the cells of ``COMPOSED3_CELLS``) composed from the 2-D level on
every depth slice and the 1-D level ops along depth on permuted copies.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Sequence, Tuple, Union

import torch

from . import _engine, _fwt
from ._wavelets import host_taps
from .constants import Wavelet, WaveletCoeff2d, WaveletCoeffNd, WaveletDetailTuple2d

__all__ = ["swt", "iswt", "swt2", "iswt2", "swt3", "iswt3"]

_i64, _vp, _dbl_p = ctypes.c_int64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
_vp4, _i64x4 = ctypes.c_void_p * 4, ctypes.c_int64 * 4
_engine.register_entries({
    "mifwt_swt_fwd": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _i64, _i64, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _dbl_p, _dbl_p, ctypes.c_double, _vp]),
    "mifwt_swt_inv": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _dbl_p, _dbl_p, ctypes.c_double, _vp]),
})
# The entries of the fused 2-D levels are registered when the first 2-D level asks for them (``_swt2_entries``): the record of engine
# calls (tests/golden/engine_calls.json) lists the signature of every entry the package binds at import and a recorded case for every
# launch entry among them, and these three are not part of that record.
_SWT2_LAUNCHES = {
    "mifwt_swt2_supported": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _i64, _i64, _i64, _i64]),
    "mifwt_swt2_fwd": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _vp4, _i64x4, _i64x4,
                                      _dbl_p, _dbl_p, _dbl_p, _dbl_p, ctypes.c_double, _vp]),
    "mifwt_swt2_inv": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _i64, _i64, _i64, _i64, _vp4, _i64x4, _i64x4, _vp, _i64, _i64,
                                      _dbl_p, _dbl_p, _dbl_p, _dbl_p, ctypes.c_double, _vp]),
}


def _swt2_entries():
    """The loaded library with ``mifwt_swt2_supported`` / ``_fwd`` / ``_inv`` bound (through ``_engine.register_entries``, once)."""
    lib = _engine.load_library()
    if getattr(lib.mifwt_swt2_fwd, "argtypes", None) is None:
        _engine.register_entries(_SWT2_LAUNCHES)
    return lib


# the fused 3-D levels likewise (``_swt3_entries``)
_vp8, _i64x8, _dbl_p6 = ctypes.c_void_p * 8, ctypes.c_int64 * 8, _dbl_p * 6
SWT3_PLAN_INTS = 11  # MIFWT_SWT3_PLAN_INTS
_SWT3_LAUNCHES = {
    "mifwt_swt3_supported": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _i64, _i64, _i64, _i64, _i64]),
    "mifwt_swt3_fwd": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _vp8, _i64x8, _i64x8,
                                      _i64x8, _dbl_p6, ctypes.c_double, _vp]),
    "mifwt_swt3_inv": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, _i64, _i64, _i64, _i64, _i64, _vp8, _i64x8, _i64x8, _i64x8, _vp, _i64, _i64,
                                      _i64, _dbl_p6, ctypes.c_double, _vp]),
    "mifwt_swt3_plan": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, _i64, _i64, _i64, _i64, _i64, ctypes.POINTER(ctypes.c_int),
                                       ctypes.c_int]),
}


def _swt3_entries():
    """The loaded library with ``mifwt_swt3_supported`` / ``_fwd`` / ``_inv`` / ``_plan`` bound (once)."""
    lib = _engine.load_library()
    if getattr(lib.mifwt_swt3_fwd, "argtypes", None) is None:
        _engine.register_entries(_SWT3_LAUNCHES)
    return lib


KID_SWT2, KID_ISWT2 = 34, 35  # kernel ids of the fused 2-D levels (``_engine.launch_count`` counts them under these ids)
KID_SWT3, KID_ISWT3 = 36, 37  # kernel ids of the fused 3-D levels
_rows = _engine._unit_last  # [B, N] with contiguous samples (row stride free)


def _level_fwd(x: torch.Tensor, lo: Sequence[float], hi: Sequence[float], dilation: int, scale: float) -> torch.Tensor:
    """x [B, N] -> buffer [B, 2, N]: plane 0 low-pass, plane 1 high-pass."""
    _engine._require_gpu(x)
    x = _rows(x)
    b, n = x.shape
    buf = torch.empty((b, 2, n), dtype=x.dtype, device=x.device)
    if buf.numel() == 0:
        return buf
    _engine._enqueue(x, _engine.load_library().mifwt_swt_fwd, _engine._DTYPE_IDS[x.dtype], len(lo), b, n, dilation, x.data_ptr(), x.stride(0),
                     buf.data_ptr(), buf.data_ptr() + n * buf.element_size(), 2 * n, 2 * n, _engine._taps_array(lo), _engine._taps_array(hi), scale)
    return buf


def _level_inv(a: torch.Tensor, d: torch.Tensor, lo: Sequence[float], hi: Sequence[float], dilation: int,
               scale: float) -> torch.Tensor:
    _engine._require_gpu(a)
    a, d = _rows(a), _rows(d)
    b, n = a.shape
    y = torch.empty((b, n), dtype=a.dtype, device=a.device)
    if y.numel() == 0:
        return y
    _engine._enqueue(a, _engine.load_library().mifwt_swt_inv, _engine._DTYPE_IDS[a.dtype], len(lo), b, n, dilation, a.data_ptr(), d.data_ptr(),
                     a.stride(0), d.stride(0), y.data_ptr(), n, _engine._taps_array(lo), _engine._taps_array(hi), scale)
    return y


# ---- learnable filter banks, second order (the per-level maps closed under differentiation, as _fwt._Axis1 … for the decimated levels) ----
# A stationary level is bilinear in (signal, taps):  lo[n] = s sum_m h[m] x[(n + D (L/2 - m)) mod N].  Analysis A(h) x, its transpose
# A(h)^T g (= the synthesis kernel with reversed taps) and the tap correlation C(x, g) form a set closed under differentiation; the
# synthesis y = S(r)(a, d), S(r)^T g_y (= the analysis kernel with reversed taps) and C'(a, d, g_y) likewise.
def _rev(t: torch.Tensor) -> torch.Tensor:
    return t.flip(0)


class _Swt1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lo_t, hi_t, dilation, scale):
        ctx.meta = (dilation, scale)
        ctx.save_for_backward(x, lo_t, hi_t)
        return _level_fwd(x, _fwt._host_floats_of(lo_t), _fwt._host_floats_of(hi_t), dilation, scale)

    @staticmethod
    def backward(ctx, g):
        x, lo_t, hi_t = ctx.saved_tensors
        dilation, scale = ctx.meta
        g_x = _Iswt1.apply(g[:, 0], g[:, 1], _rev(lo_t), _rev(hi_t), dilation, scale) if ctx.needs_input_grad[0] else None
        t_lo, t_hi = _fwt._tap_pair(ctx.needs_input_grad[1] or ctx.needs_input_grad[2], _Swt1Corr, lo_t, hi_t, x, g, lo_t.numel(), dilation, scale)
        return g_x, t_lo, t_hi, None, None


class _Iswt1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, d, lo_t, hi_t, dilation, scale):
        ctx.meta = (dilation, scale)
        ctx.save_for_backward(a, d, lo_t, hi_t)
        return _level_inv(a, d, _fwt._host_floats_of(lo_t), _fwt._host_floats_of(hi_t), dilation, scale)

    @staticmethod
    def backward(ctx, g_y):
        a, d, lo_t, hi_t = ctx.saved_tensors
        dilation, scale = ctx.meta
        g_a = g_d = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gb = _Swt1.apply(g_y, _rev(lo_t), _rev(hi_t), dilation, scale)
            g_a, g_d = gb[:, 0], gb[:, 1]
        t_lo, t_hi = _fwt._tap_pair(ctx.needs_input_grad[2] or ctx.needs_input_grad[3], _Iswt1Corr, lo_t, hi_t, a, d, g_y, lo_t.numel(), dilation, scale)
        return g_a, g_d, t_lo, t_hi, None, None


class _Swt1Corr(torch.autograd.Function):
    """(x [B, N], g [B, 2, N]) -> (t_lo, t_hi):  t_b[m] = s sum_n g_b[n] x[(n + D L/2 - D m) mod N]."""

    @staticmethod
    def forward(ctx, x, g, flen, dilation, scale):
        ctx.meta = (dilation, scale)
        ctx.save_for_backward(x, g)
        t_lo = torch.zeros(flen, dtype=torch.float64, device=x.device)
        t_hi = torch.zeros_like(t_lo)
        _engine.ENGINE.tap_correlate_dilated(g[:, 0], x, flen, dilation * (flen // 2), -dilation, t_lo)
        _engine.ENGINE.tap_correlate_dilated(g[:, 1], x, flen, dilation * (flen // 2), -dilation, t_hi)
        return t_lo * scale, t_hi * scale

    @staticmethod
    def backward(ctx, w_lo, w_hi):
        x, g = ctx.saved_tensors
        dilation, scale = ctx.meta
        w_lo, w_hi = w_lo.to(x.dtype), w_hi.to(x.dtype)
        g_x = _Iswt1.apply(g[:, 0], g[:, 1], _rev(w_lo), _rev(w_hi), dilation, scale) if ctx.needs_input_grad[0] else None
        g_g = _Swt1.apply(x, w_lo, w_hi, dilation, scale) if ctx.needs_input_grad[1] else None
        return g_x, g_g, None, None, None


class _Iswt1Corr(torch.autograd.Function):
    """(a, d, g_y [B, N]) -> (t_lo, t_hi):  t_lo[j] = s sum_n g_y[n] a[(n + D (L/2 - 1) - D j) mod N]."""

    @staticmethod
    def forward(ctx, a, d, g_y, flen, dilation, scale):
        ctx.meta = (dilation, scale)
        ctx.save_for_backward(a, d, g_y)
        t_lo = torch.zeros(flen, dtype=torch.float64, device=a.device)
        t_hi = torch.zeros_like(t_lo)
        _engine.ENGINE.tap_correlate_dilated(g_y, a, flen, dilation * (flen // 2 - 1), -dilation, t_lo)
        _engine.ENGINE.tap_correlate_dilated(g_y, d, flen, dilation * (flen // 2 - 1), -dilation, t_hi)
        return t_lo * scale, t_hi * scale

    @staticmethod
    def backward(ctx, w_lo, w_hi):
        a, d, g_y = ctx.saved_tensors
        dilation, scale = ctx.meta
        w_lo, w_hi = w_lo.to(a.dtype), w_hi.to(a.dtype)
        g_a = g_d = g_gy = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gb = _Swt1.apply(g_y, _rev(w_lo), _rev(w_hi), dilation, scale)
            g_a, g_d = gb[:, 0], gb[:, 1]
        if ctx.needs_input_grad[2]:
            g_gy = _Iswt1.apply(a, d, w_lo, w_hi, dilation, scale)
        return g_a, g_d, g_gy, None, None, None


class _SwtLevelGrad(torch.autograd.Function):
    """First-order gradients of a stationary analysis level as an op whose backward has the mixed second derivatives with a learnable
    filter bank (see _fwt._AnalysisLevelGrad)."""

    @staticmethod
    def forward(ctx, g_buf, x, lo_t, hi_t, lo, hi, dilation, scale):
        ctx.meta = (dilation, scale)
        ctx.save_for_backward(g_buf, x, lo_t, hi_t)
        g_x = _level_inv(g_buf[:, 0], g_buf[:, 1], lo[::-1], hi[::-1], dilation, scale)
        L = len(lo)
        t_lo = torch.zeros(L, dtype=torch.float64, device=x.device)
        t_hi = torch.zeros_like(t_lo)
        _engine.ENGINE.tap_correlate_dilated(g_buf[:, 0], x, L, dilation * (L // 2), -dilation, t_lo)
        _engine.ENGINE.tap_correlate_dilated(g_buf[:, 1], x, L, dilation * (L // 2), -dilation, t_hi)
        return g_x, _fwt._like(t_lo * scale, lo_t), _fwt._like(t_hi * scale, hi_t)

    @staticmethod
    def backward(ctx, w_x, w_lo, w_hi):
        g_buf, x, lo_t, hi_t = ctx.saved_tensors
        _fwt._third_order_refused((lo_t, hi_t))
        dilation, scale = ctx.meta
        d = _fwt._partials_at([g_buf, x, lo_t, hi_t], lambda lv: _Swt1.apply(lv[1], lv[2], lv[3], dilation, scale), 0, [w_x, w_lo, w_hi])
        return d[0], d[1], d[2], d[3], None, None, None, None


class _IswtLevelGrad(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g_y, a, d, lo_t, hi_t, lo, hi, dilation, scale):
        ctx.meta = (dilation, scale)
        ctx.save_for_backward(g_y, a, d, lo_t, hi_t)
        g = _level_fwd(g_y, lo[::-1], hi[::-1], dilation, scale)
        L = len(lo)
        t_lo = torch.zeros(L, dtype=torch.float64, device=g_y.device)
        t_hi = torch.zeros_like(t_lo)
        _engine.ENGINE.tap_correlate_dilated(g_y, a, L, dilation * (L // 2 - 1), -dilation, t_lo)
        _engine.ENGINE.tap_correlate_dilated(g_y, d, L, dilation * (L // 2 - 1), -dilation, t_hi)
        return g[:, 0], g[:, 1], _fwt._like(t_lo * scale, lo_t), _fwt._like(t_hi * scale, hi_t)

    @staticmethod
    def backward(ctx, w_a, w_d, w_lo, w_hi):
        g_y, a, d, lo_t, hi_t = ctx.saved_tensors
        _fwt._third_order_refused((lo_t, hi_t))
        dilation, scale = ctx.meta
        out = _fwt._partials_at([g_y, a, d, lo_t, hi_t], lambda lv: _Iswt1.apply(lv[1], lv[2], lv[3], lv[4], dilation, scale), 0,
                                [w_a, w_d, w_lo, w_hi])
        return out[0], out[1], out[2], out[3], out[4], None, None, None, None


class _SwtLevel(torch.autograd.Function):
    """One stationary analysis level (free output scale), differentiable w.r.t. its input and (optionally) the dec taps.  With
    reversed taps the synthesis kernel is its transpose and vice versa, so each Function's backward is the other Function:
    gradients of any order w.r.t. the data, as the reference has them from _circular_pad + conv1d; the tap gradients (first
    order) are the dilated correlation ``mifwt_tap_correlate_dilated``.  ``lo_t`` / ``hi_t``: the tap TENSORS or None (they only tie
    the op into the graph; the kernels take the host copies)."""

    @staticmethod
    def forward(ctx, x, lo, hi, dilation, scale=1.0, lo_t=None, hi_t=None):
        ctx.meta = (lo, hi, dilation, scale)
        ctx.taps = (lo_t, hi_t)
        need_taps = any(t is not None and t.requires_grad for t in (lo_t, hi_t))
        ctx.save_for_backward(x if need_taps else None)
        return _level_fwd(x, lo, hi, dilation, scale)

    @staticmethod
    def backward(ctx, g_buf):
        lo, hi, dilation, scale = ctx.meta
        (x,) = ctx.saved_tensors
        if x is not None and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ctx.taps):
            # create_graph=True with a learnable filter bank: the same gradients as an op that carries the mixed second derivatives
            g_x, g_lo, g_hi = _SwtLevelGrad.apply(g_buf, x, ctx.taps[0], ctx.taps[1], lo, hi, dilation, scale)
            need = ctx.needs_input_grad
            return g_x if need[0] else None, None, None, None, None, g_lo if need[5] else None, g_hi if need[6] else None
        g_x = _IswtLevel.apply(g_buf[:, 0], g_buf[:, 1], lo[::-1], hi[::-1], dilation, scale) if ctx.needs_input_grad[0] else None
        g_lo = g_hi = None
        if x is not None and (ctx.needs_input_grad[5] or ctx.needs_input_grad[6]):
            # lo[n] = s sum_m h[m] x[(n + D (L/2 - m)) mod N]  =>  dL/dh[m] = s sum_n g_lo[n] x[(n + D L/2 - D m) mod N]
            L = len(lo)
            g_lo = torch.zeros(L, dtype=torch.float64, device=x.device)
            g_hi = torch.zeros_like(g_lo)
            gb = g_buf.detach()
            _engine.ENGINE.tap_correlate_dilated(gb[:, 0], x, L, dilation * (L // 2), -dilation, g_lo)
            _engine.ENGINE.tap_correlate_dilated(gb[:, 1], x, L, dilation * (L // 2), -dilation, g_hi)
            g_lo, g_hi = _fwt._like(g_lo * scale, ctx.taps[0]), _fwt._like(g_hi * scale, ctx.taps[1])
        return g_x, None, None, None, None, g_lo, g_hi


class _IswtLevel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, d, lo, hi, dilation, scale=0.5, lo_t=None, hi_t=None):
        ctx.meta = (lo, hi, dilation, scale)
        ctx.taps = (lo_t, hi_t)
        need_taps = any(t is not None and t.requires_grad for t in (lo_t, hi_t))
        if need_taps:
            ctx.save_for_backward(a, d)
        else:
            ctx.save_for_backward()
        return _level_inv(a, d, lo, hi, dilation, scale)

    @staticmethod
    def backward(ctx, g_y):
        lo, hi, dilation, scale = ctx.meta
        if ctx.saved_tensors and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ctx.taps):
            a, d = ctx.saved_tensors
            g_a, g_d, g_lo, g_hi = _IswtLevelGrad.apply(g_y, a, d, ctx.taps[0], ctx.taps[1], lo, hi, dilation, scale)
            need = ctx.needs_input_grad
            return (g_a if need[0] else None, g_d if need[1] else None, None, None, None, None, g_lo if need[6] else None,
                    g_hi if need[7] else None)
        g_a = g_d = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            g = _SwtLevel.apply(g_y, lo[::-1], hi[::-1], dilation, scale)
            g_a, g_d = g[:, 0], g[:, 1]
        g_lo = g_hi = None
        saved = ctx.saved_tensors
        if saved and (ctx.needs_input_grad[6] or ctx.needs_input_grad[7]):
            # y[n] = s sum_j g_lo[j] a[(n + D (L/2 - 1 - j)) mod N] + g_hi[j] d[...]  =>  dL/dg_lo[j] = s sum_n g_y[n] a[(n + D (L/2 - 1) - D j) mod N]
            L = len(lo)
            g_lo = torch.zeros(L, dtype=torch.float64, device=g_y.device)
            g_hi = torch.zeros_like(g_lo)
            gy = g_y.detach()
            _engine.ENGINE.tap_correlate_dilated(gy, saved[0], L, dilation * (L // 2 - 1), -dilation, g_lo)
            _engine.ENGINE.tap_correlate_dilated(gy, saved[1], L, dilation * (L // 2 - 1), -dilation, g_hi)
            g_lo, g_hi = _fwt._like(g_lo * scale, ctx.taps[0]), _fwt._like(g_hi * scale, ctx.taps[1])
        return g_a, g_d, None, None, None, None, g_lo, g_hi


def swt_max_level(input_len: int) -> int:
    """``pywt.swt_max_level``: how often the length can be halved (src/ptwt/stationary_transform.py:93)."""
    level = 0
    while input_len > 0 and input_len % 2 == 0:
        input_len //= 2
        level += 1
    return level


def swt(data: torch.Tensor, wavelet: Union[Wavelet, str], level: Optional[int] = None, *,
        axis: _fwt.AxisHint = None) -> List[torch.Tensor]:
    """Multi-level 1-D stationary transform; returns ``[cA_n, cD_n, ..., cD_1]``, every entry as long as the input
    (drop-in for ``ptwt.swt``, src/ptwt/stationary_transform.py:56-110)."""
    axes = _fwt._ensure_axes(axis, 1)
    layout = _fwt._Layout(data, 1, axes)
    x = layout.fold(data)
    dec_lo, dec_hi, _, _ = host_taps(wavelet)
    tap_t = _fwt._tap_tensors(wavelet)  # learnable filter bank: the taps stay in the graph (src/ptwt/_util.py:115-132)
    if level is None:
        level = swt_max_level(x.shape[-1])
    out: List[torch.Tensor] = []
    cur = x
    for lvl in range(level):
        if torch.is_grad_enabled() and (cur.requires_grad or tap_t is not None):
            buf = _SwtLevel.apply(cur, dec_lo, dec_hi, 2 ** lvl, 1.0, *_fwt._graph_taps(tap_t, 0))
        else:
            buf = _level_fwd(cur, dec_lo, dec_hi, 2 ** lvl, 1.0)
        out.append(layout.unfold(buf[:, 1]))
        cur = buf[:, 0]
    out.append(layout.unfold(cur))
    out.reverse()
    return out


def iswt(coeffs: Sequence[torch.Tensor], wavelet: Union[Wavelet, str], *, axis: _fwt.AxisHint = None) -> torch.Tensor:
    """Inverse of :func:`swt` (drop-in for ``ptwt.iswt``, src/ptwt/stationary_transform.py:113-160)."""
    coeffs = list(coeffs)
    if not coeffs or not isinstance(coeffs[0], torch.Tensor):
        raise ValueError("First element of coeffs must be the approximation coefficient tensor.")
    axes = _fwt._ensure_axes(axis, 1)
    layout = _fwt._Layout(coeffs[0], 1, axes)
    for t in coeffs:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"Unexpected input type {type(t)}")
    _fwt._check_same_device_dtype(coeffs)
    _, _, rec_lo, rec_hi = host_taps(wavelet)
    tap_t = _fwt._tap_tensors(wavelet)
    cur = layout.fold(coeffs[0])
    details = [layout.fold(t) for t in coeffs[1:]]
    for pos, det in enumerate(details):
        dilation = 2 ** (len(details) - pos - 1)
        if det.shape != cur.shape:
            raise RuntimeError("stack expects each tensor to be equal size")  # torch.stack in the reference (:146)
        if torch.is_grad_enabled() and (cur.requires_grad or det.requires_grad or tap_t is not None):
            cur = _IswtLevel.apply(cur, det, rec_lo, rec_hi, dilation, 0.5, *_fwt._graph_taps(tap_t, 2))
        else:
            cur = _level_inv(cur, det, rec_lo, rec_hi, dilation, 0.5)
    return layout.unfold(cur)


# ---- 2-D levels ---------------------------------------------------------------------------------------------------------------------------
# A level takes FOUR filters (row_lo, row_hi along the last axis; col_lo, col_hi along the one before it): the transforms pass the
# wavelet's pair twice, the tests pass four different ones.  Planes of a level buffer [B, 4, H, W]: cA, cH, cV, cD — cH is high-pass
# along axis -2 and low-pass along axis -1, as wavedec2 names its bands.
FORCE_COMPOSED = False  # True: every 2-D level takes the composed route (the fused kernels' cross-check and timing baseline)
# (direction "fwd" / "inv", dtype, filter length) cells that stay on the composed route because the fused launch did not beat it
# there (tools/swt2_bench.py, EXPERIMENTS.md "2-D stationary levels"): the project's rule for every fused kernel.
COMPOSED2_CELLS: set = set()
Taps4 = Tuple[Sequence[float], Sequence[float], Sequence[float], Sequence[float]]


def _fused2(direction: str, dtype: torch.dtype, flen: int, b: int, h: int, w: int, dilation: int) -> bool:
    """Does the fused 2-D launch serve this level?  (``mifwt_swt2_supported``: float32 / float64, even lengths up to 20.)"""
    if FORCE_COMPOSED or dtype not in (torch.float32, torch.float64) or (direction, dtype, flen) in COMPOSED2_CELLS:
        return False
    return bool(_swt2_entries().mifwt_swt2_supported(_engine._DTYPE_IDS[dtype], flen, b, h, w, dilation))


_merged: dict = {}


def _merge_aliased(taps: Sequence[float], dilation: int, n: int) -> Tuple[float, ...]:
    """Along an axis of ``n`` samples, taps m and m' read the same sample when ``D (m - m')`` is a multiple of n (extent 1: all of
    them).  Their sum is taken HERE, in double, and put on the first tap of each such class (zeros on the others): the same level, but
    a sum of many taps that cancels is no longer rounded tap by tap in the kernel's float32 (a 1 x 1 plane under 22 random taps came
    out 1.1e-6 off, norm-wise, on both routes).  Filters whose taps all read different samples come back as they are."""
    taps = tuple(taps)
    flen = len(taps)
    if n > dilation * (flen - 1):
        return taps
    key = (taps, dilation, n)
    out = _merged.get(key)
    if out is None:
        classes: dict = {}
        for m in range(flen):
            classes.setdefault((dilation * m) % n, []).append(m)
        merged = [0.0] * flen
        for members in classes.values():
            merged[members[0]] = math.fsum(taps[m] for m in members)
        if len(_merged) > 512:
            _merged.clear()
        out = _merged[key] = tuple(merged)
    return out


def _merged4(taps: Taps4, dilation: int, h: int, w: int) -> Taps4:
    return (_merge_aliased(taps[0], dilation, w), _merge_aliased(taps[1], dilation, w),
            _merge_aliased(taps[2], dilation, h), _merge_aliased(taps[3], dilation, h))


def _composed2_fwd(x: torch.Tensor, taps: Taps4, dilation: int, scale: float, tap_t=None) -> torch.Tensor:
    """The level from 1-D level ops: along axis -1, then along axis -2 on a permuted copy.  Differentiable (data, and the taps when
    ``tap_t`` = the four tap tensors is given) when grad mode is on."""
    b, h, w = x.shape
    tt = tap_t if tap_t is not None else (None,) * 4
    diff = torch.is_grad_enabled() and (x.requires_grad or tap_t is not None)

    def op(rows, lo, hi, s, lo_t, hi_t):
        return _SwtLevel.apply(rows, lo, hi, dilation, s, lo_t, hi_t) if diff else _level_fwd(rows, lo, hi, dilation, s)

    rows = op(x.reshape(b * h, w), taps[0], taps[1], 1.0, tt[0], tt[1]).reshape(b, h, 2, w)  # [B, H, row band, W]
    cols = op(rows.permute(0, 2, 3, 1).reshape(b * 2 * w, h), taps[2], taps[3], scale, tt[2], tt[3])  # [B (row band) W, col band, H]
    return cols.reshape(b, 2, w, 2, h).permute(0, 1, 3, 4, 2).reshape(b, 4, h, w)  # plane = 2 (row band) + (col band)


def _composed2_inv(bands: Sequence[torch.Tensor], taps: Taps4, dilation: int, scale: float, tap_t=None) -> torch.Tensor:
    """U = S_row(cA, cV), V = S_row(cH, cD), y = S_col(U, V) from the 1-D synthesis level op."""
    ca, ch, cv, cd = bands
    b, h, w = ca.shape
    tt = tap_t if tap_t is not None else (None,) * 4
    diff = torch.is_grad_enabled() and (any(t.requires_grad for t in bands) or tap_t is not None)

    def op(a, d, lo, hi, s, lo_t, hi_t):
        return _IswtLevel.apply(a, d, lo, hi, dilation, s, lo_t, hi_t) if diff else _level_inv(a, d, lo, hi, dilation, s)

    lows = torch.stack((ca, ch)).reshape(2 * b * h, w)   # the operands the row filters' low-pass takes, for U and for V
    highs = torch.stack((cv, cd)).reshape(2 * b * h, w)
    uv = op(lows, highs, taps[0], taps[1], 1.0, tt[0], tt[1]).reshape(2, b, h, w).permute(0, 1, 3, 2).reshape(2, b * w, h)
    y = op(uv[0], uv[1], taps[2], taps[3], scale, tt[2], tt[3])
    return y.reshape(b, w, h).permute(0, 2, 1).contiguous()


def _level2_fwd(x: torch.Tensor, taps: Taps4, dilation: int, scale: float, composed: bool = False) -> torch.Tensor:
    """x [B, H, W] -> level buffer [B, 4, H, W] (planes cA, cH, cV, cD): the fused launch where it exists, else (or with
    ``composed``) the composed route.  No autograd."""
    _engine._require_gpu(x)
    b, h, w = x.shape
    flen = len(taps[0])
    taps = _merged4(taps, dilation, h, w)
    if composed or not _fused2("fwd", x.dtype, flen, b, h, w, dilation):
        with torch.no_grad():
            return _composed2_fwd(x.detach(), taps, dilation, scale)
    x = _rows(x)
    buf = torch.empty((b, 4, h, w), dtype=x.dtype, device=x.device)
    if buf.numel() == 0:
        return buf
    plane = h * w * buf.element_size()
    _engine._enqueue(x, _swt2_entries().mifwt_swt2_fwd, _engine._DTYPE_IDS[x.dtype], flen, b, h, w, dilation, x.data_ptr(),
                     x.stride(0), x.stride(1), _vp4(*[buf.data_ptr() + q * plane for q in range(4)]), _i64x4(*[4 * h * w] * 4),
                     _i64x4(*[w] * 4), *[_engine._taps_array(t) for t in taps], scale)
    return buf


def _level2_inv(bands: Sequence[torch.Tensor], taps: Taps4, dilation: int, scale: float, composed: bool = False) -> torch.Tensor:
    """(cA, cH, cV, cD), each [B, H, W] with any image / row strides -> y [B, H, W].  No autograd."""
    _engine._require_gpu(bands[0])
    b, h, w = bands[0].shape
    flen = len(taps[0])
    taps = _merged4(taps, dilation, h, w)
    if composed or not _fused2("inv", bands[0].dtype, flen, b, h, w, dilation):
        with torch.no_grad():
            return _composed2_inv([t.detach() for t in bands], taps, dilation, scale)
    bands = [_rows(t) for t in bands]
    y = torch.empty((b, h, w), dtype=bands[0].dtype, device=bands[0].device)
    if y.numel() == 0:
        return y
    _engine._enqueue(y, _swt2_entries().mifwt_swt2_inv, _engine._DTYPE_IDS[y.dtype], flen, b, h, w, dilation,
                     _vp4(*[t.data_ptr() for t in bands]), _i64x4(*[t.stride(0) for t in bands]), _i64x4(*[t.stride(1) for t in bands]),
                     y.data_ptr(), h * w, w, *[_engine._taps_array(t) for t in taps], scale)
    return y


def _rev4(taps: Taps4) -> Taps4:
    return tuple(t[::-1] for t in taps)


class _Swt2Level(torch.autograd.Function):
    """One 2-D analysis level with host taps and a free scale.  Its transpose is the synthesis level with all four filters reversed and
    the same scale (and vice versa), so each Function's backward is the other Function: data gradients of any order."""

    @staticmethod
    def forward(ctx, x, taps, dilation, scale):
        ctx.meta = (taps, dilation, scale)
        return _level2_fwd(x, taps, dilation, scale)

    @staticmethod
    def backward(ctx, g_buf):
        taps, dilation, scale = ctx.meta
        return _Iswt2Level.apply(g_buf[:, 0], g_buf[:, 1], g_buf[:, 2], g_buf[:, 3], _rev4(taps), dilation, scale), None, None, None


class _Iswt2Level(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ca, ch, cv, cd, taps, dilation, scale):
        ctx.meta = (taps, dilation, scale)
        return _level2_inv((ca, ch, cv, cd), taps, dilation, scale)

    @staticmethod
    def backward(ctx, g_y):
        taps, dilation, scale = ctx.meta
        g = _Swt2Level.apply(g_y, _rev4(taps), dilation, scale)
        return g[:, 0], g[:, 1], g[:, 2], g[:, 3], None, None, None


def _check_dtype2(t: torch.Tensor) -> None:
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"Input dtype {t.dtype} not supported")


def swt2(data: torch.Tensor, wavelet: Union[Wavelet, str], level: Optional[int] = None, *,
         axes: Tuple[int, int] = (-2, -1)) -> WaveletCoeff2d:
    """Multi-level 2-D stationary transform over ``axes``.  Returns ``[cA_n, WaveletDetailTuple2d(cH_n, cV_n, cD_n), ...,
    WaveletDetailTuple2d(cH_1, cV_1, cD_1)]``, every tensor of the input's shape: the container of ``wavedec2``, with its band names
    (``cH`` high-pass along ``axes[0]`` and low-pass along ``axes[1]``, ``cV`` the other way round, ``cD`` high-pass along both), and
    equal to ``pywt.swt2(..., trim_approx=True, norm=False)``.

    A level is the level of :func:`swt` (periodic, dilation ``2^level index``, scale 1) along both axes.  ``level=None`` means
    ``min(swt_max_level(H), swt_max_level(W))`` — odd extents give ``[data]``; as in :func:`swt` no level is refused, the periodic index
    map wraps as often as needed.  Only float32 and float64 are accepted: float16 / bfloat16 raise ``ValueError("Input dtype ... not
    supported")`` even inside ``half_storage()`` (the fused kernels have no 16-bit form).  Differentiable w.r.t. the data to any
    order; a learnable (tensor-valued) filter bank runs on the composed route and has tap gradients up to second order."""
    axes = _fwt._ensure_axes(axes, 2)
    layout = _fwt._Layout(data, 2, axes)
    _check_dtype2(data)
    x = layout.fold(data)
    dec_lo, dec_hi, _, _ = host_taps(wavelet)
    tap_t = _fwt._tap_tensors(wavelet)
    if level is None:
        level = min(swt_max_level(x.shape[-2]), swt_max_level(x.shape[-1]))
    taps = (tuple(dec_lo), tuple(dec_hi), tuple(dec_lo), tuple(dec_hi))
    out: list = []
    cur = x
    for lvl in range(level):
        _engine._require_gpu(cur)
        if tap_t is not None:
            buf = _composed2_fwd(cur, taps, 2 ** lvl, 1.0, (tap_t[0], tap_t[1], tap_t[0], tap_t[1]))
        elif torch.is_grad_enabled() and cur.requires_grad:
            buf = _Swt2Level.apply(cur, taps, 2 ** lvl, 1.0)
        else:
            buf = _level2_fwd(cur, taps, 2 ** lvl, 1.0)
        out.append(WaveletDetailTuple2d(*(layout.unfold(buf[:, q]) for q in (1, 2, 3))))
        cur = buf[:, 0]
    out.append(layout.unfold(cur))
    out.reverse()
    return out


def iswt2(coeffs: WaveletCoeff2d, wavelet: Union[Wavelet, str], *, axes: Tuple[int, int] = (-2, -1)) -> torch.Tensor:
    """Inverse of :func:`swt2` (``pywt.iswt2`` of coefficients with ``trim_approx=True, norm=False``).  Per level ``U = S(cA, cV)`` and
    ``V = S(cH, cD)`` along ``axes[1]``, ``y = S(U, V)`` along ``axes[0]``, with ``S`` the synthesis level of :func:`iswt` (scale 1/2
    per axis): a linear map of ANY coefficient set, not only of images of ``swt2``.  float32 / float64 only, as :func:`swt2`."""
    coeffs = list(coeffs)
    if not coeffs or not isinstance(coeffs[0], torch.Tensor):
        raise ValueError("First element of coeffs must be the approximation coefficient tensor.")
    axes = _fwt._ensure_axes(axes, 2)
    layout = _fwt._Layout(coeffs[0], 2, axes)
    flat = [coeffs[0]]
    for c in coeffs[1:]:
        if not isinstance(c, tuple) or len(c) != 3:
            raise ValueError(f"Unexpected detail coefficient type: {type(c)}. Detail coefficients must be a 3-tuple of tensors as "
                             "returned by swt2.")
        for t in c:
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"Unexpected input type {type(t)}")
        flat.extend(c)
    _fwt._check_same_device_dtype(flat)
    _check_dtype2(coeffs[0])
    _, _, rec_lo, rec_hi = host_taps(wavelet)
    tap_t = _fwt._tap_tensors(wavelet)
    taps = (tuple(rec_lo), tuple(rec_hi), tuple(rec_lo), tuple(rec_hi))
    cur = layout.fold(coeffs[0])
    details = [tuple(layout.fold(t) for t in c) for c in coeffs[1:]]
    for pos, det in enumerate(details):
        for t in det:
            if t.shape != cur.shape:
                raise ValueError(f"detail coefficients of shape {tuple(t.shape)} do not match the approximation of shape "
                                 f"{tuple(cur.shape)} (folded to [batch, H, W])")
    for pos, det in enumerate(details):
        dilation = 2 ** (len(details) - pos - 1)
        bands = (cur, *det)
        _engine._require_gpu(cur)
        if tap_t is not None:
            cur = _composed2_inv(bands, taps, dilation, 0.25, (tap_t[2], tap_t[3], tap_t[2], tap_t[3]))
        elif torch.is_grad_enabled() and any(t.requires_grad for t in bands):
            cur = _Iswt2Level.apply(*bands, taps, dilation, 0.25)
        else:
            cur = _level2_inv(bands, taps, dilation, 0.25)
    return layout.unfold(cur)


# ---- 3-D levels ---------------------------------------------------------------------------------------------------------------------------
# A level takes SIX filters (w_lo, w_hi along the last axis; h_lo, h_hi along the one before it; z_lo, z_hi along depth): the transforms
# pass the wavelet's pair three times, the tests pass six different ones.  Planes of a level buffer [B, 8, Dz, H, W]: plane
# 4 [depth high] + 2 [axis -2 high] + [axis -1 high] — aaa, aad, ada, add, daa, dad, dda, ddd, the keys of wavedec3 in their order.
# (direction "fwd" / "inv", dtype, filter length) cells that stay on the composed route because the fused launch did not beat it
# there (tools/swt3_bench.py, EXPERIMENTS.md part S): the project's rule for every fused kernel.
COMPOSED3_CELLS: set = set()
Taps6 = Tuple[Sequence[float], Sequence[float], Sequence[float], Sequence[float], Sequence[float], Sequence[float]]
_KEYS3 = _fwt._KEYS_ND[3]


def _fused3(direction: str, dtype: torch.dtype, flen: int, b: int, dz: int, h: int, w: int, dilation: int) -> bool:
    """Does the fused 3-D launch serve this level?  (``mifwt_swt3_supported``: float32 / float64, even lengths up to 10.)"""
    if FORCE_COMPOSED or dtype not in (torch.float32, torch.float64) or (direction, dtype, flen) in COMPOSED3_CELLS:
        return False
    return bool(_swt3_entries().mifwt_swt3_supported(_engine._DTYPE_IDS[dtype], flen, b, dz, h, w, dilation))


def _merged6(taps: Taps6, dilation: int, dz: int, h: int, w: int) -> Taps6:
    """:func:`_merge_aliased` per axis: each of the six filters against the extent it runs along."""
    return tuple(_merge_aliased(t, dilation, n) for t, n in zip(taps, (w, w, h, h, dz, dz)))


def _composed3_fwd(x: torch.Tensor, taps: Taps6, dilation: int, scale: float, tap_t=None) -> torch.Tensor:
    """The level from what exists: the 2-D level on every depth slice ([B Dz, H, W]), then the 1-D level op along depth on a permuted
    copy.  Differentiable (data, and the taps when ``tap_t`` = the six tap tensors is given) when grad mode is on."""
    b, dz, h, w = x.shape
    diff = torch.is_grad_enabled() and (x.requires_grad or tap_t is not None)
    planes = x.reshape(b * dz, h, w)
    if tap_t is not None:
        p2 = _composed2_fwd(planes, taps[:4], dilation, 1.0, tuple(tap_t[:4]))
    elif diff:
        p2 = _Swt2Level.apply(planes, tuple(taps[:4]), dilation, 1.0)
    else:
        p2 = _level2_fwd(planes, taps[:4], dilation, 1.0)
    # [B Dz, 2 [axis -1 high] + [axis -2 high], H, W] -> depth last
    lines = p2.reshape(b, dz, 4, h, w).permute(0, 2, 3, 4, 1).reshape(b * 4 * h * w, dz)
    if diff:
        zt = (tap_t[4], tap_t[5]) if tap_t is not None else (None, None)
        cols = _SwtLevel.apply(lines, taps[4], taps[5], dilation, scale, *zt)
    else:
        cols = _level_fwd(lines, taps[4], taps[5], dilation, scale)
    # [B, axis -1 band, axis -2 band, H, W, depth band, Dz] -> [B, 4 depth + 2 (axis -2) + (axis -1), Dz, H, W]
    return cols.reshape(b, 2, 2, h, w, 2, dz).permute(0, 5, 2, 1, 6, 3, 4).reshape(b, 8, dz, h, w)


def _composed3_inv(bands: Sequence[torch.Tensor], taps: Taps6, dilation: int, scale: float, tap_t=None) -> torch.Tensor:
    """V_cb = S_depth(band_a,cb, band_d,cb) from the 1-D synthesis level op on permuted copies, then the 2-D synthesis level of the four
    V on every depth slice."""
    b, dz, h, w = bands[0].shape
    diff = torch.is_grad_enabled() and (any(t.requires_grad for t in bands) or tap_t is not None)
    lows = torch.stack(tuple(bands[:4])).permute(0, 1, 3, 4, 2).reshape(4 * b * h * w, dz)
    highs = torch.stack(tuple(bands[4:])).permute(0, 1, 3, 4, 2).reshape(4 * b * h * w, dz)
    if diff:
        zt = (tap_t[4], tap_t[5]) if tap_t is not None else (None, None)
        v = _IswtLevel.apply(lows, highs, taps[4], taps[5], dilation, 1.0, *zt)
    else:
        v = _level_inv(lows, highs, taps[4], taps[5], dilation, 1.0)
    v = v.reshape(4, b, h, w, dz).permute(0, 1, 4, 2, 3).reshape(4, b * dz, h, w)  # plane 2 [axis -2 high] + [axis -1 high]
    quad = (v[0], v[2], v[1], v[3])  # cA, cH (axis -2 high), cV (axis -1 high), cD as the 2-D level takes them
    if tap_t is not None:
        y = _composed2_inv(quad, taps[:4], dilation, scale, tuple(tap_t[:4]))
    elif diff:
        y = _Iswt2Level.apply(*quad, tuple(taps[:4]), dilation, scale)
    else:
        y = _level2_inv(quad, taps[:4], dilation, scale)
    return y.reshape(b, dz, h, w)


def _vols(t: torch.Tensor) -> torch.Tensor:
    return _engine._unit_last(t)  # [B, Dz, H, W] with contiguous samples (volume / slice / row strides free)


def _taps6_array(taps: Taps6):
    return _dbl_p6(*[ctypes.cast(_engine._taps_array(t), _dbl_p) for t in taps])


def _level3_fwd(x: torch.Tensor, taps: Taps6, dilation: int, scale: float, composed: bool = False) -> torch.Tensor:
    """x [B, Dz, H, W] -> level buffer [B, 8, Dz, H, W] (planes aaa .. ddd): the fused launch where it exists, else (or with
    ``composed``) the composed route.  No autograd."""
    _engine._require_gpu(x)
    b, dz, h, w = x.shape
    flen = len(taps[0])
    taps = _merged6(taps, dilation, dz, h, w)
    if composed or not _fused3("fwd", x.dtype, flen, b, dz, h, w, dilation):
        with torch.no_grad():
            return _composed3_fwd(x.detach(), taps, dilation, scale)
    x = _vols(x)
    buf = torch.empty((b, 8, dz, h, w), dtype=x.dtype, device=x.device)
    if buf.numel() == 0:
        return buf
    plane = dz * h * w * buf.element_size()
    _engine._enqueue(x, _swt3_entries().mifwt_swt3_fwd, _engine._DTYPE_IDS[x.dtype], flen, b, dz, h, w, dilation, x.data_ptr(),
                     x.stride(0), x.stride(1), x.stride(2), _vp8(*[buf.data_ptr() + q * plane for q in range(8)]),
                     _i64x8(*[8 * dz * h * w] * 8), _i64x8(*[h * w] * 8), _i64x8(*[w] * 8), _taps6_array(taps), scale)
    return buf


def _level3_inv(bands: Sequence[torch.Tensor], taps: Taps6, dilation: int, scale: float, composed: bool = False) -> torch.Tensor:
    """(aaa, .., ddd), each [B, Dz, H, W] with any volume / slice / row strides -> y [B, Dz, H, W].  No autograd."""
    _engine._require_gpu(bands[0])
    b, dz, h, w = bands[0].shape
    flen = len(taps[0])
    taps = _merged6(taps, dilation, dz, h, w)
    if composed or not _fused3("inv", bands[0].dtype, flen, b, dz, h, w, dilation):
        with torch.no_grad():
            return _composed3_inv([t.detach() for t in bands], taps, dilation, scale)
    bands = [_vols(t) for t in bands]
    y = torch.empty((b, dz, h, w), dtype=bands[0].dtype, device=bands[0].device)
    if y.numel() == 0:
        return y
    _engine._enqueue(y, _swt3_entries().mifwt_swt3_inv, _engine._DTYPE_IDS[y.dtype], flen, b, dz, h, w, dilation,
                     _vp8(*[t.data_ptr() for t in bands]), _i64x8(*[t.stride(0) for t in bands]), _i64x8(*[t.stride(1) for t in bands]),
                     _i64x8(*[t.stride(2) for t in bands]), y.data_ptr(), dz * h * w, h * w, w, _taps6_array(taps), scale)
    return y


def swt3_plan(dtype: torch.dtype, flen: int, inverse: bool, b: int, dz: int, h: int, w: int, dilation: int) -> Optional[dict]:
    """The work split ``mifwt_swt3_plan`` reports for a fused 3-D level (host code, no launch), or None where there is no fused launch."""
    out = (ctypes.c_int * SWT3_PLAN_INTS)()
    n = _swt3_entries().mifwt_swt3_plan(_engine._DTYPE_IDS[dtype], flen, int(inverse), b, dz, h, w, dilation, out, SWT3_PLAN_INTS)
    if n != SWT3_PLAN_INTS:
        return None
    names = ("slice_residues", "row_residues", "segments", "segment_length", "row_tiles", "strips", "RT", "RW", "E", "lds_bytes", "threads")
    return dict(zip(names, (int(v) for v in out)))


class _Swt3Level(torch.autograd.Function):
    """One 3-D analysis level with host taps and a free scale.  Its transpose is the synthesis level with all six filters reversed and
    the same scale (and vice versa), so each Function's backward is the other Function: data gradients of any order."""

    @staticmethod
    def forward(ctx, x, taps, dilation, scale):
        ctx.meta = (taps, dilation, scale)
        return _level3_fwd(x, taps, dilation, scale)

    @staticmethod
    def backward(ctx, g_buf):
        taps, dilation, scale = ctx.meta
        return _Iswt3Level.apply(*(g_buf[:, q] for q in range(8)), _rev4(taps), dilation, scale), None, None, None


class _Iswt3Level(torch.autograd.Function):
    @staticmethod
    def forward(ctx, c0, c1, c2, c3, c4, c5, c6, c7, taps, dilation, scale):
        ctx.meta = (taps, dilation, scale)
        return _level3_inv((c0, c1, c2, c3, c4, c5, c6, c7), taps, dilation, scale)

    @staticmethod
    def backward(ctx, g_y):
        taps, dilation, scale = ctx.meta
        g = _Swt3Level.apply(g_y, _rev4(taps), dilation, scale)
        return (*(g[:, q] for q in range(8)), None, None, None)


def swt3(data: torch.Tensor, wavelet: Union[Wavelet, str], level: Optional[int] = None, *,
         axes: Tuple[int, int, int] = (-3, -2, -1)) -> WaveletCoeffNd:
    """Multi-level 3-D stationary transform over ``axes``.  Returns ``[cA_n, {"aad": .., "ada": .., "add": .., "daa": .., "dad": ..,
    "dda": .., "ddd": ..}_n, ..., {...}_1]``, every tensor of the input's shape: the container of ``wavedec3``, the first letter of a
    key belonging to ``axes[0]`` (``a`` low-pass, ``d`` high-pass).  By construction this is ``pywt.swtn(..., trim_approx=True,
    norm=False)`` over the three axes.

    A level is the level of :func:`swt` (periodic, dilation ``2^level index``, scale 1) along each of the three axes.  ``level=None``
    means the minimum of ``swt_max_level`` over the three extents — odd extents give ``[data]``; as in :func:`swt` no level is refused,
    the periodic index map wraps as often as needed.  Only float32 and float64 are accepted: float16 / bfloat16 raise ``ValueError("Input dtype
    ... not supported")`` even inside ``half_storage()`` (the fused kernels have no 16-bit form).  Differentiable w.r.t. the data to
    any order; a learnable (tensor-valued) filter bank runs on the composed route and has tap gradients up to second order."""
    axes = _fwt._ensure_axes(axes, 3)
    layout = _fwt._Layout(data, 3, axes)
    _check_dtype2(data)
    x = layout.fold(data)
    dec_lo, dec_hi, _, _ = host_taps(wavelet)
    tap_t = _fwt._tap_tensors(wavelet)
    if level is None:
        level = min(swt_max_level(n) for n in x.shape[-3:])
    taps = (tuple(dec_lo), tuple(dec_hi)) * 3
    out: list = []
    cur = x
    for lvl in range(level):
        _engine._require_gpu(cur)
        if tap_t is not None:
            buf = _composed3_fwd(cur, taps, 2 ** lvl, 1.0, (tap_t[0], tap_t[1]) * 3)
        elif torch.is_grad_enabled() and cur.requires_grad:
            buf = _Swt3Level.apply(cur, taps, 2 ** lvl, 1.0)
        else:
            buf = _level3_fwd(cur, taps, 2 ** lvl, 1.0)
        out.append({key: layout.unfold(buf[:, q + 1]) for q, key in enumerate(_KEYS3)})
        cur = buf[:, 0]
    out.append(layout.unfold(cur))
    out.reverse()
    return out


def iswt3(coeffs: WaveletCoeffNd, wavelet: Union[Wavelet, str], *, axes: Tuple[int, int, int] = (-3, -2, -1)) -> torch.Tensor:
    """Inverse of :func:`swt3` (by construction ``pywt.iswtn`` of coefficients with ``trim_approx=True, norm=False``).  Per level the
    synthesis level of :func:`iswt` (scale 1/2 per axis, 1/8 in all) along ``axes[2]``, ``axes[1]`` and ``axes[0]``: a linear map of ANY
    coefficient set, not only of images of ``swt3``.  float32 / float64 only, as :func:`swt3`."""
    coeffs = list(coeffs)
    if not coeffs or not isinstance(coeffs[0], torch.Tensor):
        raise ValueError("First element of coeffs must be the approximation coefficient tensor.")
    axes = _fwt._ensure_axes(axes, 3)
    layout = _fwt._Layout(coeffs[0], 3, axes)
    flat = [coeffs[0]]
    for c in coeffs[1:]:
        if not isinstance(c, dict) or set(c.keys()) != set(_KEYS3):
            raise ValueError(f"Unexpected detail coefficient type: {type(c)}. Detail coefficients must be a dict of tensors with the "
                             f"seven keys {', '.join(_KEYS3)} as returned by swt3.")
        for key in _KEYS3:
            if not isinstance(c[key], torch.Tensor):
                raise ValueError(f"Unexpected input type {type(c[key])}")
            flat.append(c[key])
    _fwt._check_same_device_dtype(flat)
    _check_dtype2(coeffs[0])
    _, _, rec_lo, rec_hi = host_taps(wavelet)
    tap_t = _fwt._tap_tensors(wavelet)
    taps = (tuple(rec_lo), tuple(rec_hi)) * 3
    cur = layout.fold(coeffs[0])
    details = [tuple(layout.fold(c[key]) for key in _KEYS3) for c in coeffs[1:]]
    for det in details:
        for t in det:
            if t.shape != cur.shape:
                raise ValueError(f"detail coefficients of shape {tuple(t.shape)} do not match the approximation of shape "
                                 f"{tuple(cur.shape)} (folded to [batch, D, H, W])")
    for pos, det in enumerate(details):
        dilation = 2 ** (len(details) - pos - 1)
        bands = (cur, *det)
        _engine._require_gpu(cur)
        if tap_t is not None:
            cur = _composed3_inv(bands, taps, dilation, 0.125, (tap_t[2], tap_t[3]) * 3)
        elif torch.is_grad_enabled() and any(t.requires_grad for t in bands):
            cur = _Iswt3Level.apply(*bands, taps, dilation, 0.125)
        else:
            cur = _level3_inv(bands, taps, dilation, 0.125)
    return layout.unfold(cur)
