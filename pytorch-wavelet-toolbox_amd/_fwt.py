"""Host side of the padded-convolution FWT: one N-D implementation behind the ten ptwt entry points.

What the reference spreads over conv_transform{,_2,_3}.py and separable_conv_transform.py is a single
level loop here, parameterised by the number of transformed axes; every level is one call into
``libmifwt.so`` (:mod:`._engine`).  This module restates only the thin glue: argument checks and their
error types, moving the transformed axes last and folding the batch, default levels, the per-level
extent / trim arithmetic, and the return containers — so results, shapes, containers and errors match the
reference (citations inline; /root/reference = ptwt 1.0.2-dev).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _engine
from . import _wavelets
from ._wavelets import device_bank, dwtn_max_level, filter_length, host_taps
from .constants import WaveletDetailTuple2d, supported_dtypes

AxisHint = Union[int, Sequence[int], None]


# ------------------------------------------------------------------------------------------ autograd
def _rows_last(t: torch.Tensor, axis: int) -> torch.Tensor:
    """[B, e_0.., e_{n-1}] -> 2-D [rows, e_axis] with ``axis`` (0-based among the trailing dims) innermost."""
    t = t.movedim(1 + axis, -1)
    return t.reshape(-1, t.shape[-1])


def _band_index(ndim: int, axis: int, sigma: int, rest: int) -> int:
    """Band index of the level buffer: bit (ndim-1-a) <=> axis a high-pass; ``rest`` enumerates the other axes' bits in
    axis order (most significant first)."""
    s, r = 0, rest
    for a in reversed(range(ndim)):
        if a == axis:
            bit = sigma
        else:
            bit = r & 1
            r >>= 1
        s |= bit << (ndim - 1 - a)
    return s


def _analysis_tap_grads(x, g_buf, dec_lo, dec_hi, mode_id):
    """d loss / d (dec_lo, dec_hi) of one analysis level (float64 [L] each).  Along axis a the level is
    c[k] = sum_m h[m] z_ext[2k+1-m] with z = the input transformed over the OTHER axes (ordinary level calls with axis a
    folded into the batch); the reduction is ``mifwt_tap_correlate`` (reference: ATen conv backward w.r.t. the weight)."""
    nd = x.dim() - 1
    flen = len(dec_lo)
    g_lo = torch.zeros(flen, dtype=torch.float64, device=x.device)
    g_hi = torch.zeros_like(g_lo)
    eng = _engine.ENGINE
    if nd == 2 and _engine.outer_axis_supported(flen, x.dtype) and hasattr(eng, "tap_correlate_planes"):
        # Two axes, every operand in its NATURAL layout (round 6: the transposed copies in front of the row reductions were a third of
        # a training step).  Along the rows axis H: z = the level along W of every row (inner-axis kernel), reduced along H by the
        # column kernel; along W: z = the level along H (outer-axis kernel on its own), reduced along W by the row kernel.  The band
        # planes of g_buf are strided views, taken as they are.  Only where the outer-axis kernels serve the bank (length and type); every
        # other bank takes the per-axis loop below.
        B, H, W = x.shape
        xc = x if x.stride(-1) == 1 else x.contiguous()
        rows = xc.reshape(B * H, W)  # (a view of a dense input; a copy of a plane of a level buffer: the deeper levels, a quarter each)
        pb = eng.analysis(rows, dec_lo, dec_hi, mode_id).reshape(B, H, 2, -1)  # [B, H, (lo, hi along W), Mw]
        for r in range(2):
            z = pb[:, :, r]  # [B, H, Mw]
            for sigma, out in ((0, g_lo), (1, g_hi)):
                eng.tap_correlate_planes(0, g_buf[:, _band_index(2, 0, sigma, r)], z, flen, 1, -1, mode_id, out)
        for r, z in enumerate(eng.analysis_outer(xc, dec_lo, dec_hi, mode_id)):  # (lo, hi along H) [B, Mh, W]
            for sigma, out in ((0, g_lo), (1, g_hi)):
                eng.tap_correlate_planes(1, g_buf[:, _band_index(2, 1, sigma, r)], z, flen, 1, -1, mode_id, out)
        return g_lo, g_hi
    for a in range(nd):
        if nd == 1:
            parts = [x]  # [B, N]
        else:
            xa = x.movedim(1 + a, 1)  # [B, N_a, others..]
            flat = xa.reshape(-1, *xa.shape[2:])
            pb = eng.analysis(flat, dec_lo, dec_hi, mode_id)  # [B * N_a, 2^(nd-1), M_others..]
            pb = pb.reshape(xa.shape[0], xa.shape[1], *pb.shape[1:])  # [B, N_a, 2^(nd-1), M_others..]
            parts = [pb[:, :, r] for r in range(1 << (nd - 1))]  # each [B, N_a, M_others..]
        for r, z in enumerate(parts):
            z2 = _rows_last(z, 0) if nd > 1 else z
            for sigma, out in ((0, g_lo), (1, g_hi)):
                band = _band_index(nd, a, sigma, r)
                g2 = _rows_last(g_buf[:, band], a)
                eng.tap_correlate(g2, z2, flen, 1, -1, mode_id, out)
    return g_lo, g_hi


def _synthesis_tap_grads(g_y, approx, details, rec_lo, rec_hi):
    """d loss / d (rec_lo, rec_hi) of one synthesis level.  Along axis a: y[n] = sum_k u[k] g[n+L-2-2k] with u = the
    bands whose axis-a letter is lo / hi, synthesised over the OTHER axes."""
    nd = approx.dim() - 1
    flen = len(rec_lo)
    g_lo = torch.zeros(flen, dtype=torch.float64, device=g_y.device)
    g_hi = torch.zeros_like(g_lo)
    eng = _engine.ENGINE
    bands = [approx] + list(details)
    if nd == 2 and _engine.outer_axis_supported(flen, g_y.dtype) and hasattr(eng, "synthesis_outer"):
        # two axes, every operand in its natural layout (see _analysis_tap_grads).  Along H: u = the two bands with letter sigma along H
        # synthesised along W (inner-axis kernel, rows (b, k_h)), reduced along H by the column kernel; along W: u = the two bands with
        # letter sigma along W synthesised along H (outer-axis kernel), reduced along W by the row kernel.
        B, Ny, Nx = g_y.shape
        gyc = g_y if g_y.stride(-1) == 1 else g_y.contiguous()
        for sigma, out in ((0, g_lo), (1, g_hi)):
            lo_w, hi_w = bands[_band_index(2, 0, sigma, 0)], bands[_band_index(2, 0, sigma, 1)]  # [B, Mh, Mw]: low / high along W
            Mh, Mw = lo_w.shape[1:]
            u = eng.synthesis(lo_w.reshape(B * Mh, Mw), [hi_w.reshape(B * Mh, Mw)], rec_lo, rec_hi, [Nx]).reshape(B, Mh, Nx)
            eng.tap_correlate_planes(0, u, gyc, flen, -(flen - 2), 1, 0, out)
            lo_h, hi_h = bands[_band_index(2, 1, sigma, 0)], bands[_band_index(2, 1, sigma, 1)]  # low / high along H
            u = eng.synthesis_outer(lo_h, hi_h, rec_lo, rec_hi, Ny)  # [B, Ny, Mw]
            eng.tap_correlate_planes(1, u, gyc, flen, -(flen - 2), 1, 0, out)
        return g_lo, g_hi
    for a in range(nd):
        gy2 = _rows_last(g_y, a)
        for sigma, out in ((0, g_lo), (1, g_hi)):
            if nd == 1:
                u2 = bands[sigma]
            else:
                sel = [bands[_band_index(nd, a, sigma, r)].movedim(1 + a, 1) for r in range(1 << (nd - 1))]  # [B, M_a, M_others..]
                flat = [t.reshape(-1, *t.shape[2:]).contiguous() for t in sel]
                out_ext = [g_y.shape[1 + o] for o in range(nd) if o != a]
                u = eng.synthesis(flat[0], flat[1:], rec_lo, rec_hi, out_ext)  # [B * M_a, N_others..]
                u = u.reshape(sel[0].shape[0], sel[0].shape[1], *u.shape[1:])  # [B, M_a, N_others..]
                u2 = _rows_last(u, 0)
            eng.tap_correlate(u2, gy2, flen, -(flen - 2), 1, 0, out)
    return g_lo, g_hi


# ---- learnable filter banks, gradients of any order -----------------------------------------------------------------------------------
# A level along ONE axis is bilinear in (signal, taps):  c = A(h) x.  Three maps close that under differentiation, each a differentiable
# op whose backward is made of the other two:
#     A(h) x            (_Axis1)      d/dx: A(h)^T g              d/dh: C(x, g)
#     A(h)^T g          (_Axis1Adj)   d/dg: A(h) gg               d/dh: C(gg, g)
#     C(x, g) = t       (_Axis1Corr)  d/dx: A(w)^T g              d/dg: A(w) x          (w = the gradient that arrives for t: taps!)
# and likewise for the synthesis  y = S(r) (a, d)  (_Syn1, _Syn1Adj, _Syn1Corr).  An N-D level is a product of such maps, one per axis,
# so autograd through their composition yields every mixed derivative the reference gets from plain ATen ops (src/ptwt/_util.py:115-132
# keeps the taps in the graph).  The fused level kernels serve the forward and the first-order backward as before; only a backward
# that is asked for a graph (create_graph=True) with a learnable filter bank re-runs the level through these ops.  Taps travel to the
# kernels as host floats (one device-to-host copy per op).
def _host_floats_of(t: torch.Tensor) -> List[float]:
    """Host copy of a filter tensor (the stationary-transform kernels take their taps in the launch arguments)."""
    return [float(v) for v in t.detach().double().cpu().reshape(-1).tolist()]


def _host_taps_of(t: torch.Tensor, device: Optional[torch.device] = None):
    """The taps of a filter tensor for a level call on data that lives on ``device``: the tensor itself (kernels read device memory) when
    it lives on THAT GPU and device taps are not switched off, else host floats (one device-to-host copy) — a kernel launched on cuda:1
    must not be handed a raw cuda:0 pointer."""
    if t.is_cuda and _wavelets._device_taps_mode != "never" and (device is None or t.device == device):
        return _engine.DevTaps(t)
    return [float(v) for v in t.detach().double().cpu().reshape(-1).tolist()]


def _tap_pair(needed: bool, corr, lo_t: torch.Tensor, hi_t: torch.Tensor, *args):
    """The tap gradients of a per-axis op's backward: ``corr.apply(*args)`` (float64 [L] each) cast like the tap tensors, or
    ``(None, None)`` when neither is asked for."""
    if not needed:
        return None, None
    t_lo, t_hi = corr.apply(*args)
    return _like(t_lo, lo_t), _like(t_hi, hi_t)


class _Axis1(torch.autograd.Function):
    """rows [R, N] -> [R, 2, M]: one analysis level along the last axis, taps as tensors."""

    @staticmethod
    def forward(ctx, x, lo_t, hi_t, mode_id):
        ctx.mode_id = mode_id
        ctx.save_for_backward(x, lo_t, hi_t)
        return _engine.ENGINE.analysis(x, _host_taps_of(lo_t, x.device), _host_taps_of(hi_t, x.device), mode_id)

    @staticmethod
    def backward(ctx, g):
        x, lo_t, hi_t = ctx.saved_tensors
        g_x = _Axis1Adj.apply(g, lo_t, hi_t, ctx.mode_id, x.shape[1]) if ctx.needs_input_grad[0] else None
        t_lo, t_hi = _tap_pair(ctx.needs_input_grad[1] or ctx.needs_input_grad[2], _Axis1Corr, lo_t, hi_t, x, g, lo_t.numel(), ctx.mode_id)
        return g_x, t_lo, t_hi, None


class _Axis1Adj(torch.autograd.Function):
    """[R, 2, M] -> rows [R, N]: the transpose of :class:`_Axis1`."""

    @staticmethod
    def forward(ctx, g, lo_t, hi_t, mode_id, n):
        ctx.mode_id = mode_id
        ctx.save_for_backward(g, lo_t, hi_t)
        return _engine.ENGINE.analysis_adjoint(g, (n,), _host_taps_of(lo_t, g.device), _host_taps_of(hi_t, g.device), mode_id)

    @staticmethod
    def backward(ctx, gg):
        g, lo_t, hi_t = ctx.saved_tensors
        g_g = _Axis1.apply(gg, lo_t, hi_t, ctx.mode_id) if ctx.needs_input_grad[0] else None
        # <gg, A(h)^T g> = <A(h) gg, g>
        t_lo, t_hi = _tap_pair(ctx.needs_input_grad[1] or ctx.needs_input_grad[2], _Axis1Corr, lo_t, hi_t, gg, g, lo_t.numel(), ctx.mode_id)
        return g_g, t_lo, t_hi, None, None


class _Axis1Corr(torch.autograd.Function):
    """(rows x [R, N], g [R, 2, M]) -> (t_lo, t_hi) float64 [L]:  t_b[m] = sum_{row, k} g_b[row, k] x_ext[row, 2 k + 1 - m]."""

    @staticmethod
    def forward(ctx, x, g, flen, mode_id):
        ctx.mode_id = mode_id
        ctx.save_for_backward(x, g)
        t_lo = torch.zeros(flen, dtype=torch.float64, device=x.device)
        t_hi = torch.zeros_like(t_lo)
        _engine.ENGINE.tap_correlate(g[:, 0], x, flen, 1, -1, mode_id, t_lo)
        _engine.ENGINE.tap_correlate(g[:, 1], x, flen, 1, -1, mode_id, t_hi)
        return t_lo, t_hi

    @staticmethod
    def backward(ctx, w_lo, w_hi):
        x, g = ctx.saved_tensors
        w_lo, w_hi = w_lo.to(x.dtype), w_hi.to(x.dtype)
        g_x = _Axis1Adj.apply(g, w_lo, w_hi, ctx.mode_id, x.shape[1]) if ctx.needs_input_grad[0] else None
        g_g = _Axis1.apply(x, w_lo, w_hi, ctx.mode_id) if ctx.needs_input_grad[1] else None
        return g_x, g_g, None, None


class _Syn1(torch.autograd.Function):
    """(a, d [R, M]) -> y [R, n_out]: one synthesis level along the last axis (cropped to n_out), taps as tensors."""

    @staticmethod
    def forward(ctx, a, d, lo_t, hi_t, n_out):
        ctx.save_for_backward(a, d, lo_t, hi_t)
        return _engine.ENGINE.synthesis(a, [d], _host_taps_of(lo_t, a.device), _host_taps_of(hi_t, a.device), [n_out])

    @staticmethod
    def backward(ctx, g_y):
        a, d, lo_t, hi_t = ctx.saved_tensors
        g_a = g_d = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gb = _Syn1Adj.apply(g_y, lo_t, hi_t, a.shape[1])
            g_a, g_d = gb[:, 0], gb[:, 1]
        t_lo, t_hi = _tap_pair(ctx.needs_input_grad[2] or ctx.needs_input_grad[3], _Syn1Corr, lo_t, hi_t, a, d, g_y, lo_t.numel())
        return g_a, g_d, t_lo, t_hi, None


class _Syn1Adj(torch.autograd.Function):
    """g_y [R, n_out] -> [R, 2, M]: the transpose of :class:`_Syn1`."""

    @staticmethod
    def forward(ctx, g_y, lo_t, hi_t, m):
        ctx.save_for_backward(g_y, lo_t, hi_t)
        return _engine.ENGINE.synthesis_adjoint(g_y, (m,), _host_taps_of(lo_t, g_y.device), _host_taps_of(hi_t, g_y.device))

    @staticmethod
    def backward(ctx, gg):
        g_y, lo_t, hi_t = ctx.saved_tensors
        g_gy = _Syn1.apply(gg[:, 0], gg[:, 1], lo_t, hi_t, g_y.shape[1]) if ctx.needs_input_grad[0] else None
        # <gg, S(r)^T g_y> = <S(r) gg, g_y>
        t_lo, t_hi = _tap_pair(ctx.needs_input_grad[1] or ctx.needs_input_grad[2], _Syn1Corr, lo_t, hi_t, gg[:, 0], gg[:, 1], g_y, lo_t.numel())
        return g_gy, t_lo, t_hi, None


class _Syn1Corr(torch.autograd.Function):
    """(a, d [R, M], g_y [R, n_out]) -> (t_lo, t_hi) float64 [L]:  t_lo[j] = sum_{row, k} a[row, k] g_y[row, 2 k - (L - 2) + j] (zeros outside)."""

    @staticmethod
    def forward(ctx, a, d, g_y, flen):
        ctx.save_for_backward(a, d, g_y)
        t_lo = torch.zeros(flen, dtype=torch.float64, device=a.device)
        t_hi = torch.zeros_like(t_lo)
        _engine.ENGINE.tap_correlate(a, g_y, flen, -(flen - 2), 1, 0, t_lo)
        _engine.ENGINE.tap_correlate(d, g_y, flen, -(flen - 2), 1, 0, t_hi)
        return t_lo, t_hi

    @staticmethod
    def backward(ctx, w_lo, w_hi):
        a, d, g_y = ctx.saved_tensors
        w_lo, w_hi = w_lo.to(a.dtype), w_hi.to(a.dtype)
        g_a = g_d = g_gy = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            gb = _Syn1Adj.apply(g_y, w_lo, w_hi, a.shape[1])
            g_a, g_d = gb[:, 0], gb[:, 1]
        if ctx.needs_input_grad[2]:
            g_gy = _Syn1.apply(a, d, w_lo, w_hi, g_y.shape[1])
        return g_a, g_d, g_gy, None


def _analysis_level_closed(x: torch.Tensor, lo_t: torch.Tensor, hi_t: torch.Tensor, mode_id: int) -> torch.Tensor:
    """One N-D analysis level [B, N..] -> [B, 2^n, M..] as a product of :class:`_Axis1` ops (last axis first): differentiable to any
    order w.r.t. the data and the taps."""
    nd = x.dim() - 1
    bands = {0: x}
    for a in reversed(range(nd)):
        bit = 1 << (nd - 1 - a)
        nxt = {}
        for s, t in bands.items():
            tt = t.movedim(1 + a, -1)
            out = _Axis1.apply(tt.reshape(-1, tt.shape[-1]), lo_t, hi_t, mode_id)  # [rows, 2, M]
            for sigma in (0, 1):
                nxt[s | (bit * sigma)] = out[:, sigma].reshape(*tt.shape[:-1], out.shape[-1]).movedim(-1, 1 + a)
        bands = nxt
    return torch.stack([bands[s] for s in range(1 << nd)], dim=1)


def _synthesis_level_closed(approx: torch.Tensor, details: Sequence[torch.Tensor], lo_t: torch.Tensor, hi_t: torch.Tensor,
                            out_ext: Sequence[int]) -> torch.Tensor:
    """One N-D synthesis level (bands [B, M..] in band order -> [B, *out_ext]) as a product of :class:`_Syn1` ops (first axis first)."""
    nd = approx.dim() - 1
    bands = {s: t for s, t in enumerate([approx, *details])}
    for a in range(nd):
        bit = 1 << (nd - 1 - a)
        nxt = {}
        for s, t in bands.items():
            if s & bit:
                continue
            lo, hi = t.movedim(1 + a, -1), bands[s | bit].movedim(1 + a, -1)
            y = _Syn1.apply(lo.reshape(-1, lo.shape[-1]), hi.reshape(-1, hi.shape[-1]), lo_t, hi_t, int(out_ext[a]))
            nxt[s] = y.reshape(*lo.shape[:-1], y.shape[-1]).movedim(-1, 1 + a)
        bands = nxt
    return bands[0]


def _partials_at(values, build, cotangent, weights):
    """Second-order partial derivatives by automatic differentiation AT DETACHED COPIES: ``values`` are the op's inputs, ``build``
    maps fresh leaves holding their values to the level's output, ``cotangent`` (one of the leaves' positions, see callers) is the
    upstream gradient.  Returns d/d(leaf) of  sum_i <weights_i, d <output, cotangent> / d leaf_i>  for every leaf: the derivatives of
    the first-order gradients (as a vector-Jacobian product with ``weights``) w.r.t. every input of the op, each a PARTIAL derivative —
    the leaves have no history, so nothing upstream is counted twice."""
    leaves = [v.detach().clone().requires_grad_(True) for v in values]
    with torch.enable_grad():
        out = build(leaves)
        first = torch.autograd.grad(out, leaves[1:], leaves[0], create_graph=True, allow_unused=True)  # (leaves[0] = the cotangent)
        s = None
        for f, w in zip(first, weights):
            if f is not None and w is not None:
                term = (f * w.to(f.dtype)).sum()
                s = term if s is None else s + term
        if s is None:
            return [None] * len(leaves)
        return list(torch.autograd.grad(s, leaves, allow_unused=True))


def _third_order_refused(taps) -> None:
    if torch.is_grad_enabled() and any(t.requires_grad for t in taps):
        raise RuntimeError("ptwt_amd: derivatives beyond second order through a learnable filter bank are not supported "
                           "(create_graph=True inside a double backward); first and second order are.")


class _AnalysisLevelGrad(torch.autograd.Function):
    """(g_buf, x, dec taps) -> (g_x, g_lo, g_hi): the first-order gradients of one analysis level, from the fused kernels as in
    :class:`_AnalysisLevel`, as an op of its own so that a double backward (create_graph=True) with a LEARNABLE filter bank gets the
    mixed second derivatives: its backward differentiates the level — rebuilt from the per-axis ops that are closed under
    differentiation (:func:`_analysis_level_closed`) — twice at detached copies of the inputs.  The reference has these terms from
    ATen's conv / pad backward (src/ptwt/_util.py:115-132 keeps the taps in the graph)."""

    @staticmethod
    def forward(ctx, g_buf, x, lo_t, hi_t, dec_lo, dec_hi, mode_id):
        ctx.mode_id = mode_id
        ctx.save_for_backward(g_buf, x, lo_t, hi_t)
        g_x = _engine.ENGINE.analysis_adjoint(g_buf, tuple(x.shape[1:]), dec_lo, dec_hi, mode_id)
        g_lo, g_hi = _analysis_tap_grads(x, g_buf, dec_lo, dec_hi, mode_id)
        return g_x, _like(g_lo, lo_t), _like(g_hi, hi_t)

    @staticmethod
    def backward(ctx, w_x, w_lo, w_hi):
        g_buf, x, lo_t, hi_t = ctx.saved_tensors
        _third_order_refused((lo_t, hi_t))
        mode_id = ctx.mode_id
        d = _partials_at([g_buf, x, lo_t, hi_t], lambda lv: _analysis_level_closed(lv[1], lv[2], lv[3], mode_id), 0, [w_x, w_lo, w_hi])
        return d[0], d[1], d[2], d[3], None, None, None


class _SynthesisLevelGrad(torch.autograd.Function):
    """(g_y, rec taps, approx, details) -> (g_lo, g_hi, g_approx, g_details...): the first-order gradients of one synthesis level (fused
    kernels) as an op whose backward has the mixed second derivatives with a learnable filter bank (see :class:`_AnalysisLevelGrad`)."""

    @staticmethod
    def forward(ctx, g_y, lo_t, hi_t, rec_lo, rec_hi, approx, *details):
        ctx.save_for_backward(g_y, lo_t, hi_t, approx, *details)
        g = _engine.ENGINE.synthesis_adjoint(g_y, tuple(approx.shape[1:]), rec_lo, rec_hi)
        g_lo, g_hi = _synthesis_tap_grads(g_y, approx, details, rec_lo, rec_hi)
        return (_like(g_lo, lo_t), _like(g_hi, hi_t), *[g[:, s] for s in range(len(details) + 1)])

    @staticmethod
    def backward(ctx, w_lo, w_hi, *w_bands):
        g_y, lo_t, hi_t, approx, *details = ctx.saved_tensors
        _third_order_refused((lo_t, hi_t))
        out_ext = tuple(g_y.shape[1:])
        d = _partials_at([g_y, lo_t, hi_t, approx, *details], lambda lv: _synthesis_level_closed(lv[3], lv[4:], lv[1], lv[2], out_ext), 0,
                         [w_lo, w_hi, *w_bands])
        return (d[0], d[1], d[2], None, None, *d[3:])


def _like(grad64: torch.Tensor, ref: Optional[torch.Tensor]):
    return None if ref is None else grad64.to(device=ref.device, dtype=ref.dtype).reshape(ref.shape)


class _AnalysisLevel(torch.autograd.Function):
    """One analysis level as a differentiable op w.r.t. its input and (optionally) the dec taps.  The reference is
    differentiable because it is built from ATen ops (F.pad + F.conv*d, src/ptwt/conv_transform.py:135-139 and the
    2-D / 3-D twins); here the backward is the explicit adjoint kernel (C ABI ``mifwt_dwt_fwd_adjoint``) and, for
    learnable filter banks, the tap correlation (``mifwt_tap_correlate``).  ``lo_t`` / ``hi_t`` are the tap TENSORS (or
    None): they only tie the op into the graph, the kernels take the host copies ``dec_lo`` / ``dec_hi``."""

    @staticmethod
    def forward(ctx, x, dec_lo, dec_hi, mode_id, lo_t=None, hi_t=None):
        ctx.meta = (tuple(x.shape[1:]), dec_lo, dec_hi, mode_id)
        ctx.taps = (lo_t, hi_t)
        need_taps = any(t is not None and t.requires_grad for t in (lo_t, hi_t))
        ctx.save_for_backward(x if need_taps else None)
        return _engine.ENGINE.analysis(x, dec_lo, dec_hi, mode_id)

    @staticmethod
    def backward(ctx, g_buf):
        sig_shape, dec_lo, dec_hi, mode_id = ctx.meta
        (x,) = ctx.saved_tensors
        if x is not None and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ctx.taps):
            # a graph of this backward is wanted (create_graph=True) and the filter bank is learnable: the same first-order gradients as
            # an op whose own backward has the mixed second derivatives (data x taps, taps x taps, upstream gradient x taps)
            lo_t, hi_t = ctx.taps
            g_x, g_lo, g_hi = _AnalysisLevelGrad.apply(g_buf, x, lo_t, hi_t, dec_lo, dec_hi, mode_id)
            return (g_x if ctx.needs_input_grad[0] else None, None, None, None,
                    g_lo if ctx.needs_input_grad[4] else None, g_hi if ctx.needs_input_grad[5] else None)
        # the adjoint is itself a differentiable level op (its derivative is this level again): gradients of any order w.r.t.
        # the data, as the reference has them from plain F.pad + conv.  (The tap gradients below are first order only.)
        g_x = _AnalysisAdjointLevel.apply(g_buf, sig_shape, dec_lo, dec_hi, mode_id) if ctx.needs_input_grad[0] else None
        g_lo = g_hi = None
        if x is not None and (ctx.needs_input_grad[4] or ctx.needs_input_grad[5]):
            g_lo, g_hi = _analysis_tap_grads(x, g_buf.detach(), dec_lo, dec_hi, mode_id)
            g_lo, g_hi = _like(g_lo, ctx.taps[0]), _like(g_hi, ctx.taps[1])
        return g_x, None, None, None, g_lo, g_hi


class _AnalysisAdjointLevel(torch.autograd.Function):
    """The transpose of one analysis level, ``g_buf`` [B, 2^n, M..] -> ``g_x`` [B, N..] (C ABI ``mifwt_dwt_fwd_adjoint``) — linear, so
    its own backward is the analysis level."""

    @staticmethod
    def forward(ctx, g_buf, sig_shape, dec_lo, dec_hi, mode_id):
        ctx.meta = (dec_lo, dec_hi, mode_id)
        return _engine.ENGINE.analysis_adjoint(g_buf, sig_shape, dec_lo, dec_hi, mode_id)

    @staticmethod
    def backward(ctx, gg_x):
        dec_lo, dec_hi, mode_id = ctx.meta
        return _AnalysisLevel.apply(gg_x, dec_lo, dec_hi, mode_id, None, None), None, None, None, None


class _AnalysisAdjointBands(torch.autograd.Function):
    """:class:`_AnalysisAdjointLevel` with the gradient of every band in a tensor of its own (no concatenation: the C ABI takes a
    pointer per band); linear as well, its backward is the analysis level."""

    @staticmethod
    def forward(ctx, sig_shape, dec_lo, dec_hi, mode_id, g_approx, *g_details):
        ctx.meta = (dec_lo, dec_hi, mode_id, len(g_details))
        return _engine.ENGINE.analysis_adjoint_bands(g_approx, g_details, sig_shape, dec_lo, dec_hi, mode_id)

    @staticmethod
    def backward(ctx, gg_x):
        dec_lo, dec_hi, mode_id, ndet = ctx.meta
        buf = _AnalysisLevel.apply(gg_x, dec_lo, dec_hi, mode_id, None, None)
        return (None, None, None, None) + tuple(buf[:, s] for s in range(ndet + 1))


def _chained_analysis_adjoint(meta, g, g_bands):
    """Backward of a multi-level analysis launch, level by level from the coarsest: ``g`` = the gradient of the last level's
    approximation, ``g_bands`` = those of the detail bands (as many per level as the launch has), finest level first; ``meta`` = (input
    shape per level, dec taps, mode).  Each step is a differentiable op in turn (gradients of any order)."""
    shapes, dec_lo, dec_hi, mode_id = meta
    ndet = len(g_bands) // len(shapes)
    for lvl in range(len(shapes) - 1, -1, -1):
        g = _AnalysisAdjointBands.apply(shapes[lvl], dec_lo, dec_hi, mode_id, g, *g_bands[ndet * lvl : ndet * lvl + ndet])
    return g


class _AnalysisPyramid(torch.autograd.Function):
    """Several 2-D analysis levels in ONE launch as a differentiable op w.r.t. the data (C ABI ``mifwt_dwt2_fwd_pyramid``: the streaming
    three-level kernel / the small-plane kernel; src/ptwt/conv_transform_2.py:142-149 per trip): the forward of a call that asks for
    gradients runs on the same fused kernels as one that does not, and saves nothing.  The outputs are the BANDS (views of the level
    buffers): the approximation of the last fused level, then (ad, da, dd) per level, finest first — autograd hands the backward one
    gradient per band, no buffer is assembled.  The backward composes the per-level adjoints coarse to fine (each a differentiable op in
    turn: gradients of any order)."""

    @staticmethod
    def forward(ctx, x, dec_lo, dec_hi, mode_id, want):
        bufs = _engine.ENGINE.analysis_pyramid(x, dec_lo, dec_hi, mode_id, want)
        shapes, n = [], list(x.shape[1:])
        out = [bufs[-1][:, 0]]
        for b in bufs:
            shapes.append(tuple(n))
            n = list(b.shape[2:])
            out.extend(b.unbind(1)[-3:])
        ctx.meta = (shapes, dec_lo, dec_hi, mode_id)
        return tuple(out)

    @staticmethod
    def backward(ctx, g_approx, *g_bands):
        shapes, dec_lo, dec_hi, mode_id = ctx.meta
        if mode_id == _engine.MODE_IDS["zero"] and not torch.is_grad_enabled():
            # zero mode, no graph of the backward wanted: the adjoint of every level is a synthesis level with the dec taps reversed,
            # so the adjoint of the whole launch is ONE multi-level synthesis launch (kernels 22 / 21) where the library serves it
            levels = [list(g_bands[3 * lvl : 3 * lvl + 3]) for lvl in range(len(shapes) - 1, -1, -1)]  # coarsest first
            g = _engine.ENGINE.synthesis_pyramid(g_approx if g_approx.stride(-1) == 1 else g_approx.contiguous(), levels, dec_lo[::-1], dec_hi[::-1],
                                                 list(shapes[0]))
            if g is not None:
                return g, None, None, None, None
        return _chained_analysis_adjoint(ctx.meta, g_approx, g_bands), None, None, None, None


class _FusedRouteUnavailable(Exception):
    """Raised inside the forward of a multi-level autograd op when the library turns the launch down after all; the caller goes level
    by level."""


class _AnalysisTail(torch.autograd.Function):
    """Several 1-D analysis levels in one launch (C ABI ``mifwt_dwt1_fwd_long`` / ``mifwt_dwt1_fwd_tail``; src/ptwt/conv_transform.py:133-140
    per trip) as a differentiable op w.r.t. the data: outputs = the last level's approximation, then the detail rows, finest first; the
    backward composes the per-level adjoints coarse to fine."""

    @staticmethod
    def forward(ctx, x, dec_lo, dec_hi, mode_id, want):
        bufs = _engine.ENGINE.analysis_tail(x, dec_lo, dec_hi, mode_id, want)
        if bufs is None:
            raise _FusedRouteUnavailable()
        shapes, n = [], int(x.shape[1])
        for b in bufs:
            shapes.append((n,))
            n = int(b.shape[2])
        ctx.meta = (shapes, dec_lo, dec_hi, mode_id)
        return (bufs[-1][:, 0], *[b[:, -1] for b in bufs])

    @staticmethod
    def backward(ctx, g_approx, *g_details):
        return _chained_analysis_adjoint(ctx.meta, g_approx, g_details), None, None, None, None


def _chained_synthesis_adjoint(meta, g_y, ndet: int, fused_launch):
    """Backward of a multi-level reconstruction w.r.t. its coefficients, level by level from the finest: ``meta`` = (rec taps, shape of
    the coefficients per level, coarsest first), ``ndet`` detail bands per level.  Returns (gradient of the coarsest approximation,
    [gradients of the detail bands, coarsest level first]).  Each step is :class:`_SynthesisAdjointLevel`, a differentiable op in turn.

    No graph of the backward wanted and host taps: the adjoint of a synthesis level is a zero-mode analysis level with the rec taps
    reversed, and a trimmed output sample is a zero the zero extension supplies anyway — so the adjoint of several levels is ONE
    multi-level analysis launch where the library serves it.  ``fused_launch(g, lo, hi, n)`` is that launch over up to ``n`` levels:
    level buffers like those of ``analysis_pyramid`` / ``analysis_tail``, or None (None in its place: there is no such launch)."""
    rec_lo, rec_hi, coef_shapes = meta
    flen = len(rec_lo)
    grads: list = []
    g = g_y
    todo = list(reversed(coef_shapes))  # finest level first
    fused = fused_launch is not None and not torch.is_grad_enabled() and not _engine._is_dev(rec_lo)
    while todo:
        bufs = None
        if fused and len(todo) >= 2:
            # what a zero-mode analysis of g yields level by level (floor((n + L - 1) / 2) per axis) against the coefficient shapes the
            # forward took: decided on the host BEFORE anything is launched — a chain with a crop the adjoint launch cannot express (a
            # separable crop of more than one sample) goes level by level from here on instead of launching, discarding and retrying
            ns, ok = [int(v) for v in g.shape[1:]], 0
            for shp in todo:
                ns = [(n + flen - 1) // 2 for n in ns]
                if tuple(ns) != tuple(shp):
                    break
                ok += 1
            if ok < 2:
                fused = False
            else:
                bufs = fused_launch(g if g.stride(-1) == 1 else g.contiguous(), list(rec_lo)[::-1], list(rec_hi)[::-1], ok)
                if bufs is not None and (len(bufs) < 2 or any(tuple(b.shape[2:]) != tuple(shp) for b, shp in zip(bufs, todo))):
                    bufs, fused = None, False
        if bufs is None:
            bufs = [_SynthesisAdjointLevel.apply(g, todo[0], rec_lo, rec_hi)]
        for b in bufs:  # (the detail bands are the last planes of a level buffer, the approximation of the last one its first)
            grads = list(b.unbind(1)[-ndet:]) + grads
        g = bufs[-1][:, 0]
        todo = todo[len(bufs):]
    return g, grads


class _SynthesisChain1d(torch.autograd.Function):
    """A whole 1-D reconstruction on the multi-level launches (``mifwt_dwt1_inv_tail`` for the coarse levels, ``mifwt_dwt1_inv_long`` for
    the fine ones; src/ptwt/conv_transform.py:184-199 per trip) as a differentiable op w.r.t. the coefficients; ``run`` does the launches
    (the caller's recursion over the two kernels), the backward composes the per-level synthesis adjoints fine to coarse."""

    @staticmethod
    def forward(ctx, run, rec_lo, rec_hi, approx, *dets):
        ctx.meta = (rec_lo, rec_hi, [tuple(d.shape[1:]) for d in dets])
        return run(approx, list(dets))

    @staticmethod
    def backward(ctx, g_y):
        zero = _engine.MODE_IDS["zero"]  # (kernels 17 / 14)
        g, grads = _chained_synthesis_adjoint(ctx.meta, g_y, 1, lambda g, lo, hi, n: _engine.ENGINE.analysis_tail(g, lo, hi, zero, n))
        return (None, None, None, g, *grads)


class _SynthesisLevel(torch.autograd.Function):
    """One synthesis level, differentiable w.r.t. the approximation, every detail band and (optionally) the rec taps
    (backward: ``mifwt_dwt_inv_adjoint`` + ``mifwt_tap_correlate``; reference: autograd through torch.stack +
    F.conv_transpose*d + crop)."""

    @staticmethod
    def forward(ctx, rec_lo, rec_hi, out_ext, lo_t, hi_t, approx, *details):
        ctx.meta = (tuple(approx.shape[1:]), rec_lo, rec_hi, len(details))
        ctx.taps = (lo_t, hi_t)
        need_taps = any(t is not None and t.requires_grad for t in (lo_t, hi_t))
        if need_taps:
            ctx.save_for_backward(approx, *details)
        else:
            ctx.save_for_backward()
        return _engine.ENGINE.synthesis(approx, list(details), rec_lo, rec_hi, out_ext)

    @staticmethod
    def backward(ctx, g_y):
        coef_shape, rec_lo, rec_hi, ndet = ctx.meta
        saved = ctx.saved_tensors
        if saved and torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ctx.taps):
            # create_graph=True with a learnable filter bank: first-order gradients as an op that carries the mixed second derivatives
            lo_t, hi_t = ctx.taps
            out = _SynthesisLevelGrad.apply(g_y, lo_t, hi_t, rec_lo, rec_hi, *saved)
            need = ctx.needs_input_grad
            return (None, None, None, out[0] if need[3] else None, out[1] if need[4] else None,
                    *[o if need[5 + i] else None for i, o in enumerate(out[2:])])
        g_bands = (None,) * (ndet + 1)
        if any(ctx.needs_input_grad[5:]):
            g = _SynthesisAdjointLevel.apply(g_y, coef_shape, rec_lo, rec_hi)  # differentiable in turn: any order w.r.t. the data
            g_bands = tuple(g[:, s] for s in range(ndet + 1))
        g_lo = g_hi = None
        if saved and (ctx.needs_input_grad[3] or ctx.needs_input_grad[4]):
            g_lo, g_hi = _synthesis_tap_grads(g_y.detach(), saved[0], saved[1:], rec_lo, rec_hi)
            g_lo, g_hi = _like(g_lo, ctx.taps[0]), _like(g_hi, ctx.taps[1])
        return (None, None, None, g_lo, g_hi) + g_bands


class _SynthesisAdjointLevel(torch.autograd.Function):
    """The transpose of one synthesis level, ``g_y`` [B, out..] -> [B, 2^n, M..] (C ABI ``mifwt_dwt_inv_adjoint``); its own backward is
    the synthesis level."""

    @staticmethod
    def forward(ctx, g_y, coef_shape, rec_lo, rec_hi):
        ctx.meta = (tuple(g_y.shape[1:]), rec_lo, rec_hi)
        return _engine.ENGINE.synthesis_adjoint(g_y, coef_shape, rec_lo, rec_hi)

    @staticmethod
    def backward(ctx, gg):
        out_ext, rec_lo, rec_hi = ctx.meta
        bands = [gg[:, s] for s in range(gg.shape[1])]
        return _SynthesisLevel.apply(rec_lo, rec_hi, out_ext, None, None, bands[0], *bands[1:]), None, None, None


class _SynthesisPyramid(torch.autograd.Function):
    """Several 2-D synthesis levels in ONE launch as a differentiable op w.r.t. the coefficients (C ABI ``mifwt_dwt2_inv_pyramid``: the
    streaming three-level kernel / the small-plane kernel; src/ptwt/conv_transform_2.py:222-249 per trip): a `waverec2` that asks for
    gradients runs its forward on the same fused kernels as one that does not.  ``dets`` = three detail bands per level, coarsest level
    first.  The backward composes the per-level synthesis adjoints (zero-mode analysis kernels) fine to coarse, each a differentiable
    op in turn."""

    @staticmethod
    def forward(ctx, rec_lo, rec_hi, out_ext, plan, nlev, approx, *dets):
        levels = [list(dets[3 * l : 3 * l + 3]) for l in range(nlev)]
        ctx.meta = (rec_lo, rec_hi, [tuple(lv[0].shape[1:]) for lv in levels])
        y = _engine.ENGINE.synthesis_pyramid(approx, levels, rec_lo, rec_hi, out_ext, plan=plan)
        if y is None:  # (bands of a level that do not share their strides: level by level, same op)
            y = approx
            for k, lv in enumerate(levels):
                nxt = levels[k + 1][0].shape[1:] if k + 1 < nlev else out_ext
                y = _engine.ENGINE.synthesis(y, lv, rec_lo, rec_hi, list(nxt))
        return y

    @staticmethod
    def backward(ctx, g_y):
        zero, eng = _engine.MODE_IDS["zero"], _engine.ENGINE

        def launch(g, lo, hi, n):  # (kernels 16 / 20, the mirror of _AnalysisPyramid.backward; the query launches nothing)
            k = eng.pyramid_levels(g, len(lo), zero, n)
            return eng.analysis_pyramid(g, lo, hi, zero, k) if k >= 2 else None

        g, grads = _chained_synthesis_adjoint(ctx.meta, g_y, 3, launch if g_y.dtype == torch.float32 else None)
        return (None, None, None, None, None, g, *grads)


def _graph_taps(tap_t, first: int):
    """What ties a level op to a learnable filter bank: its tap TENSORS ``first`` and ``first + 1`` of :func:`_tap_tensors` (0: the
    dec pair, 2: the rec pair), or ``(None, None)``."""
    return (None, None) if tap_t is None else (tap_t[first], tap_t[first + 1])


def _tap_tensors(wavelet):
    """(dec_lo, dec_hi, rec_lo, rec_hi) as the caller's TENSORS when the filter bank is learnable (any of them requires
    grad and grad mode is on), else None.  src/ptwt/_util.py:115-132 keeps such taps in the graph with torch.as_tensor."""
    if isinstance(wavelet, str) or not torch.is_grad_enabled():
        return None
    bank = wavelet if isinstance(wavelet, tuple) else getattr(wavelet, "filter_bank", ())
    if len(bank) == 4 and all(isinstance(t, torch.Tensor) for t in bank) and any(t.requires_grad for t in bank):
        return tuple(bank)
    return None


# detail-band order of each public container, as band indices of the engine (bit (n-1-a) <=> axis a high-pass)
_KEYS_ND = {
    2: ("ad", "da", "dd"),
    3: ("aad", "ada", "add", "daa", "dad", "dda", "ddd"),  # src/ptwt/conv_transform_3.py:131-141
}
# insertion order of the separable recursion (src/ptwt/separable_conv_transform.py:63-72)
_KEYS_FS = {
    2: ("da", "ad", "dd"),
    3: ("daa", "ada", "dda", "aad", "dad", "add", "ddd"),
}


def _band(key: str) -> int:
    return int(key.replace("a", "0").replace("d", "1"), 2)


# ------------------------------------------------------------------------------------------ arguments
def _mode_id(mode) -> int:
    """src/ptwt/_util.py:48-68: None means reflect, unknown strings are a ValueError."""
    if mode is None:
        mode = "reflect"
    try:
        return _engine.MODE_IDS[mode]
    except (KeyError, TypeError):
        raise ValueError(f"Padding mode not supported: {mode}") from None


def _ensure_axes(axes: AxisHint, ndim: int) -> Tuple[int, ...]:
    """src/ptwt/_util.py:817-826."""
    if axes is None:
        return tuple(range(-ndim, 0))
    if isinstance(axes, int):
        if ndim != 1:
            raise ValueError(f"tried passing single axis to {ndim}D transform")
        return (axes,)
    if len(axes) != ndim:
        raise ValueError(f"tried passing {len(axes)}D axes {axes} to {ndim}D transform")
    if len(set(axes)) != len(axes):
        raise ValueError("Cant transform the same axis twice.")
    return tuple(axes)


def _permutation(axes: Sequence[int], rank: int) -> List[int]:
    """Order that moves ``axes`` (in the given order) to the end (src/ptwt/_util.py:351-363)."""
    back = [a + rank if a < 0 else a for a in axes]
    if len(set(back)) != len(back):
        raise ValueError("Cant transform the same axis twice.")
    if any(a < 0 or a >= rank for a in back):
        raise ValueError(f"axes {tuple(axes)} out of range for a {rank}-dimensional tensor")
    return [a for a in range(rank) if a not in back] + back


class _Layout:
    """Remembers how a tensor was brought to [B, N_0..N_{n-1}] so that results can be taken back
    (src/ptwt/_util.py:493-570 forward, :613-676 backward)."""

    def __init__(self, proto: torch.Tensor, ndim: int, axes: Tuple[int, ...]):
        if not isinstance(proto, torch.Tensor):
            raise ValueError("First element of coeffs must be the approximation coefficient tensor.")
        if proto.dtype not in supported_dtypes():
            raise ValueError(f"Input dtype {proto.dtype} not supported")
        self.ndim = ndim
        self.perm = None if axes == tuple(range(-ndim, 0)) else _permutation(axes, proto.dim())
        shape = list(proto.shape) if self.perm is None else [proto.shape[p] for p in self.perm]
        if len(shape) < ndim:
            raise ValueError(f"At least {ndim} input dimensions required.")
        self.lead = shape[:-ndim]  # leading (batch) dims after the swap

    def fold(self, t: torch.Tensor) -> torch.Tensor:
        if self.perm is not None:
            t = t.permute(self.perm)
        if len(self.lead) == 0:
            return t.unsqueeze(0)
        if len(self.lead) > 1:
            return t.reshape([-1] + list(t.shape[-self.ndim:]))
        return t

    def unfold(self, t: torch.Tensor) -> torch.Tensor:
        if len(self.lead) == 0:
            t = t.squeeze(0)
        elif len(self.lead) > 1:
            t = t.reshape(self.lead + list(t.shape[-self.ndim:]))
        if self.perm is not None:
            inv = [0] * len(self.perm)
            for i, p in enumerate(self.perm):
                inv[p] = i
            t = t.permute(inv)
        return t


def _check_pad(extents: Sequence[int], flen: int, mode: str) -> None:
    """The reference pads with torch.nn.functional.pad, which refuses reflect pad >= N and circular
    pad > N (RuntimeError); symmetric/zero/constant accept anything (src/ptwt/conv_transform.py:59-66)."""
    if mode not in ("reflect", "periodic"):
        return
    for n in extents:
        padl = (2 * flen - 3) // 2
        padr = padl + n % 2
        if mode == "reflect" and max(padl, padr) >= n:
            raise RuntimeError(
                f"Padding size should be less than the corresponding input dimension, but got: padding "
                f"({padl}, {padr}) at an axis of extent {n} (reflect mode, filter length {flen})"
            )
        if mode == "periodic" and max(padl, padr) > n:
            raise RuntimeError(
                f"Padding value causes wrapping around more than once: padding ({padl}, {padr}) at an axis "
                f"of extent {n} (periodic mode, filter length {flen})"
            )


# ------------------------------------------------------------------------------------------ analysis
# geometry of a graph-free decomposition -> the launches it took ((0, levels asked of the multi-level launch) / (1, 0) level pair /
# (2, levels) 1-D tail / (3, 0) one level); idempotent values, single dict operations (see the synthesis memo below)
_route_memo: dict = {}
_engine._routing_caches.append(_route_memo)


def _check_pad_levels(extents: Sequence[int], flen: int, mode, level: int) -> None:
    """The pad check of every trip of the reference's level loop (:func:`_check_pad`), walked ONCE over all ``level`` levels of a
    geometry: raises the reference's error for the first level that fails.  Every trip and every fused route relies on it."""
    mode = "reflect" if mode is None else mode
    if mode not in ("reflect", "periodic"):
        return
    ns = list(extents)
    for _ in range(level):
        _check_pad(ns, flen, mode)
        ns = [(n + flen - 1) // 2 for n in ns]


def analysis(data: torch.Tensor, wavelet, mode, level: Optional[int], axes: AxisHint, ndim: int):
    """Multi-level analysis.  Returns ``(layout, approx [B,*M], [buffer [B,2^n,*M] per level, coarsest first])``."""
    if _is_complex(data):  # (before every dtype check: complex64 / complex128 have a route of their own, in every mode)
        return _analysis_cplx(data, wavelet, mode, level, axes, ndim)
    if isinstance(mode, str) and mode == PERIODIZATION:
        return _analysis_per(data, wavelet, level, axes, ndim)
    if isinstance(mode, str) and mode in EXT_MODES:
        return _analysis_ext(data, wavelet, mode, level, axes, ndim)
    axes = _ensure_axes(axes, ndim)
    layout = _Layout(data, ndim, axes)
    x = layout.fold(data)
    dbank = device_bank(wavelet, x.device) if x.is_cuda else None
    if dbank is not None:  # the taps stay on the GPU: per-level generic route, nothing read back (include/mifwt.h, mifwt_*_dtaps)
        dec_lo, dec_hi = _engine.DevTaps(dbank[0]), _engine.DevTaps(dbank[1])
    else:
        dec_lo, dec_hi, _, _ = host_taps(wavelet)
    on_device = dbank is not None
    tap_t = _tap_tensors(wavelet)
    flen = len(dec_lo)
    if level is None:
        level = dwtn_max_level(x.shape[1:], flen)
    eng = _engine.ENGINE
    # the call builds a graph: every level runs as an autograd op.  (A learnable filter bank — `tap_t`, which implies a graph — takes
    # the per-level ops, which also produce tap gradients; device-resident taps take the per-level generic route.)
    differentiable = torch.is_grad_enabled() and (x.requires_grad or tap_t is not None)
    fusable = not on_device and tap_t is None
    # Calls that need no graph (inference: the common case, and every timed loop) REPLAY the launches their geometry took last time:
    # which levels fuse is a function of the geometry and the routing options alone, and the pad checks raise by geometry alone — a
    # geometry is memoised only after it passed them.  (32 x 1000^2 db5 periodic level 5, five launches: 79 -> ~60 us of host time a
    # call, which is what that call costs once the GPU needs less: tools/host_profile_ref.py)
    rkey = plan = None
    if not (on_device or differentiable):
        mode_id = _mode_id(mode)
        rkey = (ndim, x.shape, x.stride(), x.dtype, x.device, flen, mode_id, level, id(eng), _engine.MAX_PYRAMID_LEVELS, _engine.ROW_ALIGN,
                _engine.PYRAMID_ROW_ALIGN)
        plan = _route_memo.get(rkey)
    elif level > 0:  # (only a trip of the level loop looks at the mode)
        mode_id = _mode_id(mode)
    if plan is None:
        _check_pad_levels(x.shape[1:], flen, mode, level)
    bufs: list = []  # coarsest level first
    steps: list = []
    cur, done, taken = x, 0, 0
    while done < level:
        if plan is not None:
            cands = (plan[taken],)
            taken += 1
        else:  # the routes in the order they are tried; the last one serves everything
            left = level - done
            cands = []
            if ndim == 2 and fusable:
                cands.append((0, min(_engine.MAX_PYRAMID_LEVELS, left)))
                if left >= 2 and not differentiable:
                    cands.append((1, 0))
            if ndim == 1 and fusable and left >= 2:
                cands.append((2, left))
            cands.append((3, 0))
        for kind, arg in cands:
            # (a differentiable multi-level op hands out the next approximation, `nxt`, and each level as a tuple of its detail bands: the
            # pack_* functions take either form)
            nxt = None
            if kind == 0 and differentiable:
                # several 2-D levels per launch as ONE differentiable op where the library serves them (a query: nothing is launched)
                got = None
                if eng.pyramid_levels(cur, flen, mode_id, arg) > 0:
                    nxt, *bands = _AnalysisPyramid.apply(cur, dec_lo, dec_hi, mode_id, arg)
                    got = [tuple(bands[i : i + 3]) for i in range(0, len(bands), 3)]
            elif kind == 0:
                # several levels per launch (three of a big plane, the whole pyramid of a small one), the approximations between them kept
                # on chip (mifwt_dwt2_fwd_pyramid); may fuse fewer levels than asked
                got = eng.analysis_pyramid(cur, dec_lo, dec_hi, mode_id, arg)
            elif kind == 1:
                # two levels per launch, the approximation between them kept on chip (mifwt_dwt2_fwd_pair)
                got = eng.analysis_pair(cur, dec_lo, dec_hi, mode_id)
            elif kind == 2 and differentiable:
                try:
                    nxt, *bands = _AnalysisTail.apply(cur, dec_lo, dec_hi, mode_id, arg)
                    got = [(d,) for d in bands]
                except _FusedRouteUnavailable:
                    got = None
            elif kind == 2:
                # the deep levels of a 1-D pyramid in one launch (mifwt_dwt1_fwd_tail) once a row fits into LDS, several levels of
                # longer rows per launch before that (mifwt_dwt1_fwd_long)
                got = eng.analysis_tail(cur, dec_lo, dec_hi, mode_id, arg)
            elif differentiable:
                got = (_AnalysisLevel.apply(cur, dec_lo, dec_hi, mode_id, *_graph_taps(tap_t, 0)),)
            else:
                got = (eng.analysis(cur, dec_lo, dec_hi, mode_id),)
            if got is not None:
                break
        else:  # a replayed step refused (cannot happen while the memo is cleared with the plans; never guess: take the long way)
            _route_memo.pop(rkey, None)
            return analysis(data, wavelet, mode, level, axes, ndim)
        if plan is None:
            steps.append((kind, arg))
        bufs[:0] = got[::-1]
        done += len(got)
        cur = got[-1][:, 0] if nxt is None else nxt
    if rkey is not None and plan is None:
        if len(_route_memo) > 512:
            _route_memo.clear()
        _route_memo[rkey] = tuple(steps)
    return layout, cur, bufs


# ------------------------------------------------------------------------------------------ synthesis
# geometry of a reconstruction that passed the reference's checks -> (output extents per level, the level at which ONE launch takes over
# the rest of a 2-D reconstruction — the number of levels: no such launch —, the plan of that launch).  Idempotent values, only touched
# through single dict operations — get / item assignment / clear — each atomic under the GIL; a thread that loses a race recomputes the
# same entry.
_rec_memo: dict = {}
_engine._routing_caches.append(_rec_memo)


def _adjust_trim(res_size: int, next_size: int) -> int:
    """src/ptwt/_util.py:231-244 on the already L-2-cropped size."""
    if next_size == res_size:
        return 0
    if next_size == res_size - 1:
        return 1
    raise AssertionError("padding error, please check if dec and rec wavelets are identical.")


def _check_same_device_dtype(tensors: Sequence[torch.Tensor]) -> None:
    """src/ptwt/_util.py:307-348."""
    first = tensors[0]
    for t in tensors:
        if t.device != first.device:
            raise ValueError("coefficients must be on the same device")
    for t in tensors:
        if t.dtype != first.dtype:
            raise ValueError("coefficients must have the same dtype")


def _walk_synthesis(shape: Tuple[int, ...], folded, flen: int, ndim: int, separable: bool):
    """The checks of every trip of the reference's level loop (shapes, trims), walked ONCE over a reconstruction: ``shape`` = the folded
    approximation's.  Returns the output extents of the levels that pass, coarsest first, and the exception the reference raises at the
    level after them (None: every level passes)."""
    exts: list = []
    try:
        for pos, det in enumerate(folded):
            trims = [0] * ndim
            if separable:
                # the separable reference crops the running approximation to the detail shape
                # (src/ptwt/separable_conv_transform.py:94-97) and never trims the synthesis output
                shape = tuple(min(c, s_) for c, s_ in zip(shape, det[0].shape))
            elif pos + 1 < len(folded):
                nxt = folded[pos + 1][0].shape
                trims = [_adjust_trim(2 * shape[1 + a] - flen + 2, nxt[1 + a]) for a in range(ndim)]
            for t in det:
                if tuple(t.shape) != tuple(shape):
                    if ndim == 1:  # torch.stack in the reference (src/ptwt/conv_transform.py:186)
                        raise RuntimeError("stack expects each tensor to be equal size")
                    raise ValueError("All coefficients on each level must have the same shape")
            out_ext = [2 * shape[1 + a] - flen + 2 - trims[a] for a in range(ndim)]
            if min(out_ext) < 1:
                raise ValueError("coefficients too short for this wavelet")
            exts.append(out_ext)
            shape = (shape[0], *out_ext)
    except (ValueError, RuntimeError, AssertionError) as err:
        return exts, err
    return exts, None


def _pyramid_route(cur: torch.Tensor, folded, exts, flen: int, separable: bool):
    """Which levels of a 2-D float32 reconstruction go in ONE launch, the running approximation kept on chip (mifwt_dwt2_inv_pyramid):
    ``(first level of that launch, its plan, whether strided planes are copied first)`` — every level of a small plane, the FINEST up to three of a big one (that is where the
    bytes are; what is coarser goes first, level by level) — or ``(number of levels, None, False)``.  Geometry only; ``exts`` from the walk."""
    eng, nlev = _engine.ENGINE, len(folded)
    if cur.dtype != torch.float32:
        return nlev, None, False
    if folded[-1][0].shape[-1] * folded[-1][0].shape[-2] <= 10240:  # (the finest level's four coefficient planes must fit into LDS)
        pl = eng.synthesis_pyramid_plan(cur, folded, flen, exts[-1])
        if pl is not None and pl[3]:
            return 0, pl, False
        # the one-launch kernel reads dense planes.  Planes with a row pitch of their own — views of a larger array, as
        # array_to_coeffs hands out — are copied first (they are small) and take the same launch, so the result of a reconstruction
        # does not depend on where its coefficients lie: the per-level kernels sum in another order.  The third entry says "copy".
        if not separable:
            meta = lambda t: torch.empty(t.shape, dtype=t.dtype, device="meta")
            pl = eng.synthesis_pyramid_plan(meta(cur), [[meta(t) for t in lv] for lv in folded], flen, exts[-1])
            if pl is not None and pl[3] == 1:
                return 0, pl, True
        return nlev, None, False
    for first in range(max(nlev - 3, 0), nlev):
        if first == 0:
            a0 = cur[tuple(slice(0, s_) for s_ in folded[0][0].shape)] if separable else cur
        else:  # the approximation the coarser levels will hand over: dense, cropped to the level's band extents
            ext = (cur.shape[0], *exts[first - 1])
            if separable:
                ext = tuple(min(c, s_) for c, s_ in zip(ext, folded[first][0].shape))
            a0 = torch.empty(ext, dtype=cur.dtype, device="meta")
        pl = eng.synthesis_pyramid_plan(a0, folded[first:], flen, exts[-1])
        if pl is not None and pl[3] == 2:
            return first, pl, False
    return nlev, None, False


def synthesis(approx: torch.Tensor, levels: List[List[torch.Tensor]], wavelet, axes: AxisHint, ndim: int,
              separable: bool, mode=None) -> torch.Tensor:
    """Multi-level synthesis.  ``levels``: per level (coarsest first) the 2^n-1 detail tensors in band order.  ``mode``: "periodization"
    selects the periodized synthesis; the padded synthesis does not depend on its mode, which is only checked."""
    if _is_complex(approx):  # (a real approximation with complex details stays with the same-dtype check below)
        return _synthesis_cplx(approx, levels, wavelet, axes, ndim, separable, mode)
    if isinstance(mode, str) and mode == PERIODIZATION:
        return _synthesis_per(approx, levels, wavelet, axes, ndim, separable)
    if mode is not None and not (isinstance(mode, str) and mode in EXT_MODES):
        _mode_id(mode)
    axes = _ensure_axes(axes, ndim)
    layout = _Layout(approx, ndim, axes)
    flat = [approx] + [t for lvl in levels for t in lvl]
    for t in flat:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"Unexpected input type {type(t)}")
    _check_same_device_dtype(flat)
    dbank = device_bank(wavelet, approx.device) if approx.is_cuda else None
    if dbank is not None:  # (see analysis)
        rec_lo, rec_hi = _engine.DevTaps(dbank[2]), _engine.DevTaps(dbank[3])
    else:
        _, _, rec_lo, rec_hi = host_taps(wavelet)
    on_device = dbank is not None
    tap_t = _tap_tensors(wavelet)
    flen = len(rec_lo)
    cur = layout.fold(approx)
    folded = [[layout.fold(t) for t in lvl] for lvl in levels]
    nlev = len(folded)
    eng = _engine.ENGINE
    grad_mode = torch.is_grad_enabled()
    # the call builds a graph.  Gradients w.r.t. the coefficients only: the multi-level launches as differentiable ops
    # (_SynthesisChain1d, _SynthesisPyramid); a learnable filter bank — `tap_t`, which implies a graph — takes the per-level ops, and so
    # do device-resident taps.  (The separable containers' crops of the running approximation take its LEADING samples, like the
    # reference's trims: the adjoint of a level sees a gradient of the cropped extents and treats the rest as zeros — same backward.)
    any_grad = grad_mode and (tap_t is not None or any([t.requires_grad for t in flat]))  # (a list: one Python-level call, not one per tensor)
    fusable = not on_device and tap_t is None
    # ONE walk of the reference's checks per call, remembered per geometry (every band's shape: the shape checks are part of what is
    # remembered) together with the multi-level route, which depends on the geometry only
    hit = gkey = err = None
    if fusable and nlev:
        gkey = (cur.dtype, cur.shape, cur.stride(), tuple((lv[0].stride(), *[t.shape for t in lv]) for lv in folded), flen, separable)
        hit = _rec_memo.get(gkey)
    if hit is None:
        exts, err = _walk_synthesis(tuple(cur.shape), folded, flen, ndim, separable)
        hit = (exts, nlev, None, False)
        if gkey is not None and err is None:  # (the fused routes are considered only when the whole walk passes)
            if ndim == 2:
                hit = (exts, *_pyramid_route(cur, folded, exts, flen, separable))
            if len(_rec_memo) > 1024:
                _rec_memo.clear()
            _rec_memo[gkey] = hit
    exts, upto, plan, densify = hit  # (densify: small planes with a row pitch get dense copies for the one-launch kernel, _pyramid_route)
    stop = -1 if err is None else len(exts)  # the level at which the loop below raises the reference's error
    pos = 0
    if ndim == 1 and not separable and nlev >= 2 and fusable and stop < 0:
        # a whole 1-D reconstruction on the multi-level launches
        outs = [e[0] for e in exts]
        cap = 16384 if cur.dtype == torch.float32 else 8192
        dets = [lvl[0] for lvl in folded]

        def fuse(fuse, cur, a, b):  # (itself as an argument: a closure over its own name would be a reference cycle per call)
            """Levels a .. b-1 with as few launches as possible: the finest ones in the chunked launch (mifwt_dwt1_inv_long:
            as many as its halo rule allows), what is coarser first — chunked as well while there are too few rows for one
            workgroup each, else in the one-workgroup-per-row launch (mifwt_dwt1_inv_tail) while the outputs fit into LDS."""
            if b - a >= 2:
                y, k = eng.synthesis_long(cur, dets[a:b], rec_lo, rec_hi, outs[a:b])
                if y is not None:
                    return y
                if 2 <= k < b - a:
                    cur = fuse(fuse, cur, a, b - k)
                    a = b - k
                    y, _k = eng.synthesis_long(cur, dets[a:b], rec_lo, rec_hi, outs[a:b])
                    if y is not None:
                        return y
                nf = 0
                while a + nf < b and outs[a + nf] <= cap:
                    nf += 1
                if nf >= 2:
                    y = eng.synthesis_tail(cur, dets[a:a + nf], rec_lo, rec_hi, outs[a:a + nf])
                    if y is not None:
                        cur, a = y, a + nf
            while a < b:
                cur = eng.synthesis(cur, folded[a], rec_lo, rec_hi, [outs[a]])
                a += 1
            return cur

        if any_grad:  # (the same launches as ONE differentiable op)
            cur = _SynthesisChain1d.apply(lambda a0, dd: fuse(fuse, a0, 0, len(dd)), rec_lo, rec_hi, cur, *dets)  # (fuse reads `dets`: the same tensors)
        else:
            cur = fuse(fuse, cur, 0, nlev)
        pos = nlev
    while pos < nlev:
        det = folded[pos]
        if separable:
            cur = cur[tuple(slice(0, s_) for s_ in det[0].shape)]
        if pos == stop:
            raise err
        if pos == upto:
            # the rest in one launch (the plan was made for a dense hand-over approximation; a strided one — a separable crop — is
            # looked up afresh)
            if densify:  # (one launch of kernel 60 for all planes was tried and is slower, host-bound: EXPERIMENTS part M)
                cur = cur.contiguous()
                folded = folded[:pos] + [[t.contiguous() for t in lv] for lv in folded[pos:]]
            same = pos == 0 or cur.is_contiguous()
            if any_grad:
                y = _SynthesisPyramid.apply(rec_lo, rec_hi, tuple(exts[-1]), plan if same else None, nlev - pos, cur,
                                            *[t for lv in folded[pos:] for t in lv])
            else:
                y = eng.synthesis_pyramid(cur, folded[pos:], rec_lo, rec_hi, exts[-1], plan=plan if same else None)
            if y is not None:
                return layout.unfold(y)
            upto = nlev  # (bands that do not share their strides: level by level)
        # PER LEVEL: a coarse level whose inputs need no gradient is a plain call even when a finer level's details require one
        differentiable = grad_mode and (cur.requires_grad or any(t.requires_grad for t in det) or tap_t is not None)
        # levels go in pairs counted from the FINEST one of those left to this loop (that is where the bytes are): an odd count
        # starts with a single level
        left = upto - pos
        if (ndim == 2 and not differentiable and not on_device and left % 2 == 0 and left >= 2
                and not (grad_mode and any(t.requires_grad for t in folded[pos + 1]))):
            # two levels per launch, the approximation between them kept on chip (mifwt_dwt2_inv_pair); the checks of the
            # second trip are the reference's own and come before anything is launched.  Separable containers: the crop of the
            # running approximation to the next detail shape IS the extent the kernel synthesises the approximation tile for
            if pos + 1 == stop:
                raise err
            y = eng.synthesis_pair(cur, det, folded[pos + 1], rec_lo, rec_hi, exts[pos + 1])
            if y is not None:
                cur = y
                pos += 2
                continue
        if differentiable:
            cur = _SynthesisLevel.apply(rec_lo, rec_hi, tuple(exts[pos]), *_graph_taps(tap_t, 2), cur, *det)
        else:
            cur = eng.synthesis(cur, det, rec_lo, rec_hi, exts[pos])
        pos += 1
    return layout.unfold(cur)


# ------------------------------------------------------------------------------------------ periodization
# PyWavelets' mode="periodization" (include/mifwt.h, _per.py): ceil(n / 2) coefficients per axis and level, any extent, one level
# call per trip.  Not one of _engine.MODE_IDS — the Matrix* classes consult those for their odd_coeff_padding_mode — so both drivers
# branch on the string before _mode_id.
PERIODIZATION = "periodization"


def _per_taps(wavelet, proto: torch.Tensor, mode: str = PERIODIZATION):
    """The refusals of the periodized mode (and of the value-map extension modes, ``mode``) that need no device, and the bank as host
    floats (tensor taps are read once)."""
    if proto.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"Input dtype {proto.dtype} not supported")
    if _tap_tensors(wavelet) is not None:
        raise NotImplementedError(f"mode='{mode}' does not take a learnable filter bank (taps that require grad)")
    bank = wavelet if isinstance(wavelet, tuple) else getattr(wavelet, "filter_bank", ())
    tensor_bank = not isinstance(wavelet, str) and len(bank) == 4 and all(isinstance(t, torch.Tensor) for t in bank)
    if tensor_bank and (_wavelets._device_taps_mode == "always" or (proto.is_cuda and device_bank(wavelet, proto.device) is not None)):
        raise NotImplementedError(f"mode='{mode}' does not take device-resident taps (set_device_taps): its kernels read host taps")
    taps = host_taps(wavelet)
    if len(taps[0]) != len(taps[2]) or len(taps[0]) % 2:
        raise ValueError(f"mode='{mode}' needs dec and rec filters of one even length")
    return taps


def _analysis_per(data: torch.Tensor, wavelet, level: Optional[int], axes: AxisHint, ndim: int):
    from . import _per

    axes = _ensure_axes(axes, ndim)
    layout = _Layout(data, ndim, axes)
    dec_lo, dec_hi, _, _ = _per_taps(wavelet, data)
    x = layout.fold(data)
    if level is None:
        level = dwtn_max_level(x.shape[1:], len(dec_lo))
    elif level < 0:  # (pywt.wavedec: "Level value must be >= 0"; level 0 returns the input as the approximation, as in every mode)
        raise ValueError(f"Level value of {level} is too low. Minimum level is 0.")
    _engine._require_gpu(x)
    bufs: list = []  # coarsest level first
    cur = x
    for _ in range(level):
        buf = _per.fwd(cur, dec_lo, dec_hi)
        bufs.insert(0, buf)
        cur = buf[:, 0]
    return layout, cur, bufs


def _synthesis_per(approx: torch.Tensor, levels: List[List[torch.Tensor]], wavelet, axes: AxisHint, ndim: int, separable: bool) -> torch.Tensor:
    from . import _per

    axes = _ensure_axes(axes, ndim)
    layout = _Layout(approx, ndim, axes)
    flat = [approx] + [t for lvl in levels for t in lvl]
    for t in flat:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"Unexpected input type {type(t)}")
    _check_same_device_dtype(flat)
    _, _, rec_lo, rec_hi = _per_taps(wavelet, approx)
    cur = layout.fold(approx)
    _engine._require_gpu(cur)
    folded = [[layout.fold(t) for t in lvl] for lvl in levels]
    for pos, det in enumerate(folded):
        if separable:  # (the separable containers crop the running approximation to the detail shape, as in the padded synthesis)
            cur = cur[tuple(slice(0, s_) for s_ in det[0].shape)]
        for t in det:
            if tuple(t.shape) != tuple(cur.shape):
                if ndim == 1:
                    raise RuntimeError("stack expects each tensor to be equal size")
                raise ValueError("All coefficients on each level must have the same shape")
        out_ext = [2 * int(m) for m in cur.shape[1:]]
        if not separable and pos + 1 < len(folded):
            # an intermediate result loses its last sample along an axis where it is one longer than the next level's details
            nxt = folded[pos + 1][0].shape
            out_ext = [n - _adjust_trim(n, int(nxt[1 + a])) for a, n in enumerate(out_ext)]
        cur = _per.inv([cur, *det], rec_lo, rec_hi, out_ext)
    return layout.unfold(cur)


# ------------------------------------------------------------------------------------------ smooth / antisymmetric / antireflect
# PyWavelets' three value-map extension modes (include/mifwt.h, _ext.py): padded levels — floor((n + L - 1) / 2) coefficients per axis, the
# padded synthesis inverts them — whose extension no index map expresses.  Not among _engine.MODE_IDS either: one level call per trip.
EXT_MODES = ("smooth", "antisymmetric", "antireflect")


def _analysis_ext(data: torch.Tensor, wavelet, mode: str, level: Optional[int], axes: AxisHint, ndim: int):
    from . import _ext

    axes = _ensure_axes(axes, ndim)
    layout = _Layout(data, ndim, axes)
    dec_lo, dec_hi, _, _ = _per_taps(wavelet, data, mode)
    x = layout.fold(data)
    if level is None:
        level = dwtn_max_level(x.shape[1:], len(dec_lo))
    elif level < 0:
        raise ValueError(f"Level value of {level} is too low. Minimum level is 0.")
    _engine._require_gpu(x)
    bufs: list = []  # coarsest level first
    cur = x
    for _ in range(level):
        buf = _ext.fwd(cur, dec_lo, dec_hi, mode)
        bufs.insert(0, buf)
        cur = buf[:, 0]
    return layout, cur, bufs


# ------------------------------------------------------------------------------------------ complex data
# complex64 / complex128 in every mode (include/mifwt.h, _cplx.py): the taps are real, so T(a + i b) = T(a) + i T(b), which is what
# PyWavelets computes.  FUSED: the five index-map modes on a ROCm tensor, host taps, no graph wanted — one complex level call per trip
# (interleaved kernels; a level outside their envelope composes itself from the two real levels).  COMPOSED: every other call is
# torch.complex(f(x.real), f(x.imag)) with f the real call of this module, whose checks raise what they raise for real data and whose
# autograd Functions, with torch's own real / imag / complex backward, give data gradients of any order and the tap gradients.
def _is_complex(t) -> bool:
    return isinstance(t, torch.Tensor) and t.dtype in (torch.complex64, torch.complex128)


def _cplx_composed(wavelet, tensors: Sequence[torch.Tensor], mode) -> bool:
    """Whether a call on complex data is composed from the real calls (see above); refuses complex taps."""
    bank = () if isinstance(wavelet, str) else (wavelet if isinstance(wavelet, tuple) else getattr(wavelet, "filter_bank", ()))
    if any(isinstance(t, torch.Tensor) and t.is_complex() for t in bank):
        raise ValueError("the filter taps of a transform of complex data must be real")
    if not (mode is None or (isinstance(mode, str) and mode in _engine.MODE_IDS)):
        return True
    if not all(t.is_cuda for t in tensors):
        return True  # (the real call raises the engine's error about the ROCm device)
    if torch.is_grad_enabled() and (_tap_tensors(wavelet) is not None or any([t.requires_grad for t in tensors])):
        return True
    return device_bank(wavelet, tensors[0].device) is not None or len(host_taps(wavelet)[0]) % 2 == 1


def _analysis_cplx(data: torch.Tensor, wavelet, mode, level: Optional[int], axes: AxisHint, ndim: int):
    from . import _cplx

    if _cplx_composed(wavelet, [data], mode):
        layout, a_re, b_re = analysis(data.real, wavelet, mode, level, axes, ndim)
        _, a_im, b_im = analysis(data.imag, wavelet, mode, level, axes, ndim)
        return layout, torch.complex(a_re, a_im), [_cplx.tree_complex(r, i) for r, i in zip(b_re, b_im)]
    axes = _ensure_axes(axes, ndim)
    layout = _Layout(data.real, ndim, axes)  # (the float view: a layout holds shapes and the permutation only)
    x = layout.fold(data)
    dec_lo, dec_hi, _, _ = host_taps(wavelet)
    flen = len(dec_lo)
    if level is None:
        level = dwtn_max_level(x.shape[1:], flen)
    mode_id = _mode_id(mode)
    _check_pad_levels(x.shape[1:], flen, mode, level)
    bufs: list = []  # coarsest level first
    cur = x
    for _ in range(level):
        buf = _cplx.level_fwd(cur, dec_lo, dec_hi, mode_id)
        bufs.insert(0, buf)
        cur = buf[:, 0]
    return layout, cur, bufs


def _synthesis_cplx(approx: torch.Tensor, levels: List[List[torch.Tensor]], wavelet, axes: AxisHint, ndim: int, separable: bool,
                    mode) -> torch.Tensor:
    from . import _cplx

    flat = [approx] + [t for lvl in levels for t in lvl]
    for t in flat:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"Unexpected input type {type(t)}")
    _check_same_device_dtype(flat)  # (a container that mixes real and complex tensors: the same-dtype error)
    if _cplx_composed(wavelet, flat, mode):
        parts = [synthesis(part(approx), [[part(t) for t in lvl] for lvl in levels], wavelet, axes, ndim, separable, mode)
                 for part in (torch.real, torch.imag)]
        return torch.complex(*parts)
    axes = _ensure_axes(axes, ndim)
    layout = _Layout(approx.real, ndim, axes)
    _, _, rec_lo, rec_hi = host_taps(wavelet)
    flen = len(rec_lo)
    cur = layout.fold(approx)
    folded = [[layout.fold(t) for t in lvl] for lvl in levels]
    exts, err = _walk_synthesis(tuple(cur.shape), folded, flen, ndim, separable)
    for pos, det in enumerate(folded):
        if separable:
            cur = cur[tuple(slice(0, s_) for s_ in det[0].shape)]
        if pos == len(exts):
            raise err
        cur = _cplx.level_inv([cur, *det], rec_lo, rec_hi, exts[pos])
    return layout.unfold(cur)


# ------------------------------------------------------------------------------------------ containers
def pack_1d(layout: _Layout, approx, bufs) -> List[torch.Tensor]:
    # (the detail row is the last plane of a level buffer — [B, 2, M] or [B, 1, M] — or the one band of a differentiable multi-level launch)
    return [layout.unfold(approx)] + [layout.unfold(b[-1] if isinstance(b, tuple) else b[:, -1]) for b in bufs]


def pack_2d(layout: _Layout, approx, bufs):
    out = [layout.unfold(approx)]
    unfold = layout.unfold
    for b in bufs:  # (H, V, D) = ('da', 'ad', 'dd') = bands 2, 1, 3 (one unbind: a third of the host time of three b[:, k])
        # ([B, 4, ..] with the approximation in plane 0, [B, 3, ..] from a multi-level launch, or the three bands of a differentiable one)
        ad, da, dd = b if isinstance(b, tuple) else b.unbind(1)[-3:]
        out.append(WaveletDetailTuple2d(unfold(da), unfold(ad), unfold(dd)))
    return tuple(out)


def pack_dict(layout: _Layout, approx, bufs, keys: Sequence[str]):
    out: list = [layout.unfold(approx)]
    unfold = layout.unfold
    keys = tuple(keys)
    idx = _BAND_OF_KEYS.get(keys)
    if idx is None:
        idx = _BAND_OF_KEYS[keys] = tuple(_band(k) for k in keys)  # (the string arithmetic of _band per key and call was 8 us of a wavedec3)
    nb = 1 << len(keys[0])
    for b in bufs:
        planes = b if isinstance(b, tuple) else b.unbind(1)
        off = nb - len(planes)  # 1 for a details-only buffer of a multi-level launch (plane s - 1 = band s)
        out.append({k: unfold(planes[i - off]) for k, i in zip(keys, idx)})
    return tuple(out)


_BAND_OF_KEYS: dict = {}


def unpack_dict_levels(coeffs, ndim: int, what: str) -> List[List[torch.Tensor]]:
    """dict levels -> band-ordered lists; validates like src/ptwt/conv_transform_3.py:194-204 /
    separable_conv_transform.py:174-177."""
    nb = 1 << ndim
    levels = []
    for c in coeffs[1:]:
        if not isinstance(c, dict) or len([k for k in c if k != "a" * ndim]) != nb - 1:
            raise ValueError(
                f"Unexpected detail coefficient type: {type(c)}. Detail coefficients must be a dict containing "
                f"{nb - 1} tensors as returned by {what}."
            )
        try:
            levels.append([c[format(s, f"0{ndim}b").replace("0", "a").replace("1", "d")] for s in range(1, nb)])
        except KeyError as e:
            raise ValueError(f"missing detail coefficient key {e} for a {ndim}D transform") from None
    return levels
