"""Host path of the COMPLEX levels (``torch.complex64`` / ``torch.complex128`` data in the five index-map modes; C ABI ``mifwt_cplx_*``,
include/mifwt.h; kernels csrc/mifwt_cplx.hip).

The taps are real, so a level filters the two components separately, ``T(a + i b) = T(a) + i T(b)``, band by band — what PyWavelets
computes for complex input.  Two maps on interleaved data, taps as host floats in PyWavelets order, ``M = floor((n + L - 1) / 2)``:

    level_fwd(x, dec_lo, dec_hi, mode_id)            x [B, n..] complex            -> buffer [B, 2^d, M..] complex
    level_inv(bands, rec_lo, rec_hi, out_extent)     2^d bands [B, M..] complex    -> y [B, *out_extent], 2 M - L + 2 or one less per axis

each ONE fused launch (kernel ids 46 / 47) for one or two transformed axes, even ``L <= 20`` and unit innermost strides (counted in
complex elements).  Three transformed axes: the fused 2-D launch over the last two axes with depth folded into the batch plus ONE pass
along depth on the real view ``[outer, n, 2 M1 M2]`` of floats (``Engine.analysis_outer`` / ``synthesis_outer``; along an outer axis
complex data is real data of doubled width).  A fused level allocates its outputs and enqueues launches, nothing else: no host round
trip, capturable.

Everything else is COMPOSED: ``torch.complex(f(x.real), f(x.imag))`` with ``f`` the real level of ``_engine.ENGINE`` — longer filters, a
non-unit innermost stride, and the cells of :data:`COMPOSED_CELLS`.  Whole calls that need a graph, device-resident taps or one of the
four other modes are composed one floor up, in ``_fwt`` (from the real calls, whose autograd Functions then give every gradient).
"""
from __future__ import annotations

import ctypes
from typing import List, Sequence, Set, Tuple

import torch

from . import _engine

KID_FWD, KID_INV = 46, 47
COMPONENT = {torch.complex64: torch.float32, torch.complex128: torch.float64}

# Tests and tools/cplx_bench.py set this to run a level through the composed route although the fused kernels would take it.
FORCE_COMPOSED = False
# (direction, dtype, L, ndim) cells of the fused envelope (direction 0 analysis, 1 synthesis; ndim 3 = the fused 2-D launch + the depth
# pass).  FUSED_AHEAD: the cells that `tools/cplx_bench.py --sweep` measured and did not find behind the composed route (median of five
# windows against median, by more than the spread of the windows).  All 120 of them: the fused median leads the composed one 2.1 - 8.8 x
# at window spreads below 1 % (profiles/cplx_sweep.jsonl; README "Complex data").
_ENVELOPE: Set[Tuple[int, torch.dtype, int, int]] = {
    (direction, dtype, flen, ndim) for direction in (0, 1) for dtype in COMPONENT for flen in range(2, 21, 2) for ndim in (1, 2, 3)
}
FUSED_AHEAD: Set[Tuple[int, torch.dtype, int, int]] = set(_ENVELOPE)
# ... and the cells that take the composed route although the kernels would serve them.  The project's rule: a cell is here where its
# fused median was measured behind the composed one by more than the spread of the windows, and where it was NOT MEASURED.  Empty.
COMPOSED_CELLS: Set[Tuple[int, torch.dtype, int, int]] = _ENVELOPE - FUSED_AHEAD

_entries = None


def is_complex_dtype(dtype: torch.dtype) -> bool:
    """The predicate of the complex route: the two complex dtypes whose components the kernels compute in."""
    return dtype in COMPONENT


def _lib():
    """The entry points of these levels (``_engine.CPLX_ENTRIES``), bound on first use."""
    global _entries
    if _entries is None:
        _entries = _engine.private_entries(_engine.CPLX_ENTRIES)
    return _entries


_unit_last = _engine._unit_last
_plans: dict = {}
_engine._routing_caches.append(_plans)


def _desc(ndim, dtype, mode_id, flen, batch, sig, sig_stride, coef, approx_stride, detail_stride):
    """The level descriptor of complex tensors: the COMPONENT type, extents and strides in complex elements (torch's own)."""
    return _engine._desc(ndim, COMPONENT[dtype], mode_id, flen, batch, sig, sig_stride, coef, approx_stride, detail_stride)


def _launch(direction: int, extent, anchor: torch.Tensor, entry, *args) -> None:
    _engine._run(("cplx_fwd", "cplx_inv")[direction], (KID_FWD, KID_INV)[direction], extent, anchor, entry, args)


def _route(direction: int, key, dtype: torch.dtype, flen: int, ndim: int, desc):
    """(reference to the level descriptor, whether the fused kernel takes the level); the descriptor ``desc()`` builds and the library's
    answer (``mifwt_cplx_supported``) are cached under ``key``, which names everything the descriptor holds."""
    def build():
        d = desc()
        ok = _lib().mifwt_cplx_supported(ctypes.byref(d), direction)
        if ok < 0:
            _engine._check(ok)
        return d, ctypes.byref(d), bool(ok)

    _, ref, fused = _engine._plan(key, build, _plans)
    return ref, fused and not FORCE_COMPOSED and (direction, dtype, flen, ndim) not in COMPOSED_CELLS


def _setup(t: torch.Tensor, ndim: int, flen: int) -> None:
    _engine._require_gpu(t)
    if not is_complex_dtype(t.dtype):
        raise ValueError(f"Input dtype {t.dtype} not supported by the complex levels (complex64 / complex128)")
    if not 1 <= ndim <= 3:
        raise NotImplementedError("complex levels exist for one, two and three transformed axes")
    if flen < 2 or flen % 2:
        raise ValueError("complex levels need filters of an even length")


def _may_fuse(dtype: torch.dtype, direction: int, flen: int, ndim: int) -> bool:
    return flen <= 20 and not FORCE_COMPOSED and (direction, dtype, flen, ndim) not in COMPOSED_CELLS


def _real3(t: torch.Tensor, outer: int, n: int) -> torch.Tensor:
    """A dense complex tensor as the float view [outer, n, 2 * rest]."""
    return torch.view_as_real(t).view(outer, n, -1)


# ---- the composed levels: the real level of each component ------------------------------------------------------------------------------
def composed_fwd(x: torch.Tensor, dec_lo, dec_hi, mode_id: int) -> torch.Tensor:
    eng = _engine.ENGINE
    return torch.complex(eng.analysis(x.real, dec_lo, dec_hi, mode_id), eng.analysis(x.imag, dec_lo, dec_hi, mode_id))


def composed_inv(bands: Sequence[torch.Tensor], rec_lo, rec_hi, out_extent: Sequence[int]) -> torch.Tensor:
    eng = _engine.ENGINE
    out_extent = [int(n) for n in out_extent]
    return torch.complex(eng.synthesis(bands[0].real, [t.real for t in bands[1:]], rec_lo, rec_hi, out_extent),
                         eng.synthesis(bands[0].imag, [t.imag for t in bands[1:]], rec_lo, rec_hi, out_extent))


# ---- the two level maps ---------------------------------------------------------------------------------------------------------------------
def level_fwd(x: torch.Tensor, dec_lo: Sequence[float], dec_hi: Sequence[float], mode_id: int) -> torch.Tensor:
    """x [B, n0(, n1(, n2))] complex -> buffer [B, 2^d, M0(, M1(, M2))], plane s = band s (bit (d-1-a) of s set <=> high-pass along axis
    a).  (Three axes on the fused route: the buffer is a view whose planes are dense tensors of their own.)"""
    ndim = x.dim() - 1
    flen = len(dec_lo)
    _setup(x, ndim, flen)
    sig = [int(n) for n in x.shape[1:]]
    coef = [(n + flen - 1) // 2 for n in sig]
    b = int(x.shape[0])
    if not _may_fuse(x.dtype, 0, flen, ndim) or x.stride(-1) != 1 or min(sig) < 1:
        return composed_fwd(x, dec_lo, dec_hi, mode_id)
    lo, hi = _engine._taps_array(dec_lo), _engine._taps_array(dec_hi)
    if ndim == 3:
        if not _engine.outer_axis_supported(flen, COMPONENT[x.dtype]):
            return composed_fwd(x, dec_lo, dec_hi, mode_id)
        xc = x if x.is_contiguous() else x.contiguous()
        x2 = xc.view(b * sig[0], sig[1], sig[2])
        tmp = torch.empty((4, b * sig[0], coef[1], coef[2]), dtype=x.dtype, device=x.device)
        st = tmp.stride()[1:]
        ref, fused = _route(0, (0, 3, mode_id, x2.shape, x2.stride(), tuple(st), x.dtype, flen), x.dtype, flen, 3,
                            lambda: _desc(2, x.dtype, mode_id, flen, b * sig[0], sig[1:], x2.stride(), coef[1:], st, st))
        if not fused:
            return composed_fwd(x, dec_lo, dec_hi, mode_id)
        out = torch.empty((8, b, *coef), dtype=x.dtype, device=x.device)
        if out.numel():
            planes = list(tmp.unbind(0))
            _launch(0, tuple(sig[1:]), x2, _lib().mifwt_cplx_fwd, ref, x2.data_ptr(), planes[0].data_ptr(), _engine._ptr_array(planes[1:]), lo, hi)
            # along depth the four planes are real data of doubled width: one pass, low bands into planes 0..3, high bands into 4..7
            _engine.ENGINE.analysis_outer(_real3(tmp, 4 * b, sig[0]), dec_lo, dec_hi, mode_id,
                                          out=(_real3(out[:4], 4 * b, coef[0]), _real3(out[4:], 4 * b, coef[0])))
        return out.transpose(0, 1)
    buf = torch.empty((b, 1 << ndim, *coef), dtype=x.dtype, device=x.device)
    if buf.numel() == 0:
        return buf
    st = [buf.stride(0), *buf.stride()[2:]]
    ref, fused = _route(0, (0, ndim, mode_id, x.shape, x.stride(), tuple(st), x.dtype, flen), x.dtype, flen, ndim,
                        lambda: _desc(ndim, x.dtype, mode_id, flen, b, sig, x.stride(), coef, st, st))
    if not fused:
        return composed_fwd(x, dec_lo, dec_hi, mode_id)
    planes = list(buf.unbind(1))
    _launch(0, tuple(sig), x, _lib().mifwt_cplx_fwd, ref, x.data_ptr(), planes[0].data_ptr(), _engine._ptr_array(planes[1:]), lo, hi)
    return buf


def level_inv(bands: Sequence[torch.Tensor], rec_lo: Sequence[float], rec_hi: Sequence[float], out_extent: Sequence[int]) -> torch.Tensor:
    """The 2^d bands [B, M0(, M1(, M2))] of a level, complex, in band order -> y [B, *out_extent]: the padded synthesis, cropped to
    ``out_extent`` (2 M - L + 2 or one less per axis)."""
    bands = list(bands)
    ndim = bands[0].dim() - 1
    flen = len(rec_lo)
    _setup(bands[0], ndim, flen)
    coef = [int(m) for m in bands[0].shape[1:]]
    sig = [int(n) for n in out_extent]
    b = int(bands[0].shape[0])
    if len(bands) != 1 << ndim or len(sig) != ndim or any(t.shape != bands[0].shape or t.dtype != bands[0].dtype for t in bands):
        raise ValueError(f"a complex level over {ndim} axes takes {1 << ndim} bands of one shape and dtype")
    if any(n not in (2 * m - flen + 2, 2 * m - flen + 1) or n < 1 for n, m in zip(sig, coef)):
        raise ValueError(f"{tuple(coef)} coefficients and {flen} taps do not synthesise an output of extent {tuple(sig)}")
    dtype = bands[0].dtype
    if not _may_fuse(dtype, 1, flen, ndim) or b == 0:
        return composed_inv(bands, rec_lo, rec_hi, sig)
    lo, hi = _engine._taps_array(rec_lo), _engine._taps_array(rec_hi)
    if ndim == 3:
        if not _engine.outer_axis_supported(flen, COMPONENT[dtype]):
            return composed_inv(bands, rec_lo, rec_hi, sig)
        y = torch.empty((b, *sig), dtype=dtype, device=bands[0].device)
        y2 = y.view(b * sig[0], sig[1], sig[2])
        st = (coef[1] * coef[2], coef[2], 1)  # (the depth pass hands over dense planes [B * n0, M1, M2])
        ref, fused = _route(1, (1, 3, y2.shape, y2.stride(), tuple(coef), dtype, flen), dtype, flen, 3,
                            lambda: _desc(2, dtype, 0, flen, b * sig[0], sig[1:], y2.stride(), coef[1:], st, st))
        if not fused:
            return composed_inv(bands, rec_lo, rec_hi, sig)
        # along depth, on the real views (band q pairs with band q + 4): four launches, each plane read once
        planes = []
        for q in range(4):
            lo_b, hi_b = (t if t.is_contiguous() else t.contiguous() for t in (bands[q], bands[q + 4]))
            u = _engine.ENGINE.synthesis_outer(_real3(lo_b, b, coef[0]), _real3(hi_b, b, coef[0]), rec_lo, rec_hi, sig[0])
            planes.append(torch.view_as_complex(u.view(b * sig[0], coef[1], coef[2], 2)))
        _launch(1, tuple(sig[1:]), y2, _lib().mifwt_cplx_inv, ref, planes[0].data_ptr(), _engine._ptr_array(planes[1:]), y2.data_ptr(), lo, hi)
        return y
    approx = _unit_last(bands[0])
    details, dst = _engine._share_strides(bands[1:], unit_last=True)
    y = torch.empty((b, *sig), dtype=dtype, device=approx.device)
    ref, fused = _route(1, (1, ndim, y.shape, y.stride(), tuple(coef), approx.stride(), tuple(dst), dtype, flen), dtype, flen, ndim,
                        lambda: _desc(ndim, dtype, 0, flen, b, sig, y.stride(), coef, approx.stride(), dst))
    if not fused:
        return composed_inv(bands, rec_lo, rec_hi, sig)
    _launch(1, tuple(sig), y, _lib().mifwt_cplx_inv, ref, approx.data_ptr(), _engine._ptr_array(details), y.data_ptr(), lo, hi)
    return y


def tree_complex(re, im):
    """``torch.complex`` over two containers of one structure (tensors, tuples, lists, dicts)."""
    if isinstance(re, torch.Tensor):
        return torch.complex(re, im)
    if isinstance(re, dict):
        return type(re)((k, tree_complex(v, im[k])) for k, v in re.items())
    if isinstance(re, (tuple, list)):
        parts = [tree_complex(a, c) for a, c in zip(re, im)]
        return type(re)(*parts) if hasattr(re, "_fields") else type(re)(parts)
    return re
