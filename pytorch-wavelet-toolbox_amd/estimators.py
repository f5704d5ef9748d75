"""Noise and threshold estimators on the device — what produces the thresholds that :func:`ptwt_amd.threshold` reads (C ABI
``mifwt_estim_*``, include/mifwt.h; kernels csrc/mifwt_estim.hip, ids 50 .. 53).

    coeffs = ptwt_amd.wavedec2(x, "db4", level=3)
    sigma = ptwt_amd.estimate_sigma(coeffs)                  # one value per image, from the finest diagonal band
    shrunk = ptwt_amd.shrink(coeffs, "bayes", "soft")        # BayesShrink thresholds per band and image, applied in one launch
    y = ptwt_amd.waverec2(shrunk, "db4")

``estimate_sigma`` is the median absolute deviation of the finest all-high band, ``median(|d|) / 0.6744897501960817``.  The median is
numpy's: for an even count the mean of the two middle order statistics.  The order statistics are EXACT — a radix selection on the bit
patterns with the sign cleared, the bits a sort gives — and the mean and the division run in float64 and are rounded once.  Zeros are
NOT masked out (scikit-image's ``estimate_sigma`` of ``denoise_wavelet`` drops exact zeros first; here a band with many zeros gives the
smaller estimate).  ``estimate_thresholds`` gives scikit-image's VisuShrink (``sigma sqrt(2 ln n)``) and BayesShrink
(``sigma^2 / sqrt(max(mean(d^2) - sigma^2, eps))``, per band) thresholds as LEADING-FORM tensors, one value per leading index (per image),
in the nesting of the container; ``shrink`` applies them with the thresholding launch of ``thresholding.py``.

Everything is written on the device and enqueued on the caller's stream: nothing is copied to the host, nothing synchronises, a call
can be captured (``ptwt_amd.capture``) and a replay sees the noise level of the data it runs on.  The selection uses integer counters
only and the sums of squares are added in a fixed order in float64: two runs give the same bits.

Two routes select.  An image of at most :func:`lds_capacity` elements is selected by one workgroup from keys held in LDS (id 50); a
longer one by digit passes over the band with per-workgroup LDS histograms flushed into integer counters (id 51).  ``FORCE_STREAM``
sends every size down the second route (tests, tools).  Limits: the collapsed form of ``thresholding._form``, beyond which the call is
composed from torch operations (:func:`_composed_sigma`, :func:`_composed_moment`), and fewer than 2^31 elements per leading index:
from there on the moments are composed and the order statistics raise ``ValueError`` (their composition is ``torch.sort``, which takes
at most 2^31 - 1 elements along the sorted axis).  float32 and float64 data only.
"""
from __future__ import annotations

import ctypes
import math
import numbers
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _engine
from . import thresholding as _thr

__all__ = ["estimate_sigma", "estimate_thresholds", "shrink"]

KID_SELECT_LDS, KID_SELECT_STREAM, KID_MOMENTS, KID_VISU = 50, 51, 52, 53
#: ``method`` of the C ABI (MIFWT_ESTIM_*)
METHODS = {"visu": 0, "bayes": 1}
MAD_SCALE = 0.6744897501960817
#: test / tool switch: the streaming selection (id 51) at every size
FORCE_STREAM = False
#: (dtype, elements per leading index) cells inside the LDS capacity that take the streaming selection all the same, and cells whose
#: order statistics come from the torch composition (a sort) instead of the kernels: a cell belongs there only where
#: tools/estimator_bench.py has shown the default's median behind by more than the spread of its windows.  Empty: the LDS-resident
#: selection led the streaming one, and both led the sort, in every cell measured (EXPERIMENTS part E).
STREAM_CELLS: set = set()
COMPOSED_CELLS: set = set()
_COUNT_LIMIT = 1 << 31
_DTYPES = (torch.float32, torch.float64)

_entries = None


def _lib():
    global _entries
    if _entries is None:
        _entries = _engine.private_entries(_engine.ESTIM_ENTRIES)
    return _entries


def max_segments() -> int:
    """Bands one moments launch takes (``mifwt_estim_max_segments``)."""
    return int(_lib().mifwt_estim_max_segments())


def lds_capacity(dtype: torch.dtype) -> int:
    """Elements per leading index the LDS-resident selection takes (``mifwt_estim_lds_capacity``)."""
    return int(_lib().mifwt_estim_lds_capacity(_engine._DTYPE_IDS[dtype]))


def stream_plan(dtype: torch.dtype) -> List[Tuple[int, int]]:
    """(shift, width) of the digit passes of the streaming selection, first pass first (``mifwt_estim_stream_plan``)."""
    dt = _engine._DTYPE_IDS[dtype]
    shift, width = ctypes.c_int(), ctypes.c_int()
    plan = []
    for p in range(_lib().mifwt_estim_stream_plan(dt, -1, None, None)):
        _lib().mifwt_estim_stream_plan(dt, p, ctypes.byref(shift), ctypes.byref(width))
        plan.append((shift.value, width.value))
    return plan


# ---- containers ------------------------------------------------------------------------------------------------------------------
def _check_dtype(t: torch.Tensor) -> None:
    if t.dtype not in _DTYPES:
        raise ValueError(f"estimators: float32 and float64 data only, got {t.dtype}")


def _finest(data, lead: Optional[int]) -> Tuple[torch.Tensor, int]:
    """(the finest all-high band of ``data``, the number of its leading axes)."""
    if isinstance(data, torch.Tensor):
        d, axes = data, None
    elif isinstance(data, (list, tuple)) and len(data) > 0:
        last = data[-1]
        if isinstance(last, torch.Tensor):
            d, axes = last, 1
        elif isinstance(last, dict):
            ndim = len(next(iter(last))) if last else 0
            if ndim == 0 or "d" * ndim not in last:
                raise ValueError("estimate_sigma: the last dict of the container has no all-high band")
            d, axes = last["d" * ndim], ndim
        elif isinstance(last, tuple) and hasattr(last, "diagonal"):
            d, axes = last.diagonal, 2
        else:
            raise TypeError(f"estimate_sigma: no detail band in a container that ends in {type(last).__name__}")
    else:
        raise TypeError(f"estimate_sigma: expected a tensor or a coefficient container, got {type(data).__name__}")
    _check_dtype(d)
    if lead is None:
        lead = 0 if axes is None else d.dim() - axes
    if not isinstance(lead, numbers.Integral) or isinstance(lead, bool) or not 0 <= lead <= d.dim():
        raise ValueError(f"estimate_sigma: lead must be in [0, {d.dim()}], got {lead!r}")
    return d, int(lead)


def _band(t: torch.Tensor, lead: int):
    """``t`` as the kernels read it: (the tensor to read — ``t`` or a contiguous copy —, extents, strides, rows per leading index
    (0: one), elements per leading index), or None outside the kernels' envelope."""
    geo = _thr._geometry(t, (lead, 0))
    if geo is None:
        return None
    xr, ext, st, rp = geo
    rows = ext[0] * ext[1]
    count = (rp[0] if rp[0] else rows) * ext[2]
    if count >= _COUNT_LIMIT:
        return None
    return xr, ext, st, rp[0], count


def _fill(b: _engine.EstimBand, band) -> None:
    xr, ext, st, rp, _ = band
    b.x = xr.data_ptr()
    b.extent[:] = ext
    b.stride[:] = st
    b.rows_per_index = rp


# ---- order statistics and sigma ----------------------------------------------------------------------------------------------------
def _composed_sigma(d: torch.Tensor, lead: int):
    """(order statistics [images, 2], sigma [images]) from torch operations: the route beyond the kernels' limits, and the emulation the
    benchmark compares them with."""
    images = math.prod(d.shape[:lead])
    s = d.detach().abs().reshape(images, -1).sort(-1).values
    c = s.shape[1]
    stats = torch.stack((s[:, (c - 1) // 2], s[:, c // 2]), -1)
    sigma = ((stats[:, 0].double() + stats[:, 1].double()) * 0.5 / MAD_SCALE).to(d.dtype)
    return stats, sigma


def _check_count(d: torch.Tensor, lead: int) -> None:
    """The order statistics of 2^31 elements per leading index and more are refused: no kernel takes them, and neither does the sort
    of the composition."""
    images = math.prod(d.shape[:lead])
    count = d.numel() // images if images else 0
    if count >= _COUNT_LIMIT:
        raise ValueError(f"estimate_sigma: the order statistics take fewer than 2^31 elements per leading index, got {count}")


def _select(d: torch.Tensor, lead: int, want_stats: bool = False):
    """(sigma in ``d``'s dtype [images], the same values in float64 [images], the two order statistics [images, 2] or None) of a
    non-empty band ``d`` on the device."""
    d = d.detach()
    images = math.prod(d.shape[:lead])
    band = _band(d, lead)
    cell = (d.dtype, d.numel() // images)
    if band is None or cell in COMPOSED_CELLS:
        stats, sigma = _composed_sigma(d, lead)
        return sigma, sigma.double(), stats
    dt = _engine._DTYPE_IDS[d.dtype]
    b = _engine.EstimBand()
    _fill(b, band)
    ref = ctypes.byref(b)
    route = int(_lib().mifwt_estim_select_route(dt, ref, int(bool(FORCE_STREAM) or cell in STREAM_CELLS)))
    if route <= 0:
        _engine._check(route if route < 0 else -1)
    sigma = torch.empty(images, dtype=d.dtype, device=d.device)
    sigma64 = torch.empty(images, dtype=torch.float64, device=d.device)
    stats = torch.empty((images, 2), dtype=d.dtype, device=d.device) if want_stats else None
    ws_bytes = int(_lib().mifwt_estim_select_workspace(dt, ref, route))
    _engine._run("estim_sigma", route, (images, band[4]), band[0], _lib().mifwt_estim_sigma,
                 (dt, ref, route, stats.data_ptr() if want_stats else None, sigma.data_ptr(), sigma64.data_ptr()), ws_bytes=ws_bytes)
    return sigma, sigma64, stats


def _order_stats(d: torch.Tensor, lead: int = 0) -> torch.Tensor:
    """The order statistics of ``|d|`` of rank ``(c - 1) // 2`` and ``c // 2`` per leading index, shape ``d.shape[:lead] + (2,)`` (tests)."""
    _check_dtype(d)
    _check_count(d, lead)
    _engine._require_gpu(d)
    return _select(d, lead, want_stats=True)[2].reshape(tuple(d.shape[:lead]) + (2,))


def _sigma_of(d: torch.Tensor, lead: int):
    """(sigma [lead shape], sigma as float64 [images]) of the band ``d``; NaN for an empty band (numpy's median of nothing), no launch."""
    _check_count(d, lead)
    _engine._require_gpu(d)
    shape = tuple(d.shape[:lead])
    images = math.prod(shape)
    if d.numel() == 0:
        sigma = torch.full(shape, float("nan"), dtype=d.dtype, device=d.device)
        return sigma, sigma.reshape(-1).double()
    sigma, sigma64, _ = _select(d, lead)
    return sigma.reshape(shape), sigma64


def estimate_sigma(data, *, lead: Optional[int] = None) -> torch.Tensor:
    """The noise level ``median(|d|) / 0.6744897501960817`` of a detail tensor, or of the finest all-high band of a coefficient
    container: the last tensor of a ``wavedec`` / ``swt`` list, ``.diagonal`` of the last ``WaveletDetailTuple2d``, key ``"d" * ndim``
    of the last dict.  One value per leading index: for a container ``lead`` is the band's rank minus the transformed axes, for a bare
    tensor 0 (one value) unless given.  Returns a detached tensor of shape ``d.shape[:lead]`` in the data's dtype on its device.

    The median is numpy's (even counts: the mean of the two middle order statistics, which are exact; mean and division in float64,
    rounded once).  Zeros are not masked out, unlike scikit-image.  A zero-size leading axis gives an empty result, an empty band NaN,
    both without a launch.  ``ValueError`` for complex, 16-bit, integer or bool data and for 2^31 elements per leading index or more;
    ``RuntimeError`` for a CPU tensor."""
    d, lead = _finest(data, lead)
    return _sigma_of(d, lead)[0]


# ---- thresholds ------------------------------------------------------------------------------------------------------------------
def _composed_moment(t: torch.Tensor, lead: int) -> torch.Tensor:
    """Sum of squares per leading index in float64 from torch operations: beyond the kernels' limits, and the benchmark's emulation."""
    return t.detach().double().pow(2).reshape(math.prod(t.shape[:lead]), -1).sum(-1)


def _details(coeffs, what: str):
    """(the detail tensors of a container in order, every tensor of it)."""
    if not isinstance(coeffs, (list, tuple)) or len(coeffs) < 2 or not isinstance(coeffs[0], torch.Tensor):
        raise TypeError(f"{what}: expected a coefficient container (an approximation followed by detail entries), got {type(coeffs).__name__}")
    leaves: List[torch.Tensor] = []
    owner: List[int] = []
    for i, e in enumerate(coeffs):
        _thr._walk(e, i, leaves, owner)
    return leaves[1:], leaves


def _sigma64_of(sigma, shape: Tuple[int, ...], device) -> torch.Tensor:
    """A given ``sigma`` (a number, a one-element or leading-form tensor) as float64 [images] on the device."""
    images = math.prod(shape)
    if isinstance(sigma, torch.Tensor):
        if sigma.is_complex() or sigma.dtype == torch.bool:
            raise ValueError(f"estimators: sigma must be real, got a {sigma.dtype} tensor")
        if sigma.device != device:
            raise ValueError(f"estimators: a tensor sigma must live on the data's device ({device}), got {sigma.device}")
        if sigma.numel() != 1 and tuple(sigma.shape) != shape:
            raise ValueError(f"estimators: a tensor sigma has one element or the leading shape of the data, {shape}: got {tuple(sigma.shape)}")
        s = sigma.detach().to(torch.float64).reshape(-1)
        return s.expand(images).contiguous() if s.numel() != images else s.contiguous()
    if isinstance(sigma, numbers.Real) and not isinstance(sigma, bool):
        if not float(sigma) >= 0.0:
            raise ValueError(f"estimators: sigma must be non-negative, got {sigma}")
        return torch.full((images,), float(sigma), dtype=torch.float64, device=device)
    raise ValueError(f"estimators: sigma must be None, a number or a tensor, got {type(sigma).__name__}")


def _thresholds(coeffs, method: str, sigma, n, what: str, moments_out: Optional[list] = None):
    """The work of :func:`estimate_thresholds`: (detail tensors, per detail tensor its threshold tensor in the data's dtype, per detail
    tensor the same values in float64 — what the thresholding launch reads without a cast —, leading shape)."""
    if method not in METHODS:
        raise ValueError(f"{what}: unknown method {method!r}; the methods are {', '.join(METHODS)}")
    details, leaves = _details(coeffs, what)
    for t in leaves:
        _check_dtype(t)
    d, lead = _finest(coeffs, None)
    shape = tuple(d.shape[:lead])
    for t in leaves:
        if t.dtype != d.dtype or t.device != d.device:
            raise ValueError(f"{what}: the tensors of a container share dtype and device")
        if t.dim() <= lead or tuple(t.shape[:lead]) != shape:
            raise ValueError(f"{what}: every tensor of the container must start with the leading shape {shape}, got {tuple(t.shape)}")
    images = math.prod(shape)
    if METHODS[method] == 0:
        if n is None:
            n = sum(t.numel() for t in leaves) // images if images else 1
        if not isinstance(n, numbers.Real) or isinstance(n, bool) or not n >= 1:
            raise ValueError(f"{what}: n must be a count of coefficients, at least 1, got {n!r}")
    given = None if sigma is None else _sigma64_of(sigma, shape, d.device)
    for t in leaves:
        _engine._require_gpu(t)
    sigma64 = _sigma_of(d, lead)[1] if given is None else given
    nd = len(details)
    thr = torch.empty((nd, images), dtype=d.dtype, device=d.device)
    thr64 = torch.empty((nd, images), dtype=torch.float64, device=d.device)
    mom = torch.empty((nd, images), dtype=torch.float64, device=d.device) if moments_out is not None else None
    if moments_out is not None:
        moments_out.append(mom)
    if images > 0:
        dt = _engine._DTYPE_IDS[d.dtype]
        cap = max_segments()
        if METHODS[method] == 0:
            factor = math.sqrt(2.0 * math.log(n))
            for c0 in range(0, nd, cap):
                k = min(cap, nd - c0)
                _engine._run("estim_visu", KID_VISU, (k, images), d, _lib().mifwt_estim_thresholds,
                             (dt, 0, None, k, images, sigma64.data_ptr(), factor, thr[c0:].data_ptr(), thr64[c0:].data_ptr(), None), ws_bytes=0)
        else:
            eps = float(torch.finfo(d.dtype).eps)
            kernel, keep = [], []
            for i, t in enumerate(details):
                band = _band(t.detach(), lead) if t.numel() else None
                if band is not None:
                    kernel.append(i)
                    keep.append(band)
                    continue
                # an empty band (NaN, the mean of nothing) or one beyond the kernels' limits: composed
                s2 = sigma64 * sigma64
                m2 = _composed_moment(t, lead) / (t.numel() // images) if t.numel() else torch.full_like(sigma64, float("nan"))
                if mom is not None:
                    mom[i] = m2 * (t.numel() // images)
                thr[i] = (s2 / torch.sqrt(torch.clamp(m2 - s2, min=eps))).to(d.dtype)
                thr64[i] = thr[i].double()
            # runs of consecutive detail tensors, so that a launch writes consecutive rows of thr / thr64
            run: List[int] = []
            runs: List[List[int]] = []
            for j, i in enumerate(kernel):
                if run and (kernel[j - 1] != i - 1 or len(run) == cap):
                    runs.append(run)
                    run = []
                run.append(j)
            if run:
                runs.append(run)
            for run in runs:
                k = len(run)
                arr = (_engine.EstimBand * k)()
                for b, j in zip(arr, run):
                    _fill(b, keep[j])
                units = int(_lib().mifwt_estim_moments_plan(dt, arr, k, images))
                if units < 0:
                    _engine._check(units)
                i0 = kernel[run[0]]
                _engine._run("estim_bayes", KID_MOMENTS, (k, images), d, _lib().mifwt_estim_thresholds,
                             (dt, 1, arr, k, images, sigma64.data_ptr(), 0.0, thr[i0:].data_ptr(), thr64[i0:].data_ptr(),
                              mom[i0:].data_ptr() if mom is not None else None), ws_bytes=8 * units)
    return details, [thr[i].reshape(shape) for i in range(nd)], [thr64[i].reshape(shape) for i in range(nd)], shape


def _nest(coeffs, per_detail: Sequence[torch.Tensor]) -> list:
    it = iter(per_detail)
    return [None] + [_thr._rebuild(e, it) for e in coeffs[1:]]


def estimate_thresholds(coeffs, method: str = "bayes", sigma=None, *, n=None) -> list:
    """VisuShrink / BayesShrink thresholds of a coefficient container, as scikit-image's ``denoise_wavelet`` computes them, in the
    nesting of the container: ``None`` for the approximation, and for every detail tensor a leading-form tensor (one threshold per
    leading index, the data's dtype, on the device, detached) where the container has that tensor.

    ``sigma``: ``None`` (:func:`estimate_sigma` of the container), a number, or a one-element / leading-form tensor.
    ``"visu"``: ``sigma sqrt(2 ln n)`` for every detail tensor, ``n`` the number of coefficients per leading index over the whole
    container unless given.  ``"bayes"``: per detail tensor and leading index ``sigma^2 / sqrt(max(mean(d^2) - sigma^2, eps))`` with the
    machine epsilon of the data's dtype (scikit-image's ``_bayes_thresh``); the sums of squares in float64, in a fixed order.
    ``ValueError`` for an unknown method and for complex, 16-bit or bool data; ``RuntimeError`` for CPU tensors."""
    _, thr, _, _ = _thresholds(coeffs, method, sigma, n, "estimate_thresholds")
    return _nest(coeffs, thr)


def _band_moments(coeffs) -> list:
    """Sum of squares per detail tensor and leading index (float64), in the nesting of the container (tests)."""
    out: list = []
    _, thr, _, shape = _thresholds(coeffs, "bayes", 1.0, None, "estimate_thresholds", moments_out=out)
    return _nest(coeffs, [out[0][i].reshape(shape) for i in range(len(thr))])


_MODES = {"soft": 0, "hard": 1, "garrote": 2, "firm": _thr.FIRM}


def shrink(coeffs, method: str = "bayes", mode: str = "soft", sigma=None, *, n=None):
    """``coeffs`` with every detail tensor shrunk by its own threshold of :func:`estimate_thresholds` — the whole denoising step between
    a decomposition and its reconstruction.  Returns the container of ``coeffs`` (same types, keys, named tuples) over fresh tensors;
    the approximation is the same object.  ``mode`` is ``"soft"``, ``"hard"``, ``"garrote"`` or ``"firm"``; firm thresholding uses
    ``value_low`` = the threshold and ``value_high = 2 * value_low``.  The thresholds are read on the device by the thresholding launch
    (``thresholding.py``), all detail tensors of a dtype in one launch.  Differentiable w.r.t. the data; the thresholds are constants
    (the estimators see detached data)."""
    if mode not in _MODES:
        raise ValueError(f"shrink: unknown mode {mode!r}; the modes are {', '.join(_MODES)}")
    details, _, thr64, _ = _thresholds(coeffs, method, sigma, n, "shrink")
    m = _MODES[mode]
    his64 = None
    if m == _thr.FIRM and thr64:
        twice = 2.0 * torch.stack(thr64)  # (one launch for every band's high threshold)
        his64 = [twice[i] for i in range(len(thr64))]
    outs: List[Optional[torch.Tensor]] = [None] * len(details)
    work = []
    for i, t in enumerate(details):
        if t.numel() == 0:
            outs[i] = torch.empty(t.shape, dtype=t.dtype, device=t.device)
        elif not _thr._kernel_takes(t, (_thr._lead(thr64[i], t), _thr._lead(his64[i], t) if his64 is not None else 0)):
            outs[i] = _thr._composed(t, thr64[i], None if his64 is None else his64[i], m, 0.0)
        else:
            work.append(i)
    if work:
        xs = [details[i] for i in work]
        los = [thr64[i] for i in work]
        his = None if his64 is None else [his64[i] for i in work]
        if torch.is_grad_enabled() and any(x.requires_grad for x in xs):
            vts = los + (his or [])
            cfg = (m, 0.0, tuple(range(len(los))), None if his is None else tuple(range(len(los), 2 * len(los))), len(xs))
            ys = _thr._Thresh.apply(cfg, *xs, *vts)
        else:
            ys = _thr._launches(xs, los, his, m, 0.0)
        for i, y in zip(work, ys):
            outs[i] = y
    it = iter(outs)
    return type(coeffs)([coeffs[0]] + [_thr._rebuild(e, it) for e in coeffs[1:]])
