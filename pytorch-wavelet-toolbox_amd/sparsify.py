"""Top-k sparsification on the device — keep the ``k`` largest coefficients of every image, drop the rest (C ABI ``mifwt_select_*``,
include/mifwt.h; kernels csrc/mifwt_select.hip, ids 54 / 55).

    coeffs = ptwt_amd.wavedec2(x, "db4", level=3)
    sparse = ptwt_amd.sparsify(coeffs, 0.05)                 # the largest 5 % of the detail coefficients of every image survive
    y = ptwt_amd.waverec2(sparse, "db4")
    v = ptwt_amd.keep_threshold(coeffs, 1000)                # the 1000-th largest detail magnitude per image

All pooled tensors of one leading index (one image, as in ``estimate_thresholds``) form ONE multiset of ``n`` magnitudes.
``keep_threshold`` is ``s[n - k]`` with ``s`` the ascending sort of ``|c|``: the k-th largest magnitude, EXACT — a radix selection on the
bit patterns with the sign cleared, the bits a sort gives.  ``sparsify`` is :func:`ptwt_amd.threshold` with that value for every pooled
tensor: with ``"hard"`` an element survives iff ``|x| >= v_k``, so at least ``k`` survive per image and exactly ``k`` where the magnitude
``v_k`` is not tied.  ``k = 0`` and an empty pool give ``+inf``.  NaN inputs are unspecified.

``keep`` is a Python ``int`` (``k`` itself, ``0 <= k <= n``), a Python ``float`` (a fraction in [0, 1]: ``k = min(n, floor(keep n + 0.5))``)
or an int64 device tensor with one element or of the leading shape (one ``k`` per image, read on the device when the kernel runs and
clipped to [0, n] there).  Everything is written on the device and enqueued on the caller's stream: nothing is copied to the host,
nothing synchronises, a call can be captured (``ptwt_amd.capture``) and a replay sees the data and the ``keep`` tensor of its own run.
Integer counters only: two runs give the same bits.

Two routes select.  A pool of at most ``estimators.lds_capacity`` elements per image in at most :func:`max_segments` tensors is selected
by one workgroup from keys held in LDS (id 54); anything else by digit passes over all tensors with per-workgroup LDS histograms flushed
into integer counters (id 55), ``max_segments`` tensors per launch.  ``FORCE_STREAM`` sends every size down the second route (tests,
tools).  Limits: the collapsed form of ``thresholding._form``, beyond which the value is composed from torch operations
(:func:`_composed_kth`), and fewer than 2^31 pooled elements per image: ``ValueError`` from there on (the composition is ``torch.sort``,
which takes at most 2^31 - 1 elements along the sorted axis).  float32 and float64 data only.

The package exports the FUNCTION under this module's name, so ``ptwt_amd.sparsify`` is :func:`sparsify`; the module and its switches
are reached with ``importlib.import_module("ptwt_amd.sparsify")``.
"""
from __future__ import annotations

import math
import numbers
from typing import List, Optional, Sequence, Tuple

import torch

from . import _engine
from . import estimators as _est
from . import thresholding as _thr

__all__ = ["keep_threshold", "sparsify"]

KID_KTH_LDS, KID_KTH_STREAM = 54, 55
MODES = {"hard": 1, "soft": 0, "garrote": 2}
#: test / tool switch: the streaming selection (id 55) at every size
FORCE_STREAM = False
#: (dtype, pooled elements per leading index) cells inside the LDS route's envelope that take the streaming selection all the same, and
#: cells whose value comes from the torch composition (a sort) instead of the kernels: a cell belongs there only where
#: tools/sparsify_bench.py has shown the default's median behind by more than the spread of its windows.  Empty: the LDS-resident selection led the streaming one, and both led the sort, in every cell measured (EXPERIMENTS part K).
STREAM_CELLS: set = set()
COMPOSED_CELLS: set = set()
_COUNT_LIMIT = 1 << 31
_DTYPES = (torch.float32, torch.float64)

_entries = None


def _lib():
    global _entries
    if _entries is None:
        _entries = _engine.private_entries(_engine.SELECT_ENTRIES)
    return _entries


def max_segments() -> int:
    """Tensors one selection launch takes (``mifwt_select_max_segments``)."""
    return int(_lib().mifwt_select_max_segments())


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def _check_dtype(t: torch.Tensor) -> None:
    if t.dtype not in _DTYPES:
        raise ValueError(f"sparsify: float32 and float64 data only, got {t.dtype}")


def _k_of(keep, n: int) -> int:
    """``k`` of a Python number ``keep`` for a pool of ``n``: an int is ``k`` itself, a float a fraction, ``min(n, floor(keep n + 0.5))``."""
    if isinstance(keep, bool):
        raise ValueError("sparsify: keep must be an int, a float or an int64 tensor, got bool")
    if isinstance(keep, numbers.Integral):
        if not 0 <= keep <= n:
            raise ValueError(f"sparsify: an int keep is a count in [0, {n}] (the pooled coefficients per image), got {keep}")
        return int(keep)
    if isinstance(keep, numbers.Real):
        if not 0.0 <= float(keep) <= 1.0:
            raise ValueError(f"sparsify: a float keep is a fraction in [0, 1], got {keep}")
        return min(n, int(math.floor(float(keep) * n + 0.5)))
    raise ValueError(f"sparsify: keep must be an int, a float or an int64 tensor, got {type(keep).__name__}")


def _keep(keep, n: int, shape: Tuple[int, ...], device):
    """``keep`` as (k, None) or (0, the int64 tensor the kernel reads, flat)."""
    if not isinstance(keep, torch.Tensor):
        return _k_of(keep, n), None
    if keep.dtype != torch.int64:
        raise ValueError(f"sparsify: a tensor keep holds int64 counts, got {keep.dtype}")
    if keep.device != device:
        raise ValueError(f"sparsify: a tensor keep must live on the data's device ({device}), got {keep.device}")
    if keep.numel() != 1 and tuple(keep.shape) != shape:
        raise ValueError(f"sparsify: a tensor keep has one element or the leading shape of the data, {shape}: got {tuple(keep.shape)}")
    return 0, keep.detach().reshape(-1).contiguous()


def _pool(coeffs, approx: bool, lead: Optional[int]):
    """(every tensor of ``coeffs``, the indices of the pooled ones, leading axes, leading shape, pooled elements per leading index)."""
    leaves, owner, _ = _thr._flatten(coeffs)
    for t in leaves:
        _check_dtype(t)
    d, lead = _est._finest(coeffs, lead)
    shape = tuple(d.shape[:lead])
    for t in leaves:
        if t.dtype != d.dtype or t.device != d.device:
            raise ValueError("sparsify: the tensors of a container share dtype and device")
        if t.dim() < lead or tuple(t.shape[:lead]) != shape:
            raise ValueError(f"sparsify: every tensor of the container must start with the leading shape {shape}, got {tuple(t.shape)}")
    whole = isinstance(coeffs, torch.Tensor) or approx
    pooled = [i for i, e in enumerate(owner) if whole or e != 0]
    n = sum(math.prod(leaves[i].shape[lead:]) for i in pooled)
    return leaves, pooled, lead, shape, n


# ---- the selection ---------------------------------------------------------------------------------------------------------------
def _composed_kth(tensors: Sequence[torch.Tensor], lead: int, k, dk: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The k-th largest magnitude per leading index [images] of the pooled ``tensors`` from torch operations (``cat`` of the flattened
    ``abs``, a full ``sort``): the route beyond the kernels' limits, and the emulation the benchmark compares them with.  ``dk``: the
    flat int64 tensor of :func:`_keep` instead of ``k``."""
    images = math.prod(tensors[0].shape[:lead])
    s = torch.cat([t.detach().abs().reshape(images, -1) for t in tensors], 1).sort(-1).values
    n = s.shape[1]
    if dk is None:
        return s[:, n - k].contiguous() if k > 0 else torch.full((images,), float("inf"), dtype=s.dtype, device=s.device)
    kk = dk.clamp(0, n).expand(images)
    v = s.gather(1, (n - kk.clamp(min=1)).unsqueeze(1)).squeeze(1)
    return torch.where(kk == 0, torch.full_like(v, float("inf")), v)


def _kth(tensors: Sequence[torch.Tensor], lead: int, shape: Tuple[int, ...], n: int, k: int, dk: Optional[torch.Tensor]):
    """(the k-th largest magnitude in the data's dtype [leading shape], the same values in float64 [images]) of the pooled ``tensors``
    (one dtype, one device, ``n`` elements per leading index together)."""
    t0 = tensors[0]
    images = math.prod(shape)
    if images == 0 or n == 0:  # no image: an empty result; an empty pool: the k-th largest of nothing bounds nothing.  No launch.
        v = torch.full(shape, float("inf"), dtype=t0.dtype, device=t0.device)
        return v, v.reshape(-1).double()
    live = [t.detach() for t in tensors if t.numel()]
    bands = [_est._band(t, lead) for t in live]
    cell = (t0.dtype, n)
    if any(b is None for b in bands) or cell in COMPOSED_CELLS:
        v = _composed_kth(live, lead, k, dk)
        return v.reshape(shape), v.double()
    dt = _engine._DTYPE_IDS[t0.dtype]
    arr = (_engine.EstimBand * len(bands))()
    for b, band in zip(arr, bands):
        _est._fill(b, band)
    route = int(_lib().mifwt_select_route(dt, arr, len(bands), images, int(bool(FORCE_STREAM) or cell in STREAM_CELLS)))
    if route <= 0:
        _engine._check(route if route < 0 else -1)
    v = torch.empty(images, dtype=t0.dtype, device=t0.device)
    v64 = torch.empty(images, dtype=torch.float64, device=t0.device)
    ws_bytes = int(_lib().mifwt_select_workspace(dt, arr, len(bands), images, route))
    _engine._run("select_kth", route, (images, n), bands[0][0], _lib().mifwt_select_kth,
                 (dt, arr, len(bands), images, k, dk.data_ptr() if dk is not None else None, int(dk is not None and dk.numel() > 1), route,
                  v.data_ptr(), v64.data_ptr()), ws_bytes=ws_bytes)
    return v.reshape(shape), v64


def _value(coeffs, keep, approx: bool, lead: Optional[int]):
    leaves, pooled, lead, shape, n = _pool(coeffs, approx, lead)
    if n >= _COUNT_LIMIT:  # no kernel takes such a pool, and neither does the sort of the composition
        raise ValueError(f"sparsify: the selection takes fewer than 2^31 pooled coefficients per image, got {n}")
    k, dk = _keep(keep, n, shape, leaves[0].device)
    for t in leaves:
        _engine._require_gpu(t)
    v, v64 = _kth([leaves[i] for i in pooled] or leaves[:1], lead, shape, n, k, dk)
    return leaves, pooled, v, v64.reshape(shape)


def keep_threshold(coeffs, keep, *, approx: bool = False, lead: Optional[int] = None) -> torch.Tensor:
    """The k-th largest magnitude per leading index (per image) of a tensor or of a coefficient container — any container
    :func:`ptwt_amd.threshold` accepts —, the magnitudes of all its tensors pooled: ``s[n - k]``, ``s`` the ascending sort of ``|c|`` of
    the image.  Exact, the bits a sort gives.  With ``approx=False`` entry 0 of a container (the approximation) stays out of the pool; a
    bare tensor is pooled whole.  One value per leading index: for a container ``lead`` is the finest band's rank minus the transformed
    axes, for a bare tensor 0 (one value) unless given, as in :func:`ptwt_amd.estimate_sigma`.  ``keep``: an ``int`` ``k`` in [0, n], a
    ``float`` fraction in [0, 1] (``k = min(n, floor(keep n + 0.5))``), or an int64 device tensor with one element or of the leading
    shape, read on the device and clipped to [0, n] there.  Returns a detached tensor of the leading shape in the data's dtype.

    ``k = 0`` gives ``+inf``; so does an empty pool, without a launch; a zero-size leading axis gives an empty result without a launch.
    NaN inputs are unspecified.  ``ValueError`` for complex, 16-bit, integer or bool data, for tensors that do not share dtype, device and
    leading shape, for any other ``keep`` and for a pool of 2^31 or more elements per image; ``RuntimeError`` for a CPU tensor."""
    return _value(coeffs, keep, approx, lead)[2]


def sparsify(coeffs, keep, mode: str = "hard", *, approx: bool = False):
    """``coeffs`` with every pooled tensor thresholded at :func:`keep_threshold` of its image — ``"hard"``: the ``k`` largest coefficients
    of every image survive (``|x| >= v_k``: at least ``k``, exactly ``k`` where the magnitude ``v_k`` is not tied), the others are 0;
    ``"soft"`` / ``"garrote"`` shrink the survivors as :func:`ptwt_amd.threshold` does.  Returns the container of ``coeffs`` (same types,
    keys, named tuples) over fresh tensors; with ``approx=False`` the approximation is the same object, with ``approx=True`` it is pooled
    and thresholded too.  The selection launches plus one thresholding launch, which reads the values on the device: no host read, so
    the call can be captured.  Differentiable w.r.t. the data; the threshold is a constant (the selection sees detached data).
    ``keep`` and the errors as for :func:`keep_threshold`; ``ValueError`` for any other mode (``"firm"`` is not offered)."""
    if mode not in MODES:
        raise ValueError(f"sparsify: unknown mode {mode!r}; the modes are {', '.join(MODES)}")
    leaves, pooled, _, v64 = _value(coeffs, keep, approx, None)
    m = MODES[mode]
    outs: List[torch.Tensor] = list(leaves)
    work = []
    for i in pooled:
        t = leaves[i]
        if t.numel() == 0:
            outs[i] = torch.empty(t.shape, dtype=t.dtype, device=t.device)
        elif not _thr._kernel_takes(t, (_thr._lead(v64, t), 0)):
            outs[i] = _thr._composed(t, v64, None, m, 0.0)
        else:
            work.append(i)
    if work:
        xs = [leaves[i] for i in work]
        if torch.is_grad_enabled() and any(x.requires_grad for x in xs):
            ys = _thr._Thresh.apply((m, 0.0, (0,) * len(xs), None, len(xs)), *xs, v64)
        else:
            ys = _thr._launches(xs, [v64] * len(xs), None, m, 0.0)
        for i, y in zip(work, ys):
            outs[i] = y
    return _thr._rebuild(coeffs, iter(outs))
