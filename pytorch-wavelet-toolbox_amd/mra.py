"""Multiresolution analysis: ``mra`` / ``imra`` (``pywt.mra`` / ``pywt.imra``, MATLAB's ``modwtmra``; the reference has none).

    parts = ptwt_amd.mra(x, "db4", level=5)          # [S_5, D_5, ..., D_1], every entry of x's shape
    trend, fine = parts[0], parts[-1]
    x_again = ptwt_amd.imra(parts)

An MRA splits a signal into ``level + 1`` signals of its own shape that add up to it again: the smooth ``S_n`` is the reconstruction from
``cA_n`` alone, the detail ``D_j`` the reconstruction from ``cD_j`` alone.  The analysis is this package's ``swt`` (default, as in
PyWavelets) or ``wavedec``; the projection of ALL bands is ONE HIP launch (C ABI ``mifwt_mra_swt`` / ``mifwt_mra_dwt``, include/mifwt.h;
kernels csrc/mifwt_mra.hip, ids 63 / 64): a band's cascade of one-input synthesis stages runs in LDS, every band is read once and every
component written once.  The bands are taken as the analysis hands them out (views with their own row strides; nothing is copied).

:func:`_composed` is the definition written with the public calls — ``level + 1`` zero-filled containers through ``iswt`` /
``waverec``.  It serves filters longer than 20 taps, 16-bit and complex data, learnable or device-resident filter banks, every call
that wants a gradient (so gradients of any order exist), the cells of ``COMPOSED_CELLS``, a component deeper than the launch takes
(:func:`max_depth`; the rest of that call stays on the launch), and the benchmark (tools/mra_bench.py) as the emulation the launch is
measured against.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Union

import torch

from . import _engine, _fwt
from ._wavelets import device_bank, host_taps
from .constants import Wavelet
from .conv_transform import wavedec, waverec
from .stationary_transform import iswt, swt

__all__ = ["mra", "imra"]

KID_MRA_SWT, KID_MRA_DWT = 63, 64
_TRANSFORMS = {"swt": 0, "dwt": 1}  # MIFWT_MRA_SWT / MIFWT_MRA_DWT
FORCE_COMPOSED = False  # True: every call takes the composed route (the launch's cross-check and timing baseline)
#: (transform, dtype, "short" / "long": rows of at most / more than :func:`tile` samples) cells that stay on the composed route: a cell
#: belongs here unless tools/mra_bench.py has shown the launch's median ahead of the composition's by more than the widest spread of
#: its windows (EXPERIMENTS part A); a cell that was not measured is listed too.
COMPOSED_CELLS: set = set()

_entries = None


def _lib():
    global _entries
    if _entries is None:
        _entries = _engine.private_entries(_engine.MRA_ENTRIES)
    return _entries


def tile() -> int:
    """Outputs per workgroup of the launch (``mifwt_mra_tile``)."""
    return int(_lib().mifwt_mra_tile())


def max_depth(dtype: torch.dtype, filt_len: int, transform: str = "swt") -> int:
    """The deepest component (number of synthesis stages) the launch takes (``mifwt_mra_max_depth``; needs no device): for ``"swt"`` the
    largest ``j`` with ``(2^j - 1)(L - 1) <= 2048``, for ``"dwt"`` 32; 0 where the launch does not serve the dtype or the length."""
    if transform not in _TRANSFORMS:
        raise ValueError(f"mra: transform must be 'swt' or 'dwt', got {transform!r}")
    if dtype not in _engine._DTYPE_IDS or filt_len < 2 or filt_len % 2:
        return 0
    return max(0, int(_lib().mifwt_mra_max_depth(_engine._DTYPE_IDS[dtype], filt_len, _TRANSFORMS[transform])))


def _analysis(data, wavelet, level, axis, transform, mode) -> List[torch.Tensor]:
    if transform == "swt":
        return swt(data, wavelet, level, axis=axis)
    return wavedec(data, wavelet, mode=mode, level=level, axis=axis)


def _only(coeffs: Sequence[torch.Tensor], i: int) -> List[torch.Tensor]:
    return [c if k == i else torch.zeros_like(c) for k, c in enumerate(coeffs)]


def _component(coeffs: Sequence[torch.Tensor], i: int, wavelet, axis, transform, mode, extent: int) -> torch.Tensor:
    """Component ``i`` from the public synthesis of a container whose other entries are zeros."""
    if transform == "swt":
        return iswt(_only(coeffs, i), wavelet, axis=axis)
    return waverec(_only(coeffs, i), wavelet, mode=mode, axis=axis).narrow(axis, 0, extent)


def _composed(data, wavelet, level, axis, transform, mode) -> List[torch.Tensor]:
    """The definition, literally: the analysis, then per band the synthesis of a container in which every other band is
    ``torch.zeros_like``.  Whatever these calls raise is what the call raises."""
    coeffs = _analysis(data, wavelet, level, axis, transform, mode)
    if len(coeffs) == 1:
        return [data]
    return [_component(coeffs, i, wavelet, axis, transform, mode, data.shape[axis]) for i in range(len(coeffs))]


def _regime(n: int) -> str:
    return "short" if n <= tile() else "long"


def _fused_bank(data: torch.Tensor, wavelet):
    """(rec_lo, rec_hi) as host floats where the launch serves the call's data and filter bank, else None."""
    if not isinstance(data, torch.Tensor) or not data.is_cuda or data.dtype not in (torch.float32, torch.float64):
        return None
    if torch.is_grad_enabled() and data.requires_grad:
        return None
    if _fwt._tap_tensors(wavelet) is not None or device_bank(wavelet, data.device) is not None:
        return None
    dec_lo, _, rec_lo, rec_hi = host_taps(wavelet)
    flen = len(rec_lo)
    if flen != len(dec_lo) or flen != len(rec_hi) or flen % 2 or not max_depth(data.dtype, flen):
        return None
    return rec_lo, rec_hi


def _project(coeffs: Sequence[torch.Tensor], depths: Sequence[int], level_len: Optional[Sequence[int]], n: int, rec_lo, rec_hi,
             circular: bool = False, out: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """The launch.  ``coeffs[i]`` is a folded band ``[B, len]`` or None (a component that is not this launch's); ``depths[i]`` its number
    of stages; entry 0 starts with ``rec_lo``, the others with ``rec_hi``.  ``level_len``: the row length per level of a decimated
    decomposition (None: stationary).  Fills and returns ``out`` ``[len(coeffs), B, n]`` (allocated here unless given: any component
    and row strides, unit innermost stride) or returns None where the entry refuses the call (nothing launched)."""
    anchor = next(c for c in coeffs if c is not None)
    rows = anchor.shape[0]
    if out is None:
        out = torch.empty((len(coeffs), rows, n), dtype=anchor.dtype, device=anchor.device)
    work = [(i, _engine._unit_last(c)) for i, c in enumerate(coeffs) if c is not None]
    if out.numel() == 0:
        return out
    arr = (_engine.MraBand * len(work))()
    for slot, (i, c) in zip(arr, work):
        slot.x, slot.row_stride, slot.index, slot.depth, slot.detail = c.data_ptr(), c.stride(0), i, depths[i], int(i > 0)
    dt, flen = _engine._DTYPE_IDS[anchor.dtype], len(rec_lo)
    tail = (arr, len(work), out.data_ptr(), out.stride(0), out.stride(1), _engine._taps_array(rec_lo), _engine._taps_array(rec_hi))
    if level_len is None:
        rc = _engine._run("mra_swt", KID_MRA_SWT, (rows, n), anchor, _lib().mifwt_mra_swt, (dt, flen, rows, n, *tail), may_refuse=True)
    else:
        lens = (ctypes.c_int64 * len(level_len))(*level_len)
        rc = _engine._run("mra_dwt", KID_MRA_DWT, (rows, n), anchor, _lib().mifwt_mra_dwt,
                          (dt, flen, int(circular), rows, lens, len(level_len) - 1, *tail), may_refuse=True)
    return None if rc else out


def mra(data: torch.Tensor, wavelet: Union[Wavelet, str], level: Optional[int] = None, *, axis: int = -1, transform: str = "swt",
        mode: str = "periodization") -> List[torch.Tensor]:
    """Multiresolution analysis along ``axis``: ``[S_n, D_n, ..., D_1]``, every entry of ``data``'s shape, dtype and device, and their
    sum is ``data`` again (:func:`imra`).  The entries may be views of one backing allocation ``[n + 1, ...]``: clone an entry before
    writing to it in place if the others are still needed.

    ``transform="swt"`` (default, as in ``pywt.mra``): ``c = swt(data, wavelet, level, axis=axis)``; component ``i`` is ``iswt`` of ``c``
    with every entry but ``c[i]`` replaced by zeros.  ``mode`` is ignored, ``level=None`` is ``swt``'s default, and any length and level
    that ``swt`` takes is valid.  The components do not depend on PyWavelets' ``norm``: the per-level factors cancel.

    ``transform="dwt"``: ``c = wavedec(data, wavelet, mode=mode, level=level, axis=axis)``; component ``i`` is ``waverec`` of ``c`` with
    the others zeroed, cropped to ``data``'s extent (an odd extent comes back one sample longer).  Every mode of ``wavedec``.

    ``level=0`` (or a default level of 0) gives ``[data]``.  ``ValueError`` for another ``transform``; every other error is the one the
    analysis call raises.  On a ROCm device, float32 / float64 data and an even filter length up to 20, all components are ONE HIP
    launch after the analysis (no host read: the call can be captured); a component deeper than :func:`max_depth` is composed while
    the others stay on the launch.  Longer filters, 16-bit and complex data, learnable or device-resident filter banks and calls on data
    that requires grad (while grad is enabled) are composed from the public calls, so gradients of any order exist."""
    if transform not in _TRANSFORMS:
        raise ValueError(f"mra: transform must be 'swt' or 'dwt', got {transform!r}")
    bank = None if FORCE_COMPOSED else _fused_bank(data, wavelet)
    if bank is None or not isinstance(axis, int) or not -data.dim() <= axis < data.dim():
        return _composed(data, wavelet, level, axis, transform, mode)
    n = data.shape[axis]
    if (transform, data.dtype, _regime(n)) in COMPOSED_CELLS:
        return _composed(data, wavelet, level, axis, transform, mode)
    with torch.no_grad():
        coeffs = _analysis(data, wavelet, level, axis, transform, mode)
        nb = len(coeffs)
        if nb == 1:
            return [data]
        layout = _fwt._Layout(data, 1, (axis,))
        depths = [nb - 1] + [nb - i for i in range(1, nb)]
        deepest = max_depth(data.dtype, len(bank[0]), transform)
        cap = int(_lib().mifwt_mra_max_bands())
        fused = [i for i in range(nb) if depths[i] <= deepest][-cap:]
        out = None
        if fused:
            folded = [layout.fold(c) if i in fused else None for i, c in enumerate(coeffs)]
            level_len = None if transform == "swt" else [n] + [int(c.shape[axis]) for c in coeffs[:0:-1]]
            out = _project(folded, depths, level_len, n, bank[0], bank[1], circular=mode == "periodization")
        parts = []
        for i in range(nb):
            if out is not None and i in fused:
                parts.append(layout.unfold(out[i]))
            else:
                parts.append(_component(coeffs, i, wavelet, axis, transform, mode, n))
        return parts


def imra(mra_coeffs: Sequence[torch.Tensor]) -> torch.Tensor:
    """The signal of its multiresolution components: the left-to-right sum ``((S_n + D_n) + ...) + D_1`` (``pywt.imra``).  Plain torch
    on any device.  ``ValueError`` for an empty list or for entries that differ in shape, dtype or device."""
    parts = list(mra_coeffs)
    if not parts:
        raise ValueError("imra: an empty list has no sum")
    first = parts[0]
    for t in parts:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"imra: expected tensors, got {type(t).__name__}")
        if t.shape != first.shape or t.dtype != first.dtype or t.device != first.device:
            raise ValueError(f"imra: the components must share shape, dtype and device; got {tuple(t.shape)} {t.dtype} {t.device} next to "
                             f"{tuple(first.shape)} {first.dtype} {first.device}")
    total = first
    for t in parts[1:]:
        total = total + t
    return total
