"""Padding-free 3-D fast wavelet transform with boundary filters: ``MatrixWavedec3`` / ``MatrixWaverec3`` (API of reference
src/ptwt/matmul_transform_3.py): a level applies the level operator of ``matmul_transform.py`` along width, height and depth and
splits the result into ``aaa`` and the seven detail bands ``"aad" .. "ddd"`` (``x`` = depth, ``y`` = height, ``z`` = width in a key
``"xyz"``, ``d`` = high-pass).

The reference runs a level as three batched sparse products with transposes between them; here it is ONE fused HIP launch (C ABI
``mifwt_bwt3_fwd`` / ``mifwt_bwt3_inv``, csrc/mifwt_bwt3.hip) that reads the volume once and writes the eight bands to their final
planes, for float32 / float64 and filters of up to 8 taps; longer filters run the per-axis passes of the 1-D / 2-D classes, seven
launches per level; levels with an axis of a few dozen samples are dense products (``_bwt.py``).  The boundary filters come from the
same small tables as in 1-D (``_boundary.py``).  The sign convention of the boundary filters — the Gram-Schmidt sign for both
``orthogonalization`` values, unlike the reference's ``"qr"`` — is described in ``matmul_transform.py``.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _bwt, _engine, _fwt
from ._wavelets import as_wavelet
from .constants import Wavelet, WaveletCoeffNd
from .matmul_transform import _bank_taps, _deprecated_alias, _mode_for, _plan_levels, _synthesis_extents

__all__ = ["MatrixWavedec3", "MatrixWaverec3"]

_KEYS = _fwt._KEYS_ND[3]  # detail s (1 .. 7) has key _KEYS[s - 1]: bit 2 of s = depth, bit 1 = height, bit 0 = width high-pass


class MatrixWavedec3:
    """3-D fast wavelet transform with boundary filters instead of padding (drop-in for ``ptwt.MatrixWavedec3``).  Returns
    ``(aaa, {"aad": ..., ..., "ddd": ...}, ...)``, coarsest level first, with the keys of ``wavedec3``.  ``pad_list`` holds
    (depth, height, width) tuples — the 2-D class keeps (width, height), as the reference does.  Both ``orthogonalization`` values give
    the same coefficients, with every boundary filter in its Gram-Schmidt sign (see ``matmul_transform.py`` for how that differs from
    the reference's ``"qr"``)."""

    @_deprecated_alias(boundary="orthogonalization")
    def __init__(self, wavelet: Union[Wavelet, str], level: Optional[int] = None, *, axes: _fwt.AxisHint = None,
                 orthogonalization: str = "qr", odd_coeff_padding_mode: str = "zero"):
        self.wavelet = as_wavelet(wavelet)
        self.level = level
        self.orthogonalization = orthogonalization
        self.odd_coeff_padding_mode = odd_coeff_padding_mode
        self.axes = _fwt._ensure_axes(axes, 3)
        self.input_signal_shape: Optional[Tuple[int, int, int]] = None
        self.pad_list: List[Tuple[bool, bool, bool]] = []
        self.size_list: List[Tuple[int, int, int]] = []
        self.padded = False
        self._built = False
        self._taps = _bank_taps(self.wavelet, orthogonalization)
        self._bank = _bwt.bank(self._taps, orthogonalization, "analysis")

    def __call__(self, input_signal: torch.Tensor) -> WaveletCoeffNd:
        layout = _fwt._Layout(input_signal, 3, self.axes)
        x = layout.fold(input_signal)
        shape = tuple(int(s) for s in x.shape[-3:])
        re_build = False
        if self.input_signal_shape != shape:
            self.input_signal_shape = shape
            re_build = True
        if self.level is None:
            wlen = self._bank.filt_len
            self.level = int(np.min([np.log2(n / (wlen - 1)) for n in shape]))
            re_build = True
        elif self.level <= 0:
            raise ValueError("level must be a positive integer.")
        if not self._built or len(self.size_list) < 2 or re_build:
            self.size_list, self.pad_list, self.padded = _plan_levels(self.level, shape, self._bank.filt_len)
            self._built = True
        nlevels = len(self.size_list) - 1
        extents = [shape] + [tuple(n // 2 for n in s) for s in self.size_list[: max(nlevels - 1, 0)]]
        mode_id = _mode_for(extents[:nlevels], self.odd_coeff_padding_mode)
        _engine._require_gpu(x)
        lll = x
        split_list = []
        for _ in range(nlevels):
            buf = _bwt.rows(lll, self._bank, mode_id)
            lll = buf[:, 0]
            split_list.append({key: layout.unfold(buf[:, s + 1]) for s, key in enumerate(_KEYS)})
        split_list.reverse()
        return (layout.unfold(lll), *split_list)


class MatrixWaverec3:
    """Inverse of :class:`MatrixWavedec3` (drop-in for ``ptwt.MatrixWaverec3``).  The samples appended to odd approximations are
    dropped between levels but not after the last one, so the output of a padded transform has the even shape, as in the reference.

    One deliberate difference: the reference's ``__call__`` writes ``"aaa"`` into the caller's detail dicts, so a second call on the
    same coefficients fails there; this class does not modify its input.  The boundary filters carry the Gram-Schmidt sign for both
    ``orthogonalization`` values (``matmul_transform.py``)."""

    @_deprecated_alias(boundary="orthogonalization")
    def __init__(self, wavelet: Union[Wavelet, str], *, axes: _fwt.AxisHint = None, orthogonalization: str = "qr"):
        self.wavelet = as_wavelet(wavelet)
        self.orthogonalization = orthogonalization
        self.axes = _fwt._ensure_axes(axes, 3)
        self.level: Optional[int] = None
        self.input_signal_shape: Optional[Tuple[int, int, int]] = None
        self.padded = False
        self._taps = _bank_taps(self.wavelet, orthogonalization)
        self._bank = _bwt.bank(self._taps, orthogonalization, "synthesis")

    def __call__(self, coefficients: WaveletCoeffNd) -> torch.Tensor:
        coefficients = tuple(coefficients)
        if not coefficients or not isinstance(coefficients[0], torch.Tensor):
            raise ValueError("First element of coeffs must be the approximation coefficient tensor.")
        if len(coefficients) > 1 and not isinstance(coefficients[-1], dict):
            raise ValueError("Waverec3 expects dicts of tensors.")
        layout = _fwt._Layout(coefficients[0], 3, self.axes)
        flat = [coefficients[0]]
        ordered: List[Dict[str, torch.Tensor]] = []
        for c in coefficients[1:]:
            if not isinstance(c, dict) or len(c) != 7 or not all(isinstance(t, torch.Tensor) for t in c.values()):
                raise ValueError(f"Unexpected detail coefficient type: {type(c)}. Detail coefficients must be a dict containing 7 "
                                 "tensors as returned by MatrixWavedec3.")
            if set(c) != set(_KEYS):
                raise ValueError(f"Unexpected detail keys {sorted(c)}: a level holds exactly {list(_KEYS)}.")
            flat.extend(c.values())
            ordered.append(c)
        _fwt._check_same_device_dtype(flat)
        lll = layout.fold(coefficients[0])
        levels = [[layout.fold(c[key]) for key in _KEYS] for c in ordered]  # (a new list per level: the caller's dicts stay as they are)
        level = len(levels)
        if level:
            shape = tuple(int(s) * 2 for s in levels[-1][-1].shape[-3:])
            if self.input_signal_shape != shape or self.level != level:
                self.input_signal_shape, self.level = shape, level
                _, _, self.padded = _plan_levels(level, shape, self._bank.filt_len)
        out_extents = _synthesis_extents(lll.shape, levels, "All coefficients on each level must have the same shape")
        _engine._require_gpu(lll)
        for bands, ext in zip(levels, out_extents):
            lll = _bwt.transposed([lll] + bands, self._bank, ext)
        return layout.unfold(lll)
