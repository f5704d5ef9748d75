"""Padding-free 2-D fast wavelet transform with boundary filters: ``MatrixWavedec2`` / ``MatrixWaverec2`` (API of reference
src/ptwt/matmul_transform_2.py), in the SEPARABLE form, the reference's default: a level is ``A_rows X A_cols^T`` split into
``ll, (lh, hl, hh)``.

The reference runs a level as two batched sparse products and two transposes; here it is ONE fused HIP launch (C ABI
``mifwt_bwt_fwd`` / ``mifwt_bwt_inv``) that filters both axes through LDS and writes the four bands to their final planes; the
boundary filters come from the same small tables as in 1-D (``_boundary.py``).  The sign convention of the boundary filters — the
Gram-Schmidt sign for both ``orthogonalization`` values, unlike the reference's ``"qr"`` — is described in ``matmul_transform.py``.

``separable=False`` is not built: it orthogonalises the boundary rows of a 2-D Kronecker matrix, which gives different numbers
than the separable form — another transform, not another route to this one.
"""
from __future__ import annotations

from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import _bwt, _engine, _fwt
from ._wavelets import as_wavelet
from .constants import Wavelet, WaveletCoeff2d, WaveletDetailTuple2d
from .matmul_transform import _bank_taps, _deprecated_alias, _mode_for, _plan_levels, _synthesis_extents

__all__ = ["MatrixWavedec2", "MatrixWaverec2"]

_NON_SEPARABLE = ("separable=False is not implemented: the non-separable boundary transform orthogonalises the boundary rows of a 2-D "
                  "Kronecker matrix and yields different coefficients than the separable one; only the separable form (the default) "
                  "is built on this engine.")


class MatrixWavedec2:
    """2-D fast wavelet transform with boundary filters instead of padding (drop-in for ``ptwt.MatrixWavedec2`` with
    ``separable=True``).  Returns ``(ll, WaveletDetailTuple2d(lh, hl, hh), ...)``, coarsest level first.  Both
    ``orthogonalization`` values give the same coefficients, with every boundary filter in its Gram-Schmidt sign (see
    ``matmul_transform.py`` for how that differs from the reference's ``"qr"``)."""

    @_deprecated_alias(boundary="orthogonalization")
    def __init__(self, wavelet: Union[Wavelet, str], level: Optional[int] = None, *, axes: _fwt.AxisHint = None,
                 orthogonalization: str = "qr", separable: bool = True, odd_coeff_padding_mode: str = "zero"):
        self.wavelet = as_wavelet(wavelet)
        self.axes = _fwt._ensure_axes(axes, 2)
        self.level = level
        self.orthogonalization = orthogonalization
        self.odd_coeff_padding_mode = odd_coeff_padding_mode
        self.separable = separable
        self.input_signal_shape: Optional[Tuple[int, int]] = None
        self.pad_list: List[Tuple[bool, bool]] = []
        self.size_list: List[Tuple[int, int]] = []
        self.padded = False
        self._built = False
        self._taps = _bank_taps(self.wavelet, orthogonalization)
        if not separable:
            raise NotImplementedError(_NON_SEPARABLE)
        self._bank = _bwt.bank(self._taps, orthogonalization, "analysis")

    @property
    def sparse_fwt_operator(self) -> torch.Tensor:
        """Separable transforms have no single operator matrix (reference matmul_transform_2.py:352-383)."""
        raise NotImplementedError

    def __call__(self, input_signal: torch.Tensor) -> WaveletCoeff2d:
        layout = _fwt._Layout(input_signal, 2, self.axes)
        x = layout.fold(input_signal)
        height, width = int(x.shape[-2]), int(x.shape[-1])
        re_build = False
        if self.input_signal_shape != (height, width):
            self.input_signal_shape = (height, width)
            re_build = True
        if self.level is None:
            wlen = self._bank.filt_len
            self.level = int(np.min([np.log2(height / (wlen - 1)), np.log2(width / (wlen - 1))]))
            re_build = True
        elif self.level <= 0:
            raise ValueError("level must be a positive integer.")
        if not self._built or len(self.size_list) < 2 or re_build:
            self.size_list, pads, self.padded = _plan_levels(self.level, self.input_signal_shape, self._bank.filt_len)
            # (as in the reference, src/ptwt/matmul_transform_2.py:234-242, a pad tuple is (width padded, height padded))
            self.pad_list, self._built = [p[::-1] for p in pads], True
        nlevels = len(self.size_list) - 1
        extents = [(height, width)] + [(s[0] // 2, s[1] // 2) for s in self.size_list[: max(nlevels - 1, 0)]]
        mode_id = _mode_for(extents[:nlevels], self.odd_coeff_padding_mode)
        _engine._require_gpu(x)
        ll = x
        split_list = []
        for _ in range(nlevels):
            buf = _bwt.rows(ll, self._bank, mode_id)
            ll = buf[:, 0]
            # band s: bit 1 = high-pass along the rows axis, bit 0 = along the columns axis: lh = 1, hl = 2, hh = 3
            split_list.append(WaveletDetailTuple2d(*(layout.unfold(buf[:, s]) for s in (1, 2, 3))))
        split_list.reverse()
        return (layout.unfold(ll), *split_list)


class MatrixWaverec2:
    """Inverse of :class:`MatrixWavedec2` (drop-in for ``ptwt.MatrixWaverec2`` with ``separable=True``).  The samples appended to odd
    approximations are dropped between levels but not after the last one, as in the reference."""

    @_deprecated_alias(boundary="orthogonalization")
    def __init__(self, wavelet: Union[Wavelet, str], *, axes: _fwt.AxisHint = None, orthogonalization: str = "qr",
                 separable: bool = True):
        self.wavelet = as_wavelet(wavelet)
        self.orthogonalization = orthogonalization
        self.separable = separable
        self.axes = _fwt._ensure_axes(axes, 2)
        self.level: Optional[int] = None
        self.input_signal_shape: Optional[Tuple[int, int]] = None
        self.padded = False
        self._taps = _bank_taps(self.wavelet, orthogonalization)
        if not separable:
            raise NotImplementedError(_NON_SEPARABLE)
        self._bank = _bwt.bank(self._taps, orthogonalization, "synthesis")

    @property
    def sparse_ifwt_operator(self) -> torch.Tensor:
        """Separable transforms have no single operator matrix (reference matmul_transform_2.py:639-675)."""
        raise NotImplementedError

    def __call__(self, coefficients: WaveletCoeff2d) -> torch.Tensor:
        coefficients = tuple(coefficients)
        if not coefficients or not isinstance(coefficients[0], torch.Tensor):
            raise ValueError("First element of coeffs must be the approximation coefficient tensor.")
        layout = _fwt._Layout(coefficients[0], 2, self.axes)
        flat = [coefficients[0]]
        for c in coefficients[1:]:
            if not isinstance(c, tuple) or len(c) != 3:
                raise ValueError(f"Unexpected detail coefficient type: {type(c)}. Detail coefficients must be a 3-tuple of tensors as "
                                 "returned by MatrixWavedec2.")
            for t in c:
                if not isinstance(t, torch.Tensor):
                    raise ValueError(f"Unexpected input type {type(t)}")
            flat.extend(c)
        _fwt._check_same_device_dtype(flat)
        ll = layout.fold(coefficients[0])
        levels = [[layout.fold(t) for t in c] for c in coefficients[1:]]
        level = len(levels)
        if level:
            height, width = (int(s) * 2 for s in levels[-1][0].shape[-2:])
            if self.input_signal_shape != (height, width) or self.level != level:
                self.input_signal_shape, self.level = (height, width), level
                _, _, self.padded = _plan_levels(level, (height, width), self._bank.filt_len)  # (the warning and ``padded``)
        out_extents = _synthesis_extents(ll.shape, levels, "All coefficients on each level must have the same shape")
        _engine._require_gpu(ll)
        for bands, ext in zip(levels, out_extents):
            lh, hl, hh = bands
            ll = _bwt.transposed([ll, lh, hl, hh], self._bank, ext)
        return layout.unfold(ll)
