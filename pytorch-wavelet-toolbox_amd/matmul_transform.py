"""Padding-free 1-D fast wavelet transform with boundary filters: ``MatrixWavedec`` / ``MatrixWaverec`` (API of reference
src/ptwt/matmul_transform.py).

The reference multiplies with an N x N sparse matrix per level.  Here a level is one fused HIP launch (C ABI ``mifwt_bwt_fwd`` /
``mifwt_bwt_inv``): the strided correlation with the plain taps everywhere except the few rows at each end of a band, whose
orthogonalised coefficients the edge workgroups read from a small table (``_boundary.py``); N samples in, N coefficients out, no
padded tensor, no split / cat copies.  Differentiable w.r.t. the data (each level map's backward is the other map with the same
filter bank).  A tensor-valued filter bank is read once, on the host, when the object is built: there are no tap gradients
through the orthogonalisation.

Sign convention — a deliberate departure from the reference.  Orthogonalisation fixes a boundary row only up to its sign.  Here
every boundary row has the Gram-Schmidt sign (a positive inner product with the truncated filter row it replaces), for BOTH
``orthogonalization="qr"`` and ``"gramschmidt"``, which therefore give the same numbers, equal to the reference's ``"gramschmidt"``.
The reference's ``"qr"`` rows are the same up to one sign per row, but that sign is an accident of LAPACK's Householder pivots:
it changes with the signal length and between float32 and float64.  Coefficients the reference produced with ``"qr"`` therefore
differ from this package's in the sign of some boundary coefficients (and, through the low-pass boundary rows, in deeper levels)
and must be reconstructed by a synthesis with the matching signs, i.e. by the reference itself.
"""
from __future__ import annotations

import functools
import sys
import warnings
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _bwt, _engine, _fwt
from ._wavelets import as_wavelet, host_taps
from .constants import Wavelet

__all__ = ["MatrixWavedec", "MatrixWaverec"]


def _deprecated_alias(**aliases: str):
    """``boundary=`` is the deprecated name of ``orthogonalization=`` (src/ptwt/_util.py:750-800)."""

    def deco(func):
        @functools.wraps(func)
        def wrapper(*args, **kwargs):
            for alias, new in aliases.items():
                if alias in kwargs:
                    if new in kwargs:
                        raise TypeError(f"{func.__name__} received both {alias} and {new} as arguments! {alias} is deprecated, "
                                        f"use {new} instead.")
                    warnings.warn(f"`{alias}` is deprecated as an argument to `{func.__name__}`; use `{new}` instead.",
                                  DeprecationWarning, stacklevel=2)
                    kwargs[new] = kwargs.pop(alias)
            return func(*args, **kwargs)

        return wrapper

    return deco


def _bank_taps(wavelet, orthogonalization):
    """Constructor checks shared by the four classes -> the filter bank as host floats."""
    if orthogonalization not in ("qr", "gramschmidt"):
        raise NotImplementedError
    taps = host_taps(wavelet)
    if len(taps[0]) != len(taps[2]):
        raise ValueError("All filters must have the same length")
    return taps


def _plan_levels(level: int, shape: Sequence[int], filt_len: int):
    """The level loop of the six classes (the reference's _construct_analysis_matrices / _construct_synthesis_matrices without the
    matrices) for a shape of one, two or three extents -> (the even sizes per level and the coarsest approximation's, the pad flags
    per level in axis order, whether anything was padded).  Writes the reference's warning where ``level`` is too deep."""
    shape = tuple(shape)
    size_list, pad_list, cur = [], [], shape
    for curr_level in range(1, level + 1):
        if min(cur) < filt_len:
            given, current = {1: (f"size {shape[0]}", f"length {cur[0]}"), 2: (f"shape {shape}", f"height and width {cur}"),
                              3: (f"shape {shape}", f"depth, height and width {cur}")}[len(shape)]
            sys.stderr.write(
                f"Warning: The selected number of decomposition levels {level} is too large for the given input {given}. At level "
                f"{curr_level}, the current signal {current} is smaller than the filter length {filt_len}. Therefore, the "
                f"transformation is only computed up to the decomposition level {curr_level - 1}.\n")
            break
        pad_list.append(tuple(n % 2 != 0 for n in cur))
        cur = tuple(n + n % 2 for n in cur)
        size_list.append(cur)
        cur = tuple(n // 2 for n in cur)
    size_list.append(cur)
    return size_list, pad_list, any(any(pad) for pad in pad_list)


def _synthesis_extents(approx_shape, levels, message: str):
    """Shapes first (the reference's checks inside its level loop), then the device: ``levels`` holds the folded detail bands
    [B, M..] per level, coarsest first.  The bands of a level must have the shape of the current approximation (``message``); a level
    gives 2 M samples per axis, or the next level's extent where that is 2 M - 1.  -> the output extents per level."""
    out_extents, cur = [], tuple(approx_shape)
    for c_pos, bands in enumerate(levels):
        if any(tuple(t.shape) != cur for t in bands):
            raise ValueError(message)
        pred = [2 * m for m in cur[1:]]
        if c_pos < len(levels) - 1:
            for a, nxt in enumerate(levels[c_pos + 1][0].shape[1:]):
                if nxt != pred[a]:
                    assert nxt == pred[a] - 1, "padding error, please open an issue on github"
                    pred[a] = int(nxt)
        out_extents.append(tuple(pred))
        cur = (cur[0], *pred)
    return out_extents


def _mode_for(extents_per_level, mode) -> int:
    """The boundary mode id if any level has an odd extent (only then the reference looks at the mode string), else zero."""
    if any(n % 2 for ext in extents_per_level for n in ext):
        return _fwt._mode_id(mode)
    return _engine.MODE_IDS["zero"]


class MatrixWavedec:
    """1-D fast wavelet transform with boundary filters instead of padding (drop-in for ``ptwt.MatrixWavedec``).

    N samples give N coefficients and the transform is orthogonal for orthogonal wavelets.  Odd lengths (of the input or of an
    approximation) get one sample appended by ``odd_coeff_padding_mode``.  ``orthogonalization`` accepts ``"qr"`` and
    ``"gramschmidt"``; both give the same coefficients here, with every boundary filter in its Gram-Schmidt sign — see the module
    docstring for how that differs from the reference's ``"qr"``.
    """

    @_deprecated_alias(boundary="orthogonalization")
    def __init__(self, wavelet: Union[Wavelet, str], level: Optional[int] = None, *, axis: _fwt.AxisHint = None,
                 orthogonalization: str = "qr", odd_coeff_padding_mode: str = "zero") -> None:
        self.wavelet = as_wavelet(wavelet)
        self.level = level
        self.odd_coeff_padding_mode = odd_coeff_padding_mode
        self.orthogonalization = orthogonalization
        self.axis = _fwt._ensure_axes(axis, 1)[0]
        self.input_length: Optional[int] = None
        self.pad_list: List[bool] = []
        self.padded = False
        self.size_list: List[int] = []
        self._built = False
        self._taps = _bank_taps(self.wavelet, orthogonalization)
        self._bank = _bwt.bank(self._taps, orthogonalization, "analysis")
        self._op_meta = None

    @property
    def sparse_fwt_operator(self) -> torch.Tensor:
        """The whole padding-free transform as one sparse matrix: ``torch.sparse.mm(op, data.T)`` is a batched FWT
        (reference matmul_transform.py:268-308).  ValueError before the first call, NotImplementedError if a level was padded."""
        if not self._built or len(self.size_list) < 2:
            raise ValueError("Call this object first to create the transformation matrices for each level.")
        device, dtype = self._op_meta
        mats = [_bwt.sparse_level(self._bank, n, device, dtype) for n in self.size_list[:-1]]
        if len(mats) == 1:
            return mats[0]
        if self.padded:
            raise NotImplementedError
        op = mats[0]
        for m in mats[1:]:
            op = torch.sparse.mm(_cat_sparse_identity(m, op.shape[0]), op)
        return op

    def __call__(self, input_signal: torch.Tensor) -> List[torch.Tensor]:
        layout = _fwt._Layout(input_signal, 1, (self.axis,))
        x = layout.fold(input_signal)
        n = int(x.shape[-1])
        length = n + n % 2
        re_build = False
        if self.input_length != length:
            self.input_length = length
            re_build = True
        if self.level is None:
            self.level = int(np.log2(length / (self._bank.filt_len - 1)))
            re_build = True
        elif self.level <= 0:
            raise ValueError("level must be a positive integer.")
        if not self._built or len(self.size_list) < 2 or re_build:
            sizes, pads, self.padded = _plan_levels(self.level, (self.input_length,), self._bank.filt_len)
            self.size_list, self.pad_list, self._built = [s[0] for s in sizes], [p[0] for p in pads], True
        nlevels = len(self.size_list) - 1
        extents = [(n,)] + [(s // 2,) for s in self.size_list[: max(nlevels - 1, 0)]]
        mode_id = _mode_for(extents[:nlevels] if nlevels else [(n,)], self.odd_coeff_padding_mode)
        _engine._require_gpu(x)
        self._op_meta = (x.device, x.dtype)
        lo = x
        details = []
        for _ in range(nlevels):
            buf = _bwt.rows(lo, self._bank, mode_id)
            lo = buf[:, 0]
            details.append(buf[:, 1])
        if nlevels == 0:
            lo = _bwt._with_virtual(lo, 1, mode_id)
        return [layout.unfold(t) for t in [lo] + details[::-1]]


class MatrixWaverec:
    """Inverse of :class:`MatrixWavedec` (drop-in for ``ptwt.MatrixWaverec``).  As in the reference, the sample appended to an odd
    approximation is dropped between levels but not after the last one: an odd-length input comes back one sample longer.  The sign
    convention of the boundary filters is the one of :class:`MatrixWavedec` (module docstring)."""

    @_deprecated_alias(boundary="orthogonalization")
    def __init__(self, wavelet: Union[Wavelet, str], *, axis: _fwt.AxisHint = None, orthogonalization: str = "qr") -> None:
        self.wavelet = as_wavelet(wavelet)
        self.orthogonalization = orthogonalization
        self.axis = _fwt._ensure_axes(axis, 1)
        self.level: Optional[int] = None
        self.input_length: Optional[int] = None
        self.padded = False
        self.size_list: List[int] = []
        self._built = False
        self._taps = _bank_taps(self.wavelet, orthogonalization)
        self._bank = _bwt.bank(self._taps, orthogonalization, "synthesis")
        self._op_meta = None

    @property
    def sparse_ifwt_operator(self) -> torch.Tensor:
        """The whole padding-free inverse as one sparse matrix (reference matmul_transform.py:559-601)."""
        if not self._built or not self.size_list:
            raise ValueError("Call this object first to create the transformation matrices for each level.")
        device, dtype = self._op_meta
        mats = [_bwt.sparse_level(self._bank, n, device, dtype) for n in self.size_list]
        if len(mats) == 1:
            return mats[0]
        if self.padded:
            raise NotImplementedError
        op = mats[-1]
        for m in mats[:-1][::-1]:
            op = torch.sparse.mm(m, _cat_sparse_identity(op, m.shape[0]))
        return op

    def __call__(self, coefficients: Sequence[torch.Tensor]) -> torch.Tensor:
        coefficients = list(coefficients)
        if not coefficients or not isinstance(coefficients[0], torch.Tensor):
            raise ValueError("First element of coeffs must be the approximation coefficient tensor.")
        layout = _fwt._Layout(coefficients[0], 1, self.axis)
        for t in coefficients:
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"Unexpected input type {type(t)}")
        _fwt._check_same_device_dtype(coefficients)
        folded = [layout.fold(t) for t in coefficients]
        level = len(folded) - 1
        input_length = int(folded[-1].shape[-1]) * 2
        if self.level != level or self.input_length != input_length or not self._built:
            self.level, self.input_length = level, input_length
            sizes, _, self.padded = _plan_levels(level, (input_length,), self._bank.filt_len)
            self.size_list, self._built = [s[0] for s in sizes[:-1]], True  # (no entry for the coarsest approximation here)
        out_extents = _synthesis_extents(folded[0].shape, [[hi] for hi in folded[1:]], "coefficients must have the same shape")
        _engine._require_gpu(folded[0])
        self._op_meta = (folded[0].device, folded[0].dtype)
        lo = folded[0]
        for hi, ext in zip(folded[1:], out_extents):
            lo = _bwt.transposed([lo, hi], self._bank, ext)
        return layout.unfold(lo)


def _cat_sparse_identity(matrix: torch.Tensor, new_length: int) -> torch.Tensor:
    """``matrix`` extended by an identity block to ``new_length`` rows and columns (the finer levels' detail coefficients pass
    through a coarser level unchanged; reference src/ptwt/sparse_math.py cat_sparse_identity_matrix)."""
    matrix = matrix.coalesce()
    n = matrix.shape[0]
    extra = torch.arange(n, new_length, device=matrix.device)
    idx = torch.cat([matrix.indices(), torch.stack([extra, extra])], 1)
    val = torch.cat([matrix.values(), torch.ones(new_length - n, dtype=matrix.dtype, device=matrix.device)])
    return torch.sparse_coo_tensor(idx, val, size=(new_length, new_length)).coalesce()
