"""Boundary-filter tables of the padding-free ("boundary wavelet") transforms — host side, numpy, float64.

One level of ``MatrixWavedec`` is ``c = A x`` with an N x N matrix (N even) whose rows ``0 .. N/2-1`` are low-pass and
``N/2 .. N-1`` high-pass (reference src/ptwt/matmul_transform.py:47-81, 434-463).  Row ``m`` of a band is the strided correlation

    y[m] = sum_t f[t] x[2 m + L/2 - t]                (f = dec_lo / dec_hi, PyWavelets order; "sameshift", zero extension)

except for the rows the zero extension truncates: the first ``ceil((L-2)/4)`` and the last ``floor(L/4)`` of each band.  The
reference orthonormalises those (in the order low-top, low-bottom, high-top, high-bottom) against one another.  For
``N >= 2 (L-1)`` the rows of the two ends do not overlap, each lives in the ``L-1`` columns next to its end, and the result does
not depend on N: two small blocks per band describe every level of every signal length.

The synthesis matrix is built the same way from the reversed ``rec_*`` filters and transposed (matmul_transform.py:84-118,
467-499); for orthogonal wavelets it is the analysis matrix transposed, for biorthogonal ones it is not.

Orthonormalisation: Householder QR (LAPACK, float64) of the compact block, every row's sign fixed to the Gram-Schmidt sign — a
positive inner product with the truncated filter row it came from.  ``"qr"`` and ``"gramschmidt"`` therefore give the SAME
tables here.  The reference's ``"gramschmidt"`` gives these rows (its classical Gram-Schmidt loses orthogonality for long filters,
this does not); its ``"qr"`` rows equal them up to one sign per row that depends on LAPACK's pivots, on N and on the dtype.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Dict, Sequence, Tuple

import numpy as np

METHODS = ("qr", "gramschmidt")


def boundary_rows(filt_len: int) -> Tuple[int, int]:
    """(top, bottom) boundary rows per band: ``ceil((L-2)/4)``, ``floor(L/4)``."""
    return (filt_len - 2 + 3) // 4, filt_len // 4


def row_filters(taps: Sequence[Sequence[float]], which: str) -> Tuple[np.ndarray, np.ndarray]:
    """The (low, high) filters ``f`` of the row formula above: the ``dec_*`` filters for "analysis", the reversed ``rec_*``
    filters for "synthesis" (whose matrix is the transpose of the rows built from them)."""
    dec_lo, dec_hi, rec_lo, rec_hi = (np.asarray(t, dtype=np.float64) for t in taps)
    if which == "analysis":
        return dec_lo, dec_hi
    if which == "synthesis":
        return rec_lo[::-1].copy(), rec_hi[::-1].copy()
    raise ValueError("which must be 'analysis' or 'synthesis'")


def _raw_rows(f: np.ndarray, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """(rows [n/2, n], entries per row) of one band with zero extension."""
    L = len(f)
    m = np.arange(n // 2)[:, None]
    j = np.arange(n)[None, :]
    t = 2 * m + L // 2 - j
    ok = (t >= 0) & (t < L)
    return np.where(ok, f[np.clip(t, 0, L - 1)], 0.0), ok.sum(axis=1)


def _orthonormalise(rows: np.ndarray) -> np.ndarray:
    """Rows -> orthonormal rows spanning the same nested subspaces, signs as Gram-Schmidt (R's diagonal positive)."""
    if rows.shape[0] == 0:
        return rows
    q, r = np.linalg.qr(rows.T)
    s = np.sign(np.diag(r))
    s[s == 0] = 1.0
    return (q * s[None, :]).T


def _check_method(method: str) -> None:
    if method not in METHODS:
        raise NotImplementedError(f"orthogonalization method {method!r} is not supported (choose 'qr' or 'gramschmidt')")


@lru_cache(maxsize=256)
def _blocks_cached(taps: tuple, which: str) -> Dict[str, np.ndarray]:
    f_lo, f_hi = row_filters(taps, which)
    L = len(f_lo)
    nt, nb = boundary_rows(L)
    n = 2 * max(L - 1, 1)  # the smallest length with disjoint ends; any larger N gives the same blocks
    w = L - 1
    lo, _ = _raw_rows(f_lo, n)
    hi, _ = _raw_rows(f_hi, n)
    top = _orthonormalise(np.concatenate([lo[:nt, :w], hi[:nt, :w]]))
    bot = _orthonormalise(np.concatenate([lo[n // 2 - nb:, n - w:], hi[n // 2 - nb:, n - w:]]))
    out = {"lo_top": top[:nt], "hi_top": top[nt:], "lo_bot": bot[:nb], "hi_bot": bot[nb:]}
    for v in out.values():
        v.setflags(write=False)
    return out


def boundary_blocks(taps: Sequence[Sequence[float]], method: str = "qr", which: str = "analysis") -> Dict[str, np.ndarray]:
    """The orthonormalised boundary rows of a filter bank: ``lo_top`` / ``hi_top`` [ceil((L-2)/4), L-1] over columns
    ``0 .. L-2`` and ``lo_bot`` / ``hi_bot`` [floor(L/4), L-1] over columns ``N-L+1 .. N-1`` (float64).  Valid for every even
    ``N >= 2 (L-1)``.  ``taps`` = (dec_lo, dec_hi, rec_lo, rec_hi) as host floats."""
    _check_method(method)
    return _blocks_cached(tuple(tuple(float(v) for v in t) for t in taps), which)


def kernel_tables(taps: Sequence[Sequence[float]], method: str = "qr", which: str = "analysis") -> np.ndarray:
    """The blocks in the layout the kernels read: float64 [2, nt + nb, L] (band, boundary row, coefficient) — rows
    ``0 .. nt-1`` are the top rows over the window of columns ``0 .. L-1`` (last coefficient 0), rows ``nt ..`` the bottom rows
    over columns ``N-L .. N-1`` (first coefficient 0), so every output of a level is L multiply-adds over a contiguous window."""
    b = boundary_blocks(taps, method, which)
    L = len(taps[0])
    nt, nb = boundary_rows(L)
    tab = np.zeros((2, max(nt + nb, 1), L), dtype=np.float64)
    for band, name in enumerate(("lo", "hi")):
        tab[band, :nt, : L - 1] = b[name + "_top"]
        tab[band, nt:nt + nb, 1:] = b[name + "_bot"]
    return tab


def level_matrix(taps: Sequence[Sequence[float]], n: int, method: str = "qr", which: str = "analysis") -> np.ndarray:
    """Dense N x N matrix of one level (float64): the analysis matrix ``A``, or the synthesis matrix ``S`` (already transposed:
    ``x = S c``).  ``L <= N``, N even.  For ``N >= 2 (L-1)`` it is assembled from the blocks; for shorter signals the two ends
    overlap and all truncated rows are orthonormalised together, in row order, as the reference does."""
    _check_method(method)
    f_lo, f_hi = row_filters(taps, which)
    L = len(f_lo)
    if n % 2 or n < L:
        raise ValueError(f"a level needs an even length of at least the filter length, got {n} for {L} taps")
    lo, cnt_lo = _raw_rows(f_lo, n)
    hi, cnt_hi = _raw_rows(f_hi, n)
    a = np.concatenate([lo, hi])
    if n >= 2 * (L - 1):
        b = boundary_blocks(taps, method, which)
        nt, nb = boundary_rows(L)
        w, h = L - 1, n // 2
        for off, name in ((0, "lo"), (h, "hi")):
            a[off:off + nt] = 0.0
            a[off:off + nt, :w] = b[name + "_top"]
            a[off + h - nb:off + h] = 0.0
            a[off + h - nb:off + h, n - w:] = b[name + "_bot"]
    else:
        sel = np.flatnonzero(np.concatenate([cnt_lo, cnt_hi]) != L)
        a[sel] = _orthonormalise(a[sel])
    return a if which == "analysis" else a.T.copy()


def level_coo(taps: Sequence[Sequence[float]], n: int, method: str = "qr", which: str = "analysis"):
    """The matrix of :func:`level_matrix` as COO triplets (row indices, column indices, values) without forming an N x N array for
    ``N >= 2 (L-1)``: about ``N L`` entries."""
    L = len(taps[0])
    if n < 2 * (L - 1):
        a = level_matrix(taps, n, method, which)
        r, c = np.nonzero(a)
        return r, c, a[r, c]
    _check_method(method)
    if n % 2:
        raise ValueError(f"a level needs an even length, got {n}")
    f_lo, f_hi = row_filters(taps, which)
    b = boundary_blocks(taps, method, which)
    nt, nb = boundary_rows(L)
    h, w = n // 2, L - 1
    rows, cols, vals = [], [], []
    m = np.arange(nt, h - nb)[:, None]
    t = np.arange(L)[None, :]
    for off, f, name in ((0, f_lo, "lo"), (h, f_hi, "hi")):
        rows.append(np.broadcast_to(m + off, (m.shape[0], L)).ravel())
        cols.append((2 * m + L // 2 - t).ravel())
        vals.append(np.broadcast_to(f[None, :], (m.shape[0], L)).ravel())
        for blk, r0, c0 in ((b[name + "_top"], off, 0), (b[name + "_bot"], off + h - nb, n - w)):
            rr, cc = np.meshgrid(np.arange(blk.shape[0]) + r0, np.arange(w) + c0, indexing="ij")
            rows.append(rr.ravel())
            cols.append(cc.ravel())
            vals.append(blk.ravel())
    r, c, v = np.concatenate(rows), np.concatenate(cols), np.concatenate(vals)
    return (r, c, v) if which == "analysis" else (c, r, v)
