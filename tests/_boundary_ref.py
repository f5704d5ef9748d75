"""The float64 CPU reference of the boundary-wavelet transforms for the tests: the level operators that
``ptwt_amd._boundary.level_coo`` / ``level_matrix`` build on the host (numpy, float64, never a kernel), applied with plain torch on
the CPU along one, two or three axes — sparse for rows and volumes, dense for planes — and chained into multi-level transforms the way the reference's classes chain theirs
(one virtual sample appended to an odd extent, dropped again between the levels of a synthesis).  Everything is differentiable torch.

tests/test_boundary_host.py pins this chain to the reference library's goldens (ptwt_ref_boundary.npz, ptwt_ref_boundary_mid.npz);
tests/test_gpu_boundary_kernels.py compares the kernels with it.
"""
import numpy as np
import torch

from ptwt_amd import _boundary

MODES = ("zero", "constant", "reflect", "periodic", "symmetric")
_OPS = {}


def virtual_index(n, mode):
    """Index of the sample that the one appended to an odd extent ``n`` copies (None: it is zero): the first sample of the right
    padding of each mode.  "reflect" needs two samples, as torch's reflection padding does."""
    if mode == "reflect" and n < 2:
        raise ValueError("reflect needs at least two samples")
    return {"zero": None, "constant": n - 1, "reflect": n - 2, "periodic": 0, "symmetric": n - 1}[mode]


def with_virtual(x, dim, mode):
    n = x.shape[dim]
    if n % 2 == 0:
        return x
    src = virtual_index(n, mode)
    extra = torch.zeros_like(x.narrow(dim, 0, 1)) if src is None else x.narrow(dim, src, 1)
    return torch.cat([x, extra], dim)


def rows_operator(taps, n, which, dense=False, round32=False, dtype=torch.float64):
    """The rows ``B`` of a bank for an even length ``n`` ([n, n], low-pass rows first): the analysis matrix for which="analysis", the
    TRANSPOSE of the synthesis matrix for which="synthesis".  ``round32``: every entry (taps and table rows) rounded to float32 first,
    as the fused float32 kernels hold them.  Sparse COO unless ``dense``; cached."""
    taps = tuple(tuple(float(v) for v in t) for t in taps)
    key = (taps, n, which, dense, round32, dtype)
    op = _OPS.get(key)
    if op is None:
        if len(_OPS) > 64:
            _OPS.clear()
        r, c, v = _boundary.level_coo(taps, n, "gramschmidt", which)
        if which == "synthesis":
            r, c = c, r
        if round32:
            v = v.astype(np.float32).astype(np.float64)
        op = torch.sparse_coo_tensor(np.stack([r, c]), v, size=(n, n), dtype=torch.float64).coalesce()
        if dense:
            op = op.to_dense()
        op = _OPS[key] = op.to(dtype)
    return op


def _apply(op, x, transpose=False):
    """op (or its transpose) applied along the last axis of x [..., n]."""
    flat = x.reshape(-1, x.shape[-1])
    if op.is_sparse:
        out = torch.sparse.mm(op.t() if transpose else op, flat.t()).t()
    else:
        out = flat @ (op if transpose else op.t())
    return out.reshape(*x.shape[:-1], out.shape[-1])


def _along(op, x, dim, transpose=False):
    return _apply(op, x.transpose(dim, -1), transpose=transpose).transpose(dim, -1)


def rows_level(x, taps, which, mode, **kw):
    """One analysis level: x [B, n0(, n1(, n2))] -> [B, 2^d, M0(, M1(, M2))]; band plane s: bit (d-1-a) set = high-pass along axis a
    (2-D: 2 (row band) + (column band); 3-D: the order of ``wavedec3``, "aad" = 1 ... "ddd" = 7).  Last axis first."""
    ndim = x.dim() - 1
    for a in range(ndim):
        x = with_virtual(x, 1 + a, mode)
    c = x
    for dim in range(ndim, 0, -1):
        c = _along(rows_operator(taps, c.shape[dim], which, dense=ndim == 2, dtype=x.dtype, **kw), c, dim)
    half = [n // 2 for n in c.shape[1:]]
    split = c.reshape(x.shape[0], *(v for m in half for v in (2, m)))
    return split.permute(0, *range(1, 2 * ndim, 2), *range(2, 2 * ndim + 1, 2)).reshape(x.shape[0], 1 << ndim, *half)


def transposed_level(bands, taps, which, out_extent, **kw):
    """One synthesis level y = B^T c from the 2^d bands [B, M0(, M1(, M2))], cropped to ``out_extent`` (2 M or 2 M - 1 per axis)."""
    ndim = bands[0].dim() - 1
    y = list(bands)
    for dim in range(-1, -ndim - 1, -1):
        y = [torch.cat(y[i: i + 2], dim) for i in range(0, len(y), 2)]
    y = y[0]
    for dim in ((2, 1) if ndim == 2 else range(1, ndim + 1)):  # (planes: columns first, volumes: depth first — as they always were)
        y = _along(rows_operator(taps, y.shape[dim], which, dense=ndim == 2, dtype=y.dtype, **kw), y, dim, transpose=True)
    return y[(slice(None), *(slice(0, n) for n in out_extent))]


def wavedec(x, taps, level, mode="zero", **kw):
    """MatrixWavedec / MatrixWavedec2 / MatrixWavedec3 on x [B, n] / [B, h, w] / [B, d, h, w]: the flat coefficient list
    [a, d_level, ..., d_1] (2-D: a, then lh, hl, hh of each level, coarsest first; 3-D: aaa, then the seven details of each level).
    A level whose input is shorter than the filter along an axis is not computed."""
    ndim, L = x.dim() - 1, len(taps[0])
    lo, details = x, []
    for _ in range(level):
        if min(lo.shape[1:]) < L:
            break
        buf = rows_level(lo, taps, "analysis", mode, **kw)
        lo = buf[:, 0]
        details.append([buf[:, s] for s in range(1, 1 << ndim)])
    out = [lo]
    for d in details[::-1]:
        out.extend(d)
    return out


def waverec(coeffs, taps, ndim, **kw):
    """MatrixWaverec / MatrixWaverec2 / MatrixWaverec3 on the flat list of :func:`wavedec`: the sample appended to an odd
    approximation is dropped between levels but not after the last one."""
    per = (1 << ndim) - 1
    lo = coeffs[0]
    levels = [coeffs[1 + i: 1 + i + per] for i in range(0, len(coeffs) - 1, per)]
    for i, bands in enumerate(levels):
        ext = [2 * m for m in lo.shape[1:]]
        if i + 1 < len(levels):
            nxt = levels[i + 1][0].shape[1:]
            assert all(e - n in (0, 1) for e, n in zip(ext, nxt))
            ext = list(nxt)
        lo = transposed_level([lo] + list(bands), taps, "synthesis", ext, **kw)
    return lo
