"""The float64 CPU reference of the boundary-wavelet transforms for the tests: the level operators that
``ptwt_amd._boundary.level_coo`` / ``level_matrix`` build on the host (numpy, float64, never a kernel), applied with plain torch on
the CPU — sparse for rows, dense for planes — and chained into multi-level transforms the way the reference's classes chain theirs
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


def rows_level(x, taps, which, mode, **kw):
    """One analysis level: x [B, n0(, n1)] -> [B, 2^d, M0(, M1)], band s = 2 (row band) + (column band)."""
    ndim = x.dim() - 1
    for a in range(ndim):
        x = with_virtual(x, 1 + a, mode)
    dense = ndim == 2
    c = _apply(rows_operator(taps, x.shape[-1], which, dense=dense, dtype=x.dtype, **kw), x)
    if ndim == 1:
        return c.reshape(x.shape[0], 2, -1)
    c = _apply(rows_operator(taps, x.shape[-2], which, dense=dense, dtype=x.dtype, **kw), c.transpose(-1, -2)).transpose(-1, -2)
    h, w = c.shape[1] // 2, c.shape[2] // 2
    return c.reshape(x.shape[0], 2, h, 2, w).permute(0, 1, 3, 2, 4).reshape(x.shape[0], 4, h, w)


def transposed_level(bands, taps, which, out_extent, **kw):
    """One synthesis level y = B^T c from the 2^d bands [B, M0(, M1)], cropped to ``out_extent`` (2 M or 2 M - 1 per axis)."""
    ndim = bands[0].dim() - 1
    dense = ndim == 2
    if ndim == 1:
        c = torch.cat(list(bands), -1)
        y = _apply(rows_operator(taps, c.shape[-1], which, dense=dense, dtype=c.dtype, **kw), c, transpose=True)
        return y[:, : out_extent[0]]
    c = torch.cat([torch.cat([bands[0], bands[1]], -1), torch.cat([bands[2], bands[3]], -1)], -2)
    y = _apply(rows_operator(taps, c.shape[-1], which, dense=dense, dtype=c.dtype, **kw), c, transpose=True)
    y = _apply(rows_operator(taps, c.shape[-2], which, dense=dense, dtype=c.dtype, **kw), y.transpose(-1, -2), transpose=True).transpose(-1, -2)
    return y[:, : out_extent[0], : out_extent[1]]


def wavedec(x, taps, level, mode="zero", **kw):
    """MatrixWavedec / MatrixWavedec2 on x [B, n] / [B, h, w]: the flat coefficient list [a, d_level, ..., d_1] (2-D: a, then lh, hl,
    hh of each level, coarsest first).  A level whose input is shorter than the filter is not computed."""
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
    """MatrixWaverec / MatrixWaverec2 on the flat list of :func:`wavedec`: the sample appended to an odd approximation is dropped
    between levels but not after the last one."""
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
