"""The float64 CPU reference of the 3-D boundary-wavelet transforms for the tests: the level operators of tests/_boundary_ref.py
(``ptwt_amd._boundary.level_coo`` on the host, never a kernel) applied along width, height and depth with plain torch, and chained into
multi-level transforms the way the reference's MatrixWavedec3 / MatrixWaverec3 chain theirs.  Everything is differentiable torch.

Band plane ``s`` of a level: bit 2 = depth high-pass, bit 1 = height, bit 0 = width (the order of ``wavedec3``: "aad" = 1 ... "ddd" = 7).
tests/test_boundary3_host.py pins this chain to the reference library's goldens (ptwt_ref_boundary3.npz); tests/test_gpu_boundary3.py
compares the kernels and the public classes with it.
"""
import numpy as np
import torch

from tests import _boundary_ref as BR

MODES = BR.MODES
KEYS = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")


def formula_input(shape, seed):
    """The stored-nowhere input of the golden entries with "stride" (tests/golden/make_ptwt_ref_boundary3_goldens.py)."""
    i = np.arange(int(np.prod(shape)), dtype=np.float64)
    return (np.cos(1.7 * i + 0.37 * seed) + np.sin(0.013 * i * i + seed)).reshape(shape)


def _along(op, x, dim, transpose=False):
    return BR._apply(op, x.transpose(dim, -1), transpose=transpose).transpose(dim, -1)


def rows_level(x, taps, which, mode, **kw):
    """One analysis level: x [B, n0, n1, n2] -> [B, 8, M0, M1, M2]."""
    for a in range(3):
        x = BR.with_virtual(x, 1 + a, mode)
    c = x
    for dim in (3, 2, 1):
        c = _along(BR.rows_operator(taps, c.shape[dim], which, dtype=x.dtype, **kw), c, dim)
    d, h, w = (n // 2 for n in c.shape[1:])
    return c.reshape(x.shape[0], 2, d, 2, h, 2, w).permute(0, 1, 3, 5, 2, 4, 6).reshape(x.shape[0], 8, d, h, w)


def transposed_level(bands, taps, which, out_extent, **kw):
    """One synthesis level y = B^T c from the eight bands [B, M0, M1, M2], cropped to ``out_extent`` (2 M or 2 M - 1 per axis)."""
    halves = [torch.cat([torch.cat([bands[q], bands[q + 1]], -1), torch.cat([bands[q + 2], bands[q + 3]], -1)], -2) for q in (0, 4)]
    y = torch.cat(halves, -3)
    for dim in (1, 2, 3):
        y = _along(BR.rows_operator(taps, y.shape[dim], which, dtype=y.dtype, **kw), y, dim, transpose=True)
    return y[:, : out_extent[0], : out_extent[1], : out_extent[2]]


def wavedec3(x, taps, level, mode="zero", **kw):
    """MatrixWavedec3 on x [B, d, h, w]: the flat list [aaa, the seven details of each level, coarsest first].  A level whose input is
    shorter than the filter along an axis is not computed."""
    L = len(taps[0])
    lo, details = x, []
    for _ in range(level):
        if min(lo.shape[1:]) < L:
            break
        buf = rows_level(lo, taps, "analysis", mode, **kw)
        lo = buf[:, 0]
        details.append([buf[:, s] for s in range(1, 8)])
    out = [lo]
    for d in details[::-1]:
        out.extend(d)
    return out


def waverec3(coeffs, taps, **kw):
    """MatrixWaverec3 on the flat list of :func:`wavedec3`: the sample appended to an odd approximation is dropped between levels but
    not after the last one."""
    lo = coeffs[0]
    levels = [coeffs[1 + i: 8 + i] for i in range(0, len(coeffs) - 1, 7)]
    for i, bands in enumerate(levels):
        ext = [2 * m for m in lo.shape[1:]]
        if i + 1 < len(levels):
            nxt = levels[i + 1][0].shape[1:]
            assert all(e - n in (0, 1) for e, n in zip(ext, nxt))
            ext = list(nxt)
        lo = transposed_level([lo] + list(bands), taps, "synthesis", ext, **kw)
    return lo
