"""TEST-ONLY float64 references of the 2-D stationary transform (``ptwt_amd.swt2`` / ``iswt2``, csrc/mifwt_swt2.hip).

A 2-D level is the 1-D level along both axes.  The numpy operators below compose it from ``tests/_oracle_engine.swt_level_fwd`` /
``swt_level_inv`` — the stand-ins that tests/test_torch_autograd_ref.py pins to the reference library's goldens — one axis at a time,
with explicit axis moves (no shared code with the library's composed route).  A level takes FOUR filters: ``row_lo, row_hi`` along
the last axis, ``col_lo, col_hi`` along the one before it.  Planes of a level: cA, cH, cV, cD with cH high-pass along axis -2 and
low-pass along axis -1 (the band names of ``wavedec2``).

The torch versions (``t_*``) are the same sums written with ``torch.roll`` in whatever dtype they are given: float64 they are the
autograd reference (data, coefficient and tap gradients of any order), float32 they are "the reference in float32" that the float32
gradient bound of tests/test_gpu_swt2.py is taken from.
"""
import numpy as np
import torch

from tests import _oracle_engine as oe


# ---- numpy, float64 -------------------------------------------------------------------------------------------------------------------
def _axis_fwd(x, lo, hi, dilation, scale, axis):
    xm = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    out = oe.swt_level_fwd(torch.from_numpy(np.ascontiguousarray(xm).reshape(-1, xm.shape[-1])), lo, hi, dilation, scale).numpy()
    return tuple(np.moveaxis(out[:, k].reshape(xm.shape), -1, axis) for k in (0, 1))


def _axis_inv(a, d, lo, hi, dilation, scale, axis):
    am = np.moveaxis(np.asarray(a, dtype=np.float64), axis, -1)
    dm = np.moveaxis(np.asarray(d, dtype=np.float64), axis, -1)
    n = am.shape[-1]
    y = oe.swt_level_inv(torch.from_numpy(np.ascontiguousarray(am).reshape(-1, n)), torch.from_numpy(np.ascontiguousarray(dm).reshape(-1, n)),
                         lo, hi, dilation, scale).numpy()
    return np.moveaxis(y.reshape(am.shape), -1, axis)


def level_fwd(x, taps, dilation, scale):
    """x [..., H, W] -> (cA, cH, cV, cD); taps = (row_lo, row_hi, col_lo, col_hi)."""
    p_lo, p_hi = _axis_fwd(x, taps[0], taps[1], dilation, 1.0, -1)
    ca, ch = _axis_fwd(p_lo, taps[2], taps[3], dilation, scale, -2)
    cv, cd = _axis_fwd(p_hi, taps[2], taps[3], dilation, scale, -2)
    return ca, ch, cv, cd


def level_inv(bands, taps, dilation, scale):
    """(cA, cH, cV, cD) -> y: U = S_row(cA, cV), V = S_row(cH, cD), y = S_col(U, V)."""
    ca, ch, cv, cd = bands
    u = _axis_inv(ca, cv, taps[0], taps[1], dilation, 1.0, -1)
    v = _axis_inv(ch, cd, taps[0], taps[1], dilation, 1.0, -1)
    return _axis_inv(u, v, taps[2], taps[3], dilation, scale, -2)


def swt_max_level(n):
    level = 0
    while n > 0 and n % 2 == 0:
        n //= 2
        level += 1
    return level


def _to_last(x, axes):
    return np.moveaxis(np.asarray(x, dtype=np.float64), axes, (-2, -1))


def swt2(x, dec_lo, dec_hi, level=None, axes=(-2, -1)):
    """[cA_n, (cH_n, cV_n, cD_n), ..., (cH_1, cV_1, cD_1)] over ``axes``, every array of x's shape."""
    cur = _to_last(x, axes)
    if level is None:
        level = min(swt_max_level(cur.shape[-2]), swt_max_level(cur.shape[-1]))
    taps = (dec_lo, dec_hi, dec_lo, dec_hi)
    out = []
    for lvl in range(level):
        cur, ch, cv, cd = level_fwd(cur, taps, 2 ** lvl, 1.0)
        out.append(tuple(np.moveaxis(t, (-2, -1), axes) for t in (ch, cv, cd)))
    out.append(np.moveaxis(cur, (-2, -1), axes))
    return out[::-1]


def iswt2(coeffs, rec_lo, rec_hi, axes=(-2, -1)):
    cur = _to_last(coeffs[0], axes)
    taps = (rec_lo, rec_hi, rec_lo, rec_hi)
    n = len(coeffs) - 1
    for pos, det in enumerate(coeffs[1:]):
        ch, cv, cd = (_to_last(t, axes) for t in det)
        cur = level_inv((cur, ch, cv, cd), taps, 2 ** (n - pos - 1), 0.25)
    return np.moveaxis(cur, (-2, -1), axes)


def level_matrix(h, w, taps, dilation, scale, inverse):
    """Dense matrix of a level on an h x w plane: analysis [4 h w, h w] (planes cA, cH, cV, cD stacked), synthesis [h w, 4 h w]."""
    n = h * w
    if not inverse:
        cols = []
        for k in range(n):
            e = np.zeros(n)
            e[k] = 1.0
            cols.append(np.concatenate([b.reshape(-1) for b in level_fwd(e.reshape(h, w), taps, dilation, scale)]))
        return np.stack(cols, axis=1)
    cols = []
    for k in range(4 * n):
        e = np.zeros(4 * n)
        e[k] = 1.0
        cols.append(level_inv(tuple(e.reshape(4, h, w)), taps, dilation, scale).reshape(-1))
    return np.stack(cols, axis=1)


# ---- torch (autograd reference in float64; "the reference in float32" when fed float32) ------------------------------------------------
def t_axis_fwd(x, lo, hi, dilation, scale, dim):
    flen = len(lo)
    a = sum(lo[m] * torch.roll(x, -dilation * (flen // 2 - m), dim) for m in range(flen))
    d = sum(hi[m] * torch.roll(x, -dilation * (flen // 2 - m), dim) for m in range(flen))
    return a * scale, d * scale


def t_axis_inv(a, d, lo, hi, dilation, scale, dim):
    flen = len(lo)
    return scale * sum(lo[j] * torch.roll(a, -dilation * (flen // 2 - 1 - j), dim) + hi[j] * torch.roll(d, -dilation * (flen // 2 - 1 - j), dim)
                       for j in range(flen))


def t_level_fwd(x, taps, dilation, scale, dims=(-2, -1)):
    p_lo, p_hi = t_axis_fwd(x, taps[0], taps[1], dilation, 1.0, dims[1])
    ca, ch = t_axis_fwd(p_lo, taps[2], taps[3], dilation, scale, dims[0])
    cv, cd = t_axis_fwd(p_hi, taps[2], taps[3], dilation, scale, dims[0])
    return ca, ch, cv, cd


def t_level_inv(bands, taps, dilation, scale, dims=(-2, -1)):
    ca, ch, cv, cd = bands
    u = t_axis_inv(ca, cv, taps[0], taps[1], dilation, 1.0, dims[1])
    v = t_axis_inv(ch, cd, taps[0], taps[1], dilation, 1.0, dims[1])
    return t_axis_inv(u, v, taps[2], taps[3], dilation, scale, dims[0])


def t_swt2(x, dec_lo, dec_hi, level=None, axes=(-2, -1)):
    if level is None:
        level = min(swt_max_level(x.shape[axes[0]]), swt_max_level(x.shape[axes[1]]))
    taps = (dec_lo, dec_hi, dec_lo, dec_hi)
    out, cur = [], x
    for lvl in range(level):
        cur, ch, cv, cd = t_level_fwd(cur, taps, 2 ** lvl, 1.0, axes)
        out.append((ch, cv, cd))
    out.append(cur)
    return out[::-1]


def t_iswt2(coeffs, rec_lo, rec_hi, axes=(-2, -1)):
    taps = (rec_lo, rec_hi, rec_lo, rec_hi)
    cur, n = coeffs[0], len(coeffs) - 1
    for pos, det in enumerate(coeffs[1:]):
        cur = t_level_inv((cur, *det), taps, 2 ** (n - pos - 1), 0.25, axes)
    return cur
