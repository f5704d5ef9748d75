"""TEST-ONLY float64 references of the 3-D stationary transform (``ptwt_amd.swt3`` / ``iswt3``, csrc/mifwt_swt3.hip).

A 3-D level is the 1-D level along the three axes of a volume.  The numpy operators below compose it from
``tests/_oracle_engine.swt_level_fwd`` / ``swt_level_inv`` — the stand-ins that tests/test_torch_autograd_ref.py pins to the reference
library's goldens — one axis at a time, with explicit axis moves (no shared code with the library's composed route).  A level takes SIX
filters: ``w_lo, w_hi`` along the last axis, ``h_lo, h_hi`` along the one before it, ``z_lo, z_hi`` along axis -3.  Bands of a level in
the order aaa, aad, ada, add, daa, dad, dda, ddd: index 4 [axis -3 high] + 2 [axis -2 high] + [axis -1 high], the keys of ``wavedec3``.

The torch versions (``t_*``) are the same sums written with ``torch.roll`` in whatever dtype they are given: float64 they are the
autograd reference (data, coefficient and tap gradients of any order), float32 they are "the reference in float32" that the float32
gradient bound of tests/test_gpu_swt3.py is taken from.
"""
import math

import numpy as np
import torch

from tests import _oracle_engine as oe

KEYS = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")
BANDS = ("aaa",) + KEYS


# ---- numpy, float64 -------------------------------------------------------------------------------------------------------------------
def _fold(filt, dilation, n):
    """The same filter along a periodic axis of n samples with the taps that read the same sample (D (m - m') a multiple of n) summed
    exactly (``math.fsum``) onto the first of them.  Same operator, but the reference no longer rounds a cancelling sum tap by tap: at
    7 x 9 x 1 under 34 random taps whose w_lo happens to sum to -8.1e-5 the plain tap-by-tap float64 sum was itself 1.1e-12 off the
    long-double result (norm-wise, the four bands through w_lo), above the 1e-12 it is the yardstick for; folded it is 6e-16."""
    filt = [float(v) for v in filt]
    if n > dilation * (len(filt) - 1):
        return filt
    groups = {}
    for m in range(len(filt)):
        groups.setdefault((dilation * m) % n, []).append(m)
    out = [0.0] * len(filt)
    for members in groups.values():
        out[members[0]] = math.fsum(filt[m] for m in members)
    return out


def _axis_fwd(x, lo, hi, dilation, scale, axis):
    xm = np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1)
    lo, hi = _fold(lo, dilation, xm.shape[-1]), _fold(hi, dilation, xm.shape[-1])
    out = oe.swt_level_fwd(torch.from_numpy(np.ascontiguousarray(xm).reshape(-1, xm.shape[-1])), lo, hi, dilation, scale).numpy()
    return tuple(np.moveaxis(out[:, k].reshape(xm.shape), -1, axis) for k in (0, 1))


def _axis_inv(a, d, lo, hi, dilation, scale, axis):
    am = np.moveaxis(np.asarray(a, dtype=np.float64), axis, -1)
    dm = np.moveaxis(np.asarray(d, dtype=np.float64), axis, -1)
    n = am.shape[-1]
    lo, hi = _fold(lo, dilation, n), _fold(hi, dilation, n)
    y = oe.swt_level_inv(torch.from_numpy(np.ascontiguousarray(am).reshape(-1, n)), torch.from_numpy(np.ascontiguousarray(dm).reshape(-1, n)),
                         lo, hi, dilation, scale).numpy()
    return np.moveaxis(y.reshape(am.shape), -1, axis)


def level_fwd(x, taps, dilation, scale):
    """x [..., Dz, H, W] -> the eight bands aaa .. ddd; taps = (w_lo, w_hi, h_lo, h_hi, z_lo, z_hi)."""
    out = []
    for zb in _axis_fwd(x, taps[4], taps[5], dilation, scale, -3):
        for hb in _axis_fwd(zb, taps[2], taps[3], dilation, 1.0, -2):
            out.extend(_axis_fwd(hb, taps[0], taps[1], dilation, 1.0, -1))
    return tuple(out)


def level_inv(bands, taps, dilation, scale):
    """(aaa, .., ddd) -> y: synthesis along axis -1 of the pairs (.., a / d), then along axis -2, then along axis -3."""
    u = [_axis_inv(bands[2 * p], bands[2 * p + 1], taps[0], taps[1], dilation, 1.0, -1) for p in range(4)]
    v = [_axis_inv(u[2 * d], u[2 * d + 1], taps[2], taps[3], dilation, 1.0, -2) for d in range(2)]
    return _axis_inv(v[0], v[1], taps[4], taps[5], dilation, scale, -3)


def swt_max_level(n):
    level = 0
    while n > 0 and n % 2 == 0:
        n //= 2
        level += 1
    return level


_LAST = (-3, -2, -1)


def _to_last(x, axes):
    return np.moveaxis(np.asarray(x, dtype=np.float64), axes, _LAST)


def swt3(x, dec_lo, dec_hi, level=None, axes=_LAST):
    """[cA_n, {aad .. ddd}_n, ..., {..}_1] over ``axes``, every array of x's shape."""
    cur = _to_last(x, axes)
    if level is None:
        level = min(swt_max_level(n) for n in cur.shape[-3:])
    taps = (dec_lo, dec_hi) * 3
    out = []
    for lvl in range(level):
        bands = level_fwd(cur, taps, 2 ** lvl, 1.0)
        out.append({k: np.moveaxis(t, _LAST, axes) for k, t in zip(KEYS, bands[1:])})
        cur = bands[0]
    out.append(np.moveaxis(cur, _LAST, axes))
    return out[::-1]


def iswt3(coeffs, rec_lo, rec_hi, axes=_LAST):
    cur = _to_last(coeffs[0], axes)
    taps = (rec_lo, rec_hi) * 3
    n = len(coeffs) - 1
    for pos, det in enumerate(coeffs[1:]):
        cur = level_inv((cur,) + tuple(_to_last(det[k], axes) for k in KEYS), taps, 2 ** (n - pos - 1), 0.125)
    return np.moveaxis(cur, _LAST, axes)


def level_matrix(shape, taps, dilation, scale, inverse):
    """Dense matrix of a level on a dz x h x w volume: analysis [8 n, n] (bands aaa .. ddd stacked), synthesis [n, 8 n]."""
    n = int(np.prod(shape))
    cols = []
    if not inverse:
        for k in range(n):
            e = np.zeros(n)
            e[k] = 1.0
            cols.append(np.concatenate([b.reshape(-1) for b in level_fwd(e.reshape(shape), taps, dilation, scale)]))
        return np.stack(cols, axis=1)
    for k in range(8 * n):
        e = np.zeros(8 * n)
        e[k] = 1.0
        cols.append(level_inv(tuple(e.reshape((8,) + tuple(shape))), taps, dilation, scale).reshape(-1))
    return np.stack(cols, axis=1)


def axis_matrix(n, filt, dilation, offset):
    """Dense [n, n] matrix of one filter along one periodic axis: row i, tap m reads sample (i + D (offset - m)) mod n."""
    mat = np.zeros((n, n))
    for i in range(n):
        for m, v in enumerate(filt):
            mat[i, (i + dilation * (offset - m)) % n] += v
    return mat


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


def t_level_fwd(x, taps, dilation, scale, dims=_LAST):
    out = []
    for zb in t_axis_fwd(x, taps[4], taps[5], dilation, scale, dims[0]):
        for hb in t_axis_fwd(zb, taps[2], taps[3], dilation, 1.0, dims[1]):
            out.extend(t_axis_fwd(hb, taps[0], taps[1], dilation, 1.0, dims[2]))
    return tuple(out)


def t_level_inv(bands, taps, dilation, scale, dims=_LAST):
    u = [t_axis_inv(bands[2 * p], bands[2 * p + 1], taps[0], taps[1], dilation, 1.0, dims[2]) for p in range(4)]
    v = [t_axis_inv(u[2 * d], u[2 * d + 1], taps[2], taps[3], dilation, 1.0, dims[1]) for d in range(2)]
    return t_axis_inv(v[0], v[1], taps[4], taps[5], dilation, scale, dims[0])


def t_swt3(x, dec_lo, dec_hi, level=None, axes=_LAST):
    if level is None:
        level = min(swt_max_level(x.shape[a]) for a in axes)
    taps = (dec_lo, dec_hi) * 3
    out, cur = [], x
    for lvl in range(level):
        bands = t_level_fwd(cur, taps, 2 ** lvl, 1.0, axes)
        out.append(dict(zip(KEYS, bands[1:])))
        cur = bands[0]
    out.append(cur)
    return out[::-1]


def t_iswt3(coeffs, rec_lo, rec_hi, axes=_LAST):
    taps = (rec_lo, rec_hi) * 3
    cur, n = coeffs[0], len(coeffs) - 1
    for pos, det in enumerate(coeffs[1:]):
        cur = t_level_inv((cur,) + tuple(det[k] for k in KEYS), taps, 2 ** (n - pos - 1), 0.125, axes)
    return cur
