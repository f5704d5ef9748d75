"""Torch reference of the PADDED transform in all eight signal-extension modes: the five of the oracle ("zero", "constant", "reflect",
"periodic", "symmetric") and PyWavelets' "smooth", "antisymmetric" and "antireflect" (the closed forms of include/mifwt.h).

A level is :func:`extend` — the extended signal built explicitly: every extended sample is a sum of at most three source samples with
integer weights — followed by a stride-2 valid correlation, one tap after the other.  Everything runs in the dtype of its input: a
float64 input gives the float64 reference, differentiable by autograd; a float32 input gives the float32 variant whose error against
the float64 run on the same inputs is the yardstick of the float32 bounds (``e_ref32``).  Taps are sequences of floats in PyWavelets order.

    terms(i, n, mode)                    the (index, weight) terms of xe[i], as integer tensors
    extend(x, mode, pl, pr, dim)         xe[-pl .. n + pr) along ``dim``
    ext_matrix(n, mode, pl, pr)          E [n + pl + pr, n], float64
    dwt_axis(x, lo, hi, mode, dim)       one analysis level along ``dim``              -> (cA, cD), floor((n + L - 1) / 2) entries
    adj_axis(ga, gd, lo, hi, mode, n, dim)   its transpose: T over the padded extent, folded with E^T
    idwt_axis(a, d, lo, hi, dim)         one (mode-free) padded synthesis level, 2 M - L + 2 samples
    level_fwd / level_adj / level_inv    N-D, separable, bands in the order bit (ndim-1-a) <=> axis a high
    wavedecn / waverecn                  multi-level: [approx, [bands 1 ..] per level, coarsest first]
"""
import numpy as np
import torch

from tests._per_ref import ZERO_BAND, e_ref32, relerr  # noqa: F401  (the zero-band rule is the periodized reference's)

OLD_MODES = ("zero", "constant", "reflect", "periodic", "symmetric")
NEW_MODES = ("smooth", "antisymmetric", "antireflect")
MODES = OLD_MODES + NEW_MODES


def terms(i, n, mode):
    """[(idx, w), ...] with int64 tensors shaped like ``i``: xe[i] = sum_t w_t x[idx_t].  Floor division throughout."""
    i = torch.as_tensor(i, dtype=torch.int64)
    zero, one = torch.zeros_like(i), torch.ones_like(i)
    inside = (i >= 0) & (i < n)
    if mode == "zero":
        return [(torch.where(inside, i, zero), inside.to(torch.int64))]
    if mode == "constant":
        return [(i.clamp(0, n - 1), one)]
    if mode == "periodic":
        return [(i % n, one)]
    if mode == "symmetric" or mode == "antisymmetric":
        q, r = i // n, i % n
        odd = (q % 2) == 1
        sign = torch.where(odd, -one, one) if mode == "antisymmetric" else one
        return [(torch.where(odd, n - 1 - r, r), sign)]
    if n == 1:  # reflect / smooth / antireflect of one sample: that sample
        return [(zero, one)]
    if mode == "reflect":
        r = i % (2 * (n - 1))
        return [(torch.where(r <= n - 1, r, 2 * (n - 1) - r), one)]
    if mode == "antireflect":
        p = n - 1
        q, r = i // p, i % p
        odd = (q % 2) == 1
        out = [(torch.where(odd, p - r, r), torch.where(odd, -one, one)),
               (zero + (n - 1), torch.where(odd, q + 1, q)),
               (zero, torch.where(odd, -(q - 1), -q))]
        # (inside the signal the three terms collapse to x[i]: i = n - 1 is q = 1, r = 0, that is -x[n-1] + 2 x[n-1]; keep it exact)
        return [(torch.where(inside, i, out[0][0]), torch.where(inside, one, out[0][1])),
                (out[1][0], torch.where(inside, zero, out[1][1])), (out[2][0], torch.where(inside, zero, out[2][1]))]
    if mode == "smooth":
        left, right = i < 0, i >= n
        k = i - n + 1
        return [(torch.where(left, zero, torch.where(right, zero + (n - 1), i)), torch.where(left, 1 - i, torch.where(right, 1 + k, one))),
                (torch.where(left, one, torch.where(right, zero + (n - 2), zero)), torch.where(left, i, torch.where(right, -k, zero)))]
    raise ValueError(mode)


def extend(x, mode, pl, pr, dim):
    """The extended signal xe[-pl .. n + pr) along ``dim``, in the dtype of ``x``."""
    n = x.shape[dim]
    xm = x.movedim(dim, -1)
    out = None
    for idx, w in terms(torch.arange(-pl, n + pr), n, mode):
        t = xm.index_select(-1, idx.to(x.device)) * w.to(x.dtype).to(x.device)
        out = t if out is None else out + t
    return out.movedim(-1, dim)


def ext_matrix(n, mode, pl, pr):
    return extend(torch.eye(n, dtype=torch.float64), mode, pl, pr, 0)


def pads(n, flen):
    return flen - 2, flen - 2 + (n & 1)


def _taps(t, like):
    return [float(v) for v in t] if like.dtype == torch.float64 else [float(np.float32(v)) for v in t]


def dwt_axis(x, lo, hi, mode, dim):
    n, flen = x.shape[dim], len(lo)
    pl, pr = pads(n, flen)
    m = (n + flen - 1) // 2
    xe = extend(x, mode, pl, pr, dim).movedim(dim, -1)
    lo, hi = _taps(lo, x), _taps(hi, x)
    k = torch.arange(m, device=x.device)
    ca = cd = None
    for j in range(flen):
        g = xe.index_select(-1, 2 * k + 1 - j + pl)
        ca = lo[j] * g if ca is None else ca + lo[j] * g
        cd = hi[j] * g if cd is None else cd + hi[j] * g
    return ca.movedim(-1, dim), cd.movedim(-1, dim)


def adj_axis(ga, gd, lo, hi, mode, n, dim):
    """The transpose of :func:`dwt_axis` at extent ``n``: the uncropped transposed convolution T over the padded extent, then the fold
    g_x[s] = sum_p E[p, s] T[p]."""
    flen, m = len(lo), ga.shape[dim]
    pl, pr = pads(n, flen)
    assert m == (n + flen - 1) // 2
    am, dm = ga.movedim(dim, -1), gd.movedim(dim, -1)
    lo, hi = _taps(lo, ga), _taps(hi, ga)
    k = torch.arange(m, device=ga.device)
    t = torch.zeros(*am.shape[:-1], n + pl + pr, dtype=ga.dtype, device=ga.device)
    for j in range(flen):
        t = t.index_add(-1, 2 * k + 1 - j + pl, lo[j] * am + hi[j] * dm)
    e = ext_matrix(n, mode, pl, pr).to(ga.dtype).to(ga.device)
    return (t @ e).movedim(-1, dim)


def idwt_axis(a, d, lo, hi, dim):
    """The padded synthesis level (no mode): y_full[2 k + t] += rec_lo[t] a[k] + rec_hi[t] d[k], L - 2 samples cropped on both sides."""
    m, flen = a.shape[dim], len(lo)
    am, dm = a.movedim(dim, -1), d.movedim(dim, -1)
    lo, hi = _taps(lo, a), _taps(hi, a)
    k = torch.arange(m, device=a.device)
    y = torch.zeros(*am.shape[:-1], 2 * m + flen - 2, dtype=a.dtype, device=a.device)
    for t in range(flen):
        y = y.index_add(-1, 2 * k + t, lo[t] * am + hi[t] * dm)
    return y[..., flen - 2: 2 * m].movedim(-1, dim)


def level_fwd(x, bank, mode, ndim):
    dec_lo, dec_hi = bank[0], bank[1]
    bands = {0: x}
    for a in reversed(range(ndim)):
        bit, nxt = 1 << (ndim - 1 - a), {}
        for s, t in bands.items():
            nxt[s], nxt[s | bit] = dwt_axis(t, dec_lo, dec_hi, mode, a - ndim)
        bands = nxt
    return [bands[s] for s in range(1 << ndim)]


def level_adj(bands, bank, mode, ndim, extent):
    dec_lo, dec_hi = bank[0], bank[1]
    cur = {s: t for s, t in enumerate(bands)}
    for a in range(ndim):
        bit, nxt = 1 << (ndim - 1 - a), {}
        for s, t in cur.items():
            if not s & bit:
                nxt[s] = adj_axis(t, cur[s | bit], dec_lo, dec_hi, mode, int(extent[a]), a - ndim)
        cur = nxt
    return cur[0]


def level_inv(bands, bank, ndim):
    rec_lo, rec_hi = bank[2], bank[3]
    cur = {s: t for s, t in enumerate(bands)}
    for a in range(ndim):
        bit, nxt = 1 << (ndim - 1 - a), {}
        for s, t in cur.items():
            if not s & bit:
                nxt[s] = idwt_axis(t, cur[s | bit], rec_lo, rec_hi, a - ndim)
        cur = nxt
    return cur[0]


def wavedecn(x, bank, mode, ndim, level):
    out, cur = [], x
    for _ in range(level):
        bands = level_fwd(cur, bank, mode, ndim)
        out.insert(0, bands[1:])
        cur = bands[0]
    return [cur] + out


def waverecn(coeffs, bank, ndim):
    """The padded reconstruction: a running approximation one sample longer than the next level's details loses its last sample."""
    cur = coeffs[0]
    for det in coeffs[1:]:
        idx = [slice(None)] * cur.dim()
        for a in range(1, ndim + 1):
            assert cur.shape[-a] - det[0].shape[-a] in (0, 1), "coefficient shapes do not belong to one decomposition"
            idx[-a] = slice(0, det[0].shape[-a])
        cur = level_inv([cur[tuple(idx)], *det], bank, ndim)
    return cur


def matrix(n, lo, hi, mode):
    """The [2 M, n] float64 matrix of one analysis level (rows: cA then cD)."""
    ca, cd = dwt_axis(torch.eye(n, dtype=torch.float64), lo, hi, mode, 0)
    return torch.cat([ca, cd], 0)
