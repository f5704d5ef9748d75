"""Torch reference of the periodized transform (PyWavelets mode="periodization"; the formulas of include/mifwt.h), by index gather.

Everything runs in the dtype of its input, one tap after the other: a float64 input gives the float64 reference, differentiable by
autograd; a float32 input gives the float32 tap-by-tap variant whose error against the float64 run on the same inputs is the yardstick
of the float32 bounds (``e_ref32``).  Taps are sequences of floats in PyWavelets order.

    dwt_axis(x, lo, hi, dim)            one analysis level along ``dim``                -> (cA, cD), ceil(n / 2) entries
    idwt_axis(a, d, lo, hi, dim, n)     one synthesis level along ``dim``, n in {2M, 2M-1}
    level_fwd(x, bank, ndim)            one N-D level over the last ``ndim`` axes       -> list of 2^ndim bands (bit (ndim-1-a) <=> axis a high)
    level_inv(bands, bank, ndim, ext)   its inverse
    wavedecn / waverecn                 multi-level: [approx, [bands 1 ..] per level, coarsest first]
"""
import json
import os

import numpy as np
import torch

_GOLDENS = []


def goldens():
    """The cases of tests/golden/pywt_per.npz (make_pywt_per_goldens.py): dicts with "ndim", "wavelet", "shape", "level" and float64
    tensors "x", "rec" and "coeffs" = {name: tensor} in the naming of tests/_golden.flatten_coeffs."""
    if not _GOLDENS:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pywt_per.npz"))
        data = z["data"]

        def get(ref):
            off, shape = ref
            return torch.from_numpy(data[off:off + int(np.prod(shape))].reshape(shape).copy())

        for c in json.loads(str(z["index"])):
            _GOLDENS.append({**{k: c[k] for k in ("ndim", "wavelet", "level")}, "shape": tuple(c["shape"]), "x": get(c["x"]),
                             "rec": get(c["rec"]), "coeffs": {name: get(ref) for name, ref in c["coeffs"]}})
    return _GOLDENS


def flat_ref(coeffs, ndim):
    """{name: tensor} of a `wavedecn` result of this module, named like the goldens (2-D: h = 'da' = band 2, v = 'ad' = band 1)."""
    out = {"a": coeffs[0]}
    for i, det in enumerate(coeffs[1:]):
        if ndim == 1:
            out["%d" % i] = det[0]
        elif ndim == 2:
            out["%d_h" % i], out["%d_v" % i], out["%d_d" % i] = det[1], det[0], det[2]
        else:
            for s, t in enumerate(det, start=1):
                out["%d_%s" % (i, format(s, "03b").replace("0", "a").replace("1", "d"))] = t
    return out


def _taps(t, like):
    return [float(v) for v in t] if like.dtype == torch.float64 else [float(np.float32(v)) for v in t]


def dwt_axis(x, lo, hi, dim):
    n = x.shape[dim]
    nt = n + (n & 1)
    m, flen = nt // 2, len(lo)
    xm = x.movedim(dim, -1)
    k = torch.arange(m, device=x.device)
    lo, hi = _taps(lo, x), _taps(hi, x)
    ca = cd = None
    for j in range(flen):
        idx = torch.clamp((2 * k + flen // 2 - j) % nt, max=n - 1)
        g = xm.index_select(-1, idx)
        ca = lo[j] * g if ca is None else ca + lo[j] * g
        cd = hi[j] * g if cd is None else cd + hi[j] * g
    return ca.movedim(-1, dim), cd.movedim(-1, dim)


def idwt_axis(a, d, lo, hi, dim, n_out=None):
    m, flen = a.shape[dim], len(lo)
    am, dm = a.movedim(dim, -1), d.movedim(dim, -1)
    lo, hi = _taps(lo, a), _taps(hi, a)
    k = torch.arange(m, device=a.device)
    y = torch.zeros(*am.shape[:-1], 2 * m, dtype=a.dtype, device=a.device)
    for t in range(flen):
        pos = (2 * k + t - flen // 2 + 1) % (2 * m)
        y = y.index_add(-1, pos, lo[t] * am + hi[t] * dm)
    if n_out is not None:
        assert n_out in (2 * m, 2 * m - 1)
        y = y[..., :n_out]
    return y.movedim(-1, dim)


def level_fwd(x, bank, ndim):
    dec_lo, dec_hi = bank[0], bank[1]
    bands = {0: x}
    for a in reversed(range(ndim)):
        bit, nxt = 1 << (ndim - 1 - a), {}
        for s, t in bands.items():
            nxt[s], nxt[s | bit] = dwt_axis(t, dec_lo, dec_hi, a - ndim)
        bands = nxt
    return [bands[s] for s in range(1 << ndim)]


def level_inv(bands, bank, ndim, out_extent=None):
    rec_lo, rec_hi = bank[2], bank[3]
    cur = {s: t for s, t in enumerate(bands)}
    for a in range(ndim):
        bit, nxt = 1 << (ndim - 1 - a), {}
        for s, t in cur.items():
            if not s & bit:
                nxt[s] = idwt_axis(t, cur[s | bit], rec_lo, rec_hi, a - ndim, None if out_extent is None else int(out_extent[a]))
        cur = nxt
    return cur[0]


def wavedecn(x, bank, ndim, level):
    out, cur = [], x
    for _ in range(level):
        bands = level_fwd(cur, bank, ndim)
        out.insert(0, bands[1:])
        cur = bands[0]
    return [cur] + out


def waverecn(coeffs, bank, ndim):
    cur = coeffs[0]
    for pos, det in enumerate(coeffs[1:]):
        ext = [2 * m for m in cur.shape[-ndim:]]
        if pos + 2 < len(coeffs):
            nxt = coeffs[pos + 2][0].shape[-ndim:]
            for a in range(ndim):
                assert ext[a] - nxt[a] in (0, 1), "coefficient shapes do not belong to one decomposition"
                ext[a] = int(nxt[a])
        cur = level_inv([cur, *det], bank, ndim, ext)
    return cur


def matrix(n, lo, hi):
    """The [2 ceil(n/2), n] float64 matrix of one analysis level (rows: cA then cD)."""
    ca, cd = dwt_axis(torch.eye(n, dtype=torch.float64), lo, hi, 0)
    return torch.cat([ca, cd], 0)


# A band whose norm is below this share of the norm of the transform's input is ZERO in exact arithmetic (the details of an axis of
# one sample: a filter whose taps sum to zero applied to a constant); what it holds is rounding of terms of the input's size, so its
# error is taken relative to the input's norm.  Every other band is far above it (the smallest genuine band of the goldens is at 2e-3 of it).
ZERO_BAND = 1e-9


def relerr(got, want, scale=0.0):
    """Norm-wise relative error of one tensor; ``scale`` = the norm of the transform's input: a band that is zero in exact arithmetic
    (``ZERO_BAND``) is measured against it, every other band against its own norm."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    den = float(want.norm())
    if scale and den < ZERO_BAND * scale:
        den = float(scale)
    return float((got - want).norm()) / den if den > 0 else float((got - want).norm())


def e_ref32(fn, *inputs, scale=0.0):
    """Worst norm-wise error (:func:`relerr`, with its ``scale``) over the outputs of ``fn`` run on float32 copies of ``inputs`` against
    its float64 run on the SAME (already float32-representable) values.  ``fn`` returns a tensor or a list of tensors."""
    def run(dt):
        out = fn(*[t.to(dt) for t in inputs])
        return list(out) if isinstance(out, (list, tuple)) else [out]

    return max([relerr(a, b, scale) for a, b in zip(run(torch.float32), run(torch.float64))] + [0.0])
