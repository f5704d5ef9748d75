"""TEST-ONLY torch reference of the multiresolution analysis (``ptwt_amd.mra``, csrc/mifwt_mra.hip), from the closed forms of
include/mifwt.h.

Everything runs along the LAST axis in the dtype of its input, one tap after the other: a float64 input gives the float64 reference,
differentiable by autograd; a float32 input gives the float32 tap-by-tap variant whose error against the float64 run on the same
inputs is the yardstick of the float32 bounds (``e_ref32``, tests/_per_ref.py).

    analysis(x, bank, level, transform, mode)     [cA_n, cD_n, .., cD_1]: the stationary levels of tests/_swt2_ref.py, the periodized
                                                  ones of tests/_per_ref.py, padded ones by explicit extension (pinned to the oracle)
    synthesis(coeffs, bank, transform, mode)      the two-band synthesis, level by level
    mra(x, wavelet, level, transform, mode, axis) THE DEFINITION: component i = synthesis of the container with every other band zeroed,
                                                  cropped to x's extent
    swt_cascade(coeffs, bank, wrong=None)         the same components of a stationary container as cascades of ONE-input stages
                                                  D_j = U_1 .. U_{j-1} G_j W_j, S_n = U_1 .. U_n V_n — what the kernel computes —, and
                                                  three deliberately wrong engines (tests/test_mra_host.py)
"""
import numpy as np
import torch

from oracle import fwt_oracle as O
from tests import _per_ref as P
from tests import _swt2_ref as S2
from tests._per_ref import e_ref32, relerr  # noqa: F401

PERIODIZATION = "periodization"
PADDED = O.MODES + ("smooth",)


def bank_of(wavelet):
    """(dec_lo, dec_hi, rec_lo, rec_hi) as lists of floats."""
    return tuple([float(v) for v in t] for t in O.filter_bank(wavelet))


def _t(taps, like):
    return [float(v) for v in taps] if like.dtype == torch.float64 else [float(np.float32(v)) for v in taps]


# ---- padded levels ---------------------------------------------------------------------------------------------------------------------
def extend(x, mode, pl, pr):
    """xe[-pl .. n + pr) along the last axis.  "smooth": the straight line through the two end samples on either side."""
    n = x.shape[-1]
    i = torch.arange(-pl, n + pr)
    if mode == "smooth":
        if n == 1:
            return x.index_select(-1, torch.zeros_like(i))
        left, right = (i < 0).to(x.dtype), (i >= n).to(x.dtype)
        inner = x.index_select(-1, i.clamp(0, n - 1))
        slope_l, slope_r = x[..., 1:2] - x[..., 0:1], x[..., n - 1:n] - x[..., n - 2:n - 1]
        return inner + left * i.to(x.dtype) * slope_l + right * (i - (n - 1)).to(x.dtype) * slope_r
    idx = torch.from_numpy(O.ext_index(i.numpy(), n, mode))
    return x.index_select(-1, idx.clamp(min=0)) * (idx >= 0).to(x.dtype)


def dwt_pad(x, lo, hi, mode):
    """One padded analysis level: floor((n + L - 1) / 2) coefficients, c[k] = sum_j h[j] xe[2k + 1 - j] with xe the extended signal."""
    n, flen = x.shape[-1], len(lo)
    pl, pr = flen - 2, flen - 2 + (n & 1)
    xe = extend(x, mode, pl, pr)
    lo, hi = _t(lo, x), _t(hi, x)
    k = torch.arange((n + flen - 1) // 2)
    ca = cd = None
    for j in range(flen):
        g = xe.index_select(-1, 2 * k + 1 - j + pl)
        ca = lo[j] * g if ca is None else ca + lo[j] * g
        cd = hi[j] * g if cd is None else cd + hi[j] * g
    return ca, cd


def idwt_pad(a, d, lo, hi, n_out=None):
    """One padded synthesis level: y[n] = sum_k a[k] rec_lo[n + L - 2 - 2k] + d[k] rec_hi[..], n in [0, n_out), n_out = 2 M - L + 2 or
    one less."""
    m, flen = a.shape[-1], len(lo)
    lo, hi = _t(lo, a), _t(hi, a)
    k = torch.arange(m)
    y = torch.zeros(*a.shape[:-1], 2 * m + flen - 2, dtype=a.dtype)
    for t in range(flen):
        y = y.index_add(-1, 2 * k + t, lo[t] * a + hi[t] * d)
    full = 2 * m - flen + 2
    n_out = full if n_out is None else n_out
    assert n_out in (full, full - 1)
    return y[..., flen - 2: flen - 2 + n_out]


# ---- containers ------------------------------------------------------------------------------------------------------------------------
def analysis(x, bank, level, transform, mode=PERIODIZATION):
    out, cur = [], x
    for lvl in range(level):
        if transform == "swt":
            cur, det = S2.t_axis_fwd(cur, _t(bank[0], x), _t(bank[1], x), 2 ** lvl, 1.0, -1)
        elif mode == PERIODIZATION:
            cur, det = P.dwt_axis(cur, bank[0], bank[1], -1)
        else:
            cur, det = dwt_pad(cur, bank[0], bank[1], mode)
        out.append(det)
    out.append(cur)
    return out[::-1]


def synthesis(coeffs, bank, transform, mode=PERIODIZATION):
    cur, n = coeffs[0], len(coeffs) - 1
    for pos, det in enumerate(coeffs[1:]):
        if transform == "swt":
            cur = S2.t_axis_inv(cur, det, _t(bank[2], cur), _t(bank[3], cur), 2 ** (n - pos - 1), 0.5, -1)
            continue
        circular = mode == PERIODIZATION
        full = 2 * cur.shape[-1] - (0 if circular else len(bank[2]) - 2)
        n_out = full
        if pos + 2 < len(coeffs):
            n_out = coeffs[pos + 2].shape[-1]
            assert n_out in (full, full - 1), "coefficient shapes do not belong to one decomposition"
        cur = P.idwt_axis(cur, det, bank[2], bank[3], -1, n_out) if circular else idwt_pad(cur, det, bank[2], bank[3], n_out)
    return cur


def components(coeffs, bank, n, transform, mode=PERIODIZATION):
    out = []
    for i in range(len(coeffs)):
        only = [c if k == i else torch.zeros_like(c) for k, c in enumerate(coeffs)]
        out.append(synthesis(only, bank, transform, mode)[..., :n])
    return out


def mra(x, wavelet, level, transform="swt", mode=PERIODIZATION, axis=-1):
    """[S_n, D_n, .., D_1] of ``x`` along ``axis``, each of x's shape, in x's dtype."""
    if level == 0:
        return [x]
    bank = bank_of(wavelet)
    xm = x.movedim(axis, -1)
    parts = components(analysis(xm, bank, level, transform, mode), bank, xm.shape[-1], transform, mode)
    return [p.movedim(-1, axis) for p in parts]


# ---- the cascade of one-input stages (stationary) ----------------------------------------------------------------------------------------
def swt_stage(c, r, dilation, scale=0.5):
    """y[n] = 0.5 sum_i r[i] c[(n + D (L/2 - 1 - i)) mod N]."""
    flen = len(r)
    r = _t(r, c)
    y = None
    for i in range(flen):
        g = r[i] * torch.roll(c, -dilation * (flen // 2 - 1 - i), -1)
        y = g if y is None else y + g
    return scale * y


WRONG = ("hi_everywhere", "no_half", "dilations_reversed")


def swt_cascade(coeffs, bank, wrong=None):
    """The components of a stationary container ``[cA_n, cD_n, .., cD_1]``: band of level j through the stage of level j with rec_hi
    (rec_lo for cA_n), then the stages of levels j - 1 .. 1 with rec_lo, the stage of level l at dilation 2^(l-1).  ``wrong``: one of
    ``WRONG`` — rec_hi on every stage of a detail / the factor 0.5 dropped / the dilations 1 .. 2^(j-1) applied in that order."""
    assert wrong is None or wrong in WRONG
    n = len(coeffs) - 1
    out = []
    for i, c in enumerate(coeffs):
        j = n if i == 0 else n + 1 - i
        levels = list(range(j, 0, -1))
        dil = [2 ** (l - 1) for l in levels]
        if wrong == "dilations_reversed":
            dil = dil[::-1]
        cur = c
        for s, d in enumerate(dil):
            hi = i > 0 and (s == 0 or wrong == "hi_everywhere")
            cur = swt_stage(cur, bank[3] if hi else bank[2], d, 1.0 if wrong == "no_half" else 0.5)
        out.append(cur)
    return out
