"""DIFFERENTIABLE float64 CPU reference of the padded-convolution FWT, used only by tests (never imported by the product
package, never by bench.py).

It restates the reference's ATen op sequence per level on CPU tensors, with the four filters of the bank as tensors that stay in the
autograd graph: analysis = boundary extension (pad amounts src/ptwt/_util.py:198-228, the general arithmetic, so odd filter lengths
follow the same sequence), one stride-2 ``conv{1,2,3}d`` with the outer-product bank of the flipped decomposition filters, channel
split (src/ptwt/conv_transform.py:133-140, conv_transform_2.py:142-149, conv_transform_3.py:121-141); synthesis = ``torch.stack``,
stride-2 ``conv_transpose{1,2,3}d`` with the reconstruction filters, the crops and ``adjust_trim`` (src/ptwt/_util.py:231-244);
separable transforms = one 1-D level per axis (src/ptwt/separable_conv_transform.py).  Gradients w.r.t. the data and all four filters
come from ``torch.autograd``, to any order.

The stationary transform (``swt`` / ``iswt``, src/ptwt/stationary_transform.py:95-107, :142-156) is restated the same way: per level
the circular extension by ``D (L/2 - 1)`` and ``D (L/2)`` samples (swapped for synthesis), the stride-1 correlation with dilation
``D = 2^level`` and, for synthesis, the mean of the pair — written as index gathers of the closed form those ops amount to (any
number of wraps around the row).

A wavelet argument is either a name (taps from the committed pywt banks, float64 tensors) or a 4-tuple
``(dec_lo, dec_hi, rec_lo, rec_hi)`` of 1-D tensors, taken as they are (flips are ``torch.flip``, outer products ``torch.einsum``).
3-D levels of more than :data:`DENSE_3D_MAX_TAPS` taps run as one 1-D level per axis (the same operator; a dense L^3 kernel is slow
on the host), which the CPU tests pin against the dense form.
"""
from __future__ import annotations

import itertools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import fwt_oracle as O

DENSE_3D_MAX_TAPS = 16
_CONV = {1: F.conv1d, 2: F.conv2d, 3: F.conv3d}
_CONV_T = {1: F.conv_transpose1d, 2: F.conv_transpose2d, 3: F.conv_transpose3d}
_EINSUM = {1: "i->i", 2: "i,j->ij", 3: "i,j,k->ijk"}


def bank_of(wavelet, dtype: torch.dtype = torch.float64) -> Tuple[torch.Tensor, ...]:
    """The four filters as 1-D tensors: a tuple of tensors is returned as it is (it keeps its autograd history), anything else goes
    through :func:`oracle.fwt_oracle.filter_bank`."""
    if isinstance(wavelet, (tuple, list)) and len(wavelet) == 4 and all(isinstance(t, torch.Tensor) for t in wavelet):
        return tuple(t.reshape(-1) for t in wavelet)
    return tuple(torch.tensor(f, dtype=dtype) for f in O.filter_bank(wavelet))


def _keys(n: int) -> List[str]:
    """Band keys of an n-axis level, letter i <-> transformed axis i ('a' low, 'd' high), in band-index order."""
    return ["".join(k) for k in itertools.product("ad", repeat=n)]


def _pad_axis(x: torch.Tensor, axis: int, flen: int, mode: str) -> torch.Tensor:
    """Boundary extension of one axis by the reference's amounts, as an index gather (differentiable; the same values as torch's
    constant / replicate / reflect / circular pads and the reference's repeated half-sample mirror)."""
    n = x.shape[axis]
    padl, padr = O.get_pad(n, flen)
    O.check_pad_like_torch(n, padl, padr, mode)
    idx = O.ext_index(np.arange(-padl, n + padr), n, mode)
    out = x.index_select(axis, torch.from_numpy(np.where(idx < 0, 0, idx)))
    if mode == "zero":
        shape = [1] * x.dim()
        shape[axis] = -1
        out = out * torch.from_numpy(idx >= 0).to(x.dtype).reshape(shape)
    return out


def _crop_axis(y: torch.Tensor, axis: int, flen: int, trim: int) -> torch.Tensor:
    pad = (2 * flen - 3) // 2
    return y.narrow(axis, pad, y.shape[axis] - 2 * pad - trim)


def _analysis_dense(x: torch.Tensor, bank, mode: str, n: int) -> Dict[str, torch.Tensor]:
    """One n-axis level of [B, e_0..e_{n-1}]: pad, one strided conv with the outer-product bank, channel split."""
    flen = bank[0].shape[0]
    for a in range(n):
        x = _pad_axis(x, 1 + a, flen, mode)
    f = (torch.flip(bank[0], [0]), torch.flip(bank[1], [0]))
    keys = _keys(n)
    w = torch.stack([torch.einsum(_EINSUM[n], *[f[c == "d"] for c in k]) for k in keys]).unsqueeze(1).to(x.dtype)
    res = _CONV[n](x.unsqueeze(1), w, stride=2)
    return {k: res[:, i] for i, k in enumerate(keys)}


def _synthesis_dense(bands: Dict[str, torch.Tensor], bank, n: int, trims: Sequence[int]) -> torch.Tensor:
    """One n-axis synthesis level: stack the bands, one strided transposed conv with the (unflipped) reconstruction bank, crops."""
    flen = bank[2].shape[0]
    keys = _keys(n)
    g = (bank[2], bank[3])
    w = torch.stack([torch.einsum(_EINSUM[n], *[g[c == "d"] for c in k]) for k in keys]).unsqueeze(1)
    stacked = torch.stack([bands[k] for k in keys], 1)
    y = _CONV_T[n](stacked, w.to(stacked.dtype), stride=2)[:, 0]
    for a in range(n):
        y = _crop_axis(y, 1 + a, flen, trims[a])
    return y


def _analysis_axis(x: torch.Tensor, bank, mode: str, axis: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """One 1-D level along ``axis`` of any tensor (the separable reference's ``wavedec(..., level=1, axis=...)``)."""
    xt = x.movedim(axis, -1)
    rows = xt.reshape(-1, 1, xt.shape[-1])
    b = _analysis_dense(rows[:, 0], bank, mode, 1)
    lo, hi = (b[k].reshape(*xt.shape[:-1], -1).movedim(-1, axis) for k in ("a", "d"))
    return lo, hi


def _synthesis_axis(lo: torch.Tensor, hi: torch.Tensor, bank, axis: int, trim: int) -> torch.Tensor:
    lt, ht = lo.movedim(axis, -1), hi.movedim(axis, -1)
    y = _synthesis_dense({"a": lt.reshape(-1, lt.shape[-1]), "d": ht.reshape(-1, ht.shape[-1])}, bank, 1, [trim])
    return y.reshape(*lt.shape[:-1], -1).movedim(-1, axis)


def _analysis_level(x, bank, mode, n, per_axis):
    if not per_axis:
        return _analysis_dense(x, bank, mode, n)
    out = {"": x}
    for a in range(n):
        nxt = {}
        for key, val in out.items():
            nxt[key + "a"], nxt[key + "d"] = _analysis_axis(val, bank, mode, 1 + a)
        out = nxt
    return out


def _synthesis_level(bands, bank, n, trims, per_axis):
    if not per_axis:
        return _synthesis_dense(bands, bank, n, trims)
    cur = dict(bands)
    for pos in reversed(range(n)):
        cur = {key: _synthesis_axis(cur[key + "a"], cur[key + "d"], bank, 1 + pos, trims[pos]) for key in sorted({k[:pos] for k in cur})}
    return cur[""]


# ---- axes plumbing: move the transformed axes last, fold the rest into one batch axis -------------------------------------------------
def _fold(x: torch.Tensor, axes, n: int):
    axes = O._norm_axes(axes, x.dim(), n)
    xt = x.movedim(axes, tuple(range(x.dim() - n, x.dim())))
    lead = xt.shape[: x.dim() - n]
    return xt.reshape(-1, *xt.shape[x.dim() - n:]), (axes, lead, x.dim())


def _unfold(t: torch.Tensor, meta) -> torch.Tensor:
    axes, lead, ndim = meta
    n = len(axes)
    t = t.reshape(*lead, *t.shape[1:])
    return t.movedim(tuple(range(ndim - n, ndim)), axes)


def _per_axis(n: int, flen: int, separable: bool) -> bool:
    return separable or (n == 3 and flen > DENSE_3D_MAX_TAPS)


def _decn(x, wavelet, mode, level, axes, n, separable=False):
    bank = bank_of(wavelet)
    flen = bank[0].shape[0]
    xf, meta = _fold(x, axes, n)
    if level is None:
        level = O._max_level(xf.shape[1:], flen)
    details, cur = [], xf
    for _ in range(level):
        bands = _analysis_level(cur, bank, mode, n, _per_axis(n, flen, separable))
        cur = bands.pop("a" * n)
        details.append({k: _unfold(v, meta) for k, v in bands.items()})
    return _unfold(cur, meta), details[::-1]


def _recn(approx, details, wavelet, axes, n, separable=False):
    bank = bank_of(wavelet)
    flen = bank[2].shape[0]
    cur, meta = _fold(approx, axes, n)
    for pos, det in enumerate(details):
        det = {k: _fold(v, axes, n)[0] for k, v in det.items()}
        d0 = next(iter(det.values()))
        trims = [0] * n
        if separable:  # src/ptwt/separable_conv_transform.py:94-97: the approximation is cropped to the details, the output never is
            cur = cur[(slice(None),) + tuple(slice(0, s) for s in d0.shape[1:])]
        elif pos + 1 < len(details):
            nxt = _fold(next(iter(details[pos + 1].values())), axes, n)[0]
            trims = [O.adjust_trim(2 * cur.shape[1 + a] - flen + 2, nxt.shape[1 + a]) for a in range(n)]
        bands = dict(det)
        bands["a" * n] = cur
        cur = _synthesis_level(bands, bank, n, trims, _per_axis(n, flen, separable))
    return _unfold(cur, meta)


# ---- the reference's ten entry points (containers and default modes as in src/ptwt) ------------------------------------------------------
def wavedec(x, wavelet, *, mode: str = "reflect", level: Optional[int] = None, axis: int = -1) -> List[torch.Tensor]:
    cur, details = _decn(x, wavelet, mode, level, axis, 1)
    return [cur] + [d["d"] for d in details]


def waverec(coeffs, wavelet, *, axis: int = -1) -> torch.Tensor:
    return _recn(coeffs[0], [{"d": c} for c in coeffs[1:]], wavelet, axis, 1)


def wavedec2(x, wavelet, *, mode: str = "reflect", level: Optional[int] = None, axes=(-2, -1)):
    cur, details = _decn(x, wavelet, mode, level, axes, 2)
    # H = high along axes[0] ('da'), V = 'ad', D = 'dd' (src/ptwt/_util.py:901-905)
    return (cur,) + tuple((d["da"], d["ad"], d["dd"]) for d in details)


def waverec2(coeffs, wavelet, *, axes=(-2, -1)) -> torch.Tensor:
    return _recn(coeffs[0], [{"da": c[0], "ad": c[1], "dd": c[2]} for c in coeffs[1:]], wavelet, axes, 2)


_ORDER3 = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")


def wavedec3(x, wavelet, *, mode: str = "zero", level: Optional[int] = None, axes=(-3, -2, -1)):
    cur, details = _decn(x, wavelet, mode, level, axes, 3)
    return (cur,) + tuple({k: d[k] for k in _ORDER3} for d in details)


def waverec3(coeffs, wavelet, *, axes=(-3, -2, -1)) -> torch.Tensor:
    return _recn(coeffs[0], list(coeffs[1:]), wavelet, axes, 3)


def _fswavedec(x, wavelet, n, mode, level, axes):
    axes = tuple(range(-n, 0)) if axes is None else axes
    if level is None:  # src/ptwt/separable_conv_transform.py:140-144
        flen = bank_of(wavelet)[0].shape[0]
        level = int(min(np.log2(x.shape[a] / (flen - 1)) for a in axes))
    cur, details = _decn(x, wavelet, mode, level, axes, n, separable=True)
    order = [k for k in O._fs_order(n) if k != "a" * n]
    return (cur,) + tuple({k: d[k] for k in order} for d in details)


def _fswaverec(coeffs, wavelet, n, axes):
    axes = tuple(range(-n, 0)) if axes is None else axes
    return _recn(coeffs[0], list(coeffs[1:]), wavelet, axes, n, separable=True)


def fswavedec2(x, wavelet, *, mode: str = "reflect", level: Optional[int] = None, axes=None):
    return _fswavedec(x, wavelet, 2, mode, level, axes)


def fswavedec3(x, wavelet, *, mode: str = "reflect", level: Optional[int] = None, axes=None):
    return _fswavedec(x, wavelet, 3, mode, level, axes)


def fswaverec2(coeffs, wavelet, *, axes=None) -> torch.Tensor:
    return _fswaverec(coeffs, wavelet, 2, axes)


def fswaverec3(coeffs, wavelet, *, axes=None) -> torch.Tensor:
    return _fswaverec(coeffs, wavelet, 3, axes)


# ---- stationary transform (src/ptwt/stationary_transform.py) ------------------------------------------------------------------------------
def _circular_taps(x: torch.Tensor, flen: int, first: int, dilation: int) -> torch.Tensor:
    """[B, N] -> [B, L, N]: plane m holds ``x[(n + first - D m) mod N]``, the sample tap m meets at output n once the row is extended
    circularly and correlated with dilation D (the modulo takes any number of wraps)."""
    n = x.shape[-1]
    idx = (torch.arange(n).unsqueeze(0) + first - dilation * torch.arange(flen).unsqueeze(1)) % n
    return x.index_select(1, idx.reshape(-1)).reshape(x.shape[0], flen, n)


def _weighted(h: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """sum_m h[m] w[:, m, :] as a product and ``torch.sum`` (whose backward w.r.t. h is again a ``torch.sum``: pairwise summation, so a
    float32 run of this module — the yardstick of the float32 gradient bounds on the GPU tier — does not add up a row sequentially)."""
    return (h.to(w.dtype).reshape(1, -1, 1) * w).sum(1)


def swt_level(x: torch.Tensor, dec_lo: torch.Tensor, dec_hi: torch.Tensor, dilation: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """One analysis level of [B, N]: ``lo / hi[n] = sum_m h[m] x[(n + D (L/2 - m)) mod N]`` (pad left D (L/2 - 1), right D (L/2),
    conv1d with the flipped filters)."""
    flen = dec_lo.shape[0]
    w = _circular_taps(x, flen, dilation * (flen // 2), dilation)
    return _weighted(dec_lo, w), _weighted(dec_hi, w)


def iswt_level(a: torch.Tensor, d: torch.Tensor, rec_lo: torch.Tensor, rec_hi: torch.Tensor, dilation: int) -> torch.Tensor:
    """One synthesis level: ``y[n] = 1/2 sum_j g_lo[j] a[(n + D (L/2 - 1 - j)) mod N] + g_hi[j] d[...]`` (pad left D (L/2), right
    D (L/2 - 1), grouped conv_transpose1d cropped by the pads, mean of the pair)."""
    flen = rec_lo.shape[0]
    first = dilation * (flen // 2 - 1)
    return (_weighted(rec_lo, _circular_taps(a, flen, first, dilation)) + _weighted(rec_hi, _circular_taps(d, flen, first, dilation))) / 2


def _swt_max_level(n: int) -> int:
    """How often the extent can be halved (pywt.swt_max_level)."""
    level = 0
    while n > 0 and n % 2 == 0:
        n //= 2
        level += 1
    return level


def swt(data: torch.Tensor, wavelet, level: Optional[int] = None, *, axis: Optional[int] = None) -> List[torch.Tensor]:
    """``[cA_n, cD_n, ..., cD_1]``, every entry shaped like the input."""
    bank = bank_of(wavelet)
    cur, meta = _fold(data, axis, 1)
    if level is None:
        level = _swt_max_level(cur.shape[-1])
    out = []
    for lvl in range(level):
        cur, hi = swt_level(cur, bank[0], bank[1], 2 ** lvl)
        out.append(_unfold(hi, meta))
    out.append(_unfold(cur, meta))
    return out[::-1]


def iswt(coeffs, wavelet, *, axis: Optional[int] = None) -> torch.Tensor:
    bank = bank_of(wavelet)
    coeffs = list(coeffs)
    cur, meta = _fold(coeffs[0], axis, 1)
    details = coeffs[1:]
    for pos, det in enumerate(details):
        cur = iswt_level(cur, _fold(det, axis, 1)[0], bank[2], bank[3], 2 ** (len(details) - pos - 1))
    return _unfold(cur, meta)
