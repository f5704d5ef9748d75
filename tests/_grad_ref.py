"""Shared helpers of the data-gradient tests (tests/test_gpu_data_gradients.py, tests/test_data_gradients_host.py): one differentiable
call with a wavelet NAME (fixed taps) through the float64 differentiable CPU reference (oracle/torch_autograd_ref.py), seeded Gaussian
inputs and cotangents, and the three error measures of a compared tensor.

A case is ``(fn, shape, wavelet, mode, level, dtype)`` plus optional ``axes``; :func:`reference` yields everything one side of the
comparison needs, computed by ``R`` in ``compute`` precision from inputs quantised to the case's dtype first:

* ``coeffs``   the flattened coefficients of ``R.<fn>(x)``;
* ``gx``       d/dx of ``sum_i <w_i, c_i>`` with Gaussian ``w_i``;
* ``rec``      ``R.<rec>(leaves)``, the leaves being the float64 coefficients quantised to the dtype;
* ``gleaves``  the gradients of ``<v, rec(leaves)>`` w.r.t. every leaf, Gaussian ``v``.

The cotangents are Gaussian on purpose: a smooth cotangent (the suite's ``cos(0.37 k + i)`` weights) is almost annihilated by the
high-pass adjoint, so the relative error of a float32 chain is cancellation noise (3.5e-6 .. 2.5e-5 norm-wise for the float32 reference
itself) and a bound derived from it would be 20 - 100 times too loose to see a wrong border sample.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import fwt_oracle as O
from oracle import torch_autograd_ref as R
from tests import _golden as G

# analysis entry point -> (synthesis entry point, transformed axes)
FNS = {"wavedec": ("waverec", 1), "wavedec2": ("waverec2", 2), "fswavedec2": ("fswaverec2", 2), "wavedec3": ("waverec3", 3),
       "fswavedec3": ("fswaverec3", 3)}
MEASURES = ("norm", "maxabs", "border")


def gaussian(shape: Sequence[int], seed: int, dtype: torch.dtype) -> torch.Tensor:
    """A seeded standard-normal tensor, drawn in float64 and quantised to ``dtype`` (CPU)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)


def flat(coeffs) -> List[torch.Tensor]:
    return [t for _, t in G.flatten_coeffs(coeffs)]


def rebuild(template, leaves: Sequence[torch.Tensor]):
    """The container of ``template`` (a list / tuple of tensors, 3-tuples or dicts) filled with ``leaves`` in :func:`flat` order."""
    it = iter(leaves)
    out = []
    for c in template:
        if isinstance(c, dict):
            out.append({k: next(it) for k in c})
        elif isinstance(c, (tuple, list)):
            out.append(tuple(next(it) for _ in c))
        else:
            out.append(next(it))
    return type(template)(out) if isinstance(template, (tuple, list)) else out


def filt_len(wavelet: str) -> int:
    return len(O.filter_bank(wavelet)[0])


def norm_axes(fn: str, ndim_tensor: int, axes) -> Tuple[int, ...]:
    n = FNS[fn][1]
    if axes is None:
        axes = tuple(range(-n, 0))
    if isinstance(axes, int):
        axes = (axes,)
    return tuple(a % ndim_tensor for a in axes)


def border_width(flen: int, n: int) -> int:
    """Samples of an axis of extent ``n`` within reach of a boundary extension of one level: ``L - 1 + n % 2`` per edge (the border
    kernels' own width)."""
    return flen - 1 + n % 2


def border_mask(shape: Sequence[int], axes: Sequence[int], flen: int) -> np.ndarray:
    """True for the samples within ``L - 1 + N % 2`` of any edge of any transformed axis."""
    mask = np.zeros(tuple(shape), dtype=bool)
    for a in axes:
        n = shape[a]
        b = min(border_width(flen, n), n)
        idx = [slice(None)] * len(shape)
        idx[a] = slice(0, b)
        mask[tuple(idx)] = True
        idx[a] = slice(n - b, n)
        mask[tuple(idx)] = True
    return mask


def measures(got, want, mask: Optional[np.ndarray] = None) -> Dict[str, float]:
    """Norm-wise error, max-abs error over the largest reference value and (with a mask) the norm-wise error of the masked samples."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    out = {"norm": float(G.relerr(got, want)), "maxabs": float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-300))}
    if mask is not None:
        out["border"] = float(G.relerr(got[mask], want[mask]))
    return out


def rowwise_measures(got, want_distinct, distinct: int, mask: Optional[np.ndarray] = None) -> Dict[str, float]:
    """:func:`measures` of ``got`` [rows, ...] against a reference known for ``distinct`` rows only, row ``r`` of ``got`` being a copy of
    source row ``r % distinct``: the same numbers as against the full, tiled reference, without ever building it.  ``mask``: the border
    strip of ONE row (shape ``got.shape[1:]``)."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want_distinct, dtype=np.float64)
    assert got.shape[1:] == want.shape[1:] and want.shape[0] == distinct, (got.shape, want.shape)
    num = den = bnum = bden = worst = 0.0
    for r0 in range(0, got.shape[0], distinct):
        blk = got[r0 : r0 + distinct]
        w = want[: blk.shape[0]]
        diff = blk - w
        num += float(np.sum(diff * diff))
        den += float(np.sum(w * w))
        worst = max(worst, float(np.abs(diff).max()))
        if mask is not None:
            bnum += float(np.sum(diff[:, mask] ** 2))
            bden += float(np.sum(w[:, mask] ** 2))
    out = {"norm": float(np.sqrt(num) / np.sqrt(den)) if den > 0 else float(np.sqrt(num)),
           "maxabs": worst / max(float(np.abs(want).max()), 1e-300)}
    if mask is not None:
        out["border"] = float(np.sqrt(bnum) / np.sqrt(bden)) if bden > 0 else float(np.sqrt(bnum))
    return out


def tile_rows(t: torch.Tensor, rows: int) -> torch.Tensor:
    """``rows`` rows, row ``r`` a copy of row ``r % len(t)`` of ``t``."""
    reps = -(-rows // t.shape[0])
    return t.repeat(reps, *([1] * (t.dim() - 1)))[:rows].contiguous()


def _bank(wavelet: str, compute: torch.dtype):
    """float64: the name itself (float64 taps of the committed banks); float32: the same taps rounded to float32."""
    return wavelet if compute == torch.float64 else R.bank_of(wavelet, dtype=torch.float32)


def inputs(fn: str, shape, wavelet: str, mode: str, level: int, dtype: torch.dtype, axes=None, seed: int = 0):
    """The inputs of a case, quantised to its dtype: ``x``, the cotangents ``w`` of the coefficients, the ``leaves`` of the
    reconstruction (the float64 reference coefficients, quantised), the cotangent ``v`` of the reconstruction; and the container
    ``template`` of the coefficients."""
    rec = FNS[fn][0]
    kw = {"mode": mode, "level": level}
    akw = {} if axes is None else ({"axis": axes} if fn == "wavedec" else {"axes": axes})
    x = gaussian(shape, 1000 + seed, dtype)
    with torch.no_grad():
        template = getattr(R, fn)(x.double(), wavelet, **kw, **akw)
        leaves = [t.to(dtype) for t in flat(template)]
        y = getattr(R, rec)(rebuild(template, [t.double() for t in leaves]), wavelet, **akw)
    w = [gaussian(t.shape, 2000 + 17 * seed + i, dtype) for i, t in enumerate(leaves)]
    v = gaussian(y.shape, 3000 + seed, dtype)
    return {"x": x, "w": w, "leaves": leaves, "v": v, "template": template, "kw": kw, "akw": akw}


def chain(fn: str, wavelet: str, inp, compute: torch.dtype = torch.float64):
    """The four results of a case through ``R`` in ``compute`` precision (float32: float32 inputs and float32 taps)."""
    rec = FNS[fn][0]
    bank = _bank(wavelet, compute)
    x = inp["x"].to(compute).requires_grad_(True)
    coeffs = flat(getattr(R, fn)(x, bank, **inp["kw"], **inp["akw"]))
    (gx,) = torch.autograd.grad(sum((w.to(compute) * c).sum() for w, c in zip(inp["w"], coeffs)), x)
    leaves = [t.to(compute).requires_grad_(True) for t in inp["leaves"]]
    y = getattr(R, rec)(rebuild(inp["template"], leaves), bank, **inp["akw"])
    gl = torch.autograd.grad((inp["v"].to(compute) * y).sum(), leaves)
    return {"coeffs": [c.detach() for c in coeffs], "gx": gx.detach(), "rec": y.detach(), "gleaves": [g.detach() for g in gl]}


def compare(got, want, fn: str, wavelet: str, axes=None) -> Dict[str, float]:
    """Worst value of every measure over the tensors of two :func:`chain`-shaped results (the border strip for d/dx only)."""
    worst = {m: 0.0 for m in MEASURES}

    def take(m):
        for k, v in m.items():
            worst[k] = max(worst[k], v)

    for a, b in zip(got["coeffs"] + [got["rec"]] + got["gleaves"], want["coeffs"] + [want["rec"]] + want["gleaves"]):
        take(measures(a.double().numpy(), b.double().numpy()))
    shape = tuple(want["gx"].shape)
    take(measures(got["gx"].double().numpy(), want["gx"].double().numpy(), border_mask(shape, norm_axes(fn, len(shape), axes), filt_len(wavelet))))
    return worst


def reference_deviation(fn, shape, wavelet, mode, level, axes=None, seed: int = 0) -> Dict[str, float]:
    """What the float32 run of the reference itself (float32 inputs, float32 taps) deviates from its float64 run on the same quantised
    inputs, per measure: the yardstick of the float32 bounds."""
    inp = inputs(fn, shape, wavelet, mode, level, torch.float32, axes, seed)
    return compare(chain(fn, wavelet, inp, torch.float32), chain(fn, wavelet, inp, torch.float64), fn, wavelet, axes)
