"""bfloat16 forms of the impulse-probe helpers of ``tests/_probe_ref.py`` (host only; that module is imported, not changed).

bfloat16 is the library's second 16-bit STORAGE type (f32 arithmetic): 8 significant bits, unit roundoff 2^-8, the
exponent range of float32.  What differs from the float16 helpers:

  * a store: half the bf16 spacing at the bound of the result's magnitude, 2^(E-8) in the binade [2^E, 2^(E+1)) — no subnormals within
    reach of any test (the smallest normal is 2^-126);
  * the tap pairs of the matrix-core kernels (ids 11 / 23, mifwt_mfma_elem.h): th = RN_bf16(t32), tl = RN_bf16(t32 - th) with t32 the
    double tap cast to float.  r = t32 - th is exact in float (|r| <= 2^(E-8) for |t32| in [2^E, 2^(E+1)), a multiple of 2^(E-23): 15
    bits) and |r| <= 2^-8 |t32|; tl errs by at most 2^-8 |r|: the RESIDUAL is at most 2^-16 |t32| — a RELATIVE accuracy (the f16 pair's is
    absolute, ``_probe_ref.pair16_err``), 1/256 of the output's unit roundoff;
  * bf16 x bf16 products are exact in f32 (8 + 8 significant bits); of the 2 x 64 products of an output 2 L are not structural zeros.

The bound is the recurrence of ``_probe_ref.axis_pass`` term by term, with these two pieces exchanged; nothing is fitted to outputs.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from tests import _probe_ref as R

UBF16 = 2.0 ** -8  # unit roundoff of bfloat16


# --------------------------------------------------------------------------------------------------- bf16 helpers
def bf16_up(mag: torch.Tensor) -> torch.Tensor:
    """The magnitudes (>= 0, float64) rounded UP to bfloat16 (the larger bf16 neighbour), as float64."""
    h = mag.to(torch.float32).to(torch.bfloat16)
    bits = h.view(torch.int16).to(torch.int32)
    up = torch.where(h.to(torch.float64) < mag, bits + 1, bits).to(torch.int16).view(torch.bfloat16)
    return up.to(torch.float64)


def half_spacing_bf16(mag: torch.Tensor) -> torch.Tensor:
    """Half the bfloat16 spacing at the larger bf16 neighbour of ``mag`` (>= 0): the largest error of a round-to-nearest store of any
    value of at most that magnitude; 0 at 0."""
    up = bf16_up(mag)
    _, e = torch.frexp(up)  # up = m 2^e, m in [0.5, 1): the binade [2^(e-1), 2^e) has spacing 2^(e-8)
    e = torch.clamp(e.to(torch.float64) - 1.0, min=-126.0)
    return torch.where(up > 0, torch.exp2(e - 8.0), torch.zeros_like(up))


def round_bf16(x: torch.Tensor) -> torch.Tensor:
    """Round to nearest even, as ``v_cvt_pk_bf16_f32`` does (x: float32 — one rounding — or float64 values that are floats)."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def trunc_bf16(x: torch.Tensor) -> torch.Tensor:
    """Mutation (c): a bfloat16 store that truncates toward zero (the upper 16 bits of the float)."""
    h = x.to(torch.float32).to(torch.bfloat16)
    bits = h.view(torch.int16).to(torch.int32)
    over = h.to(torch.float64).abs() > x.to(torch.float64).abs()
    return torch.where(over, bits - 1, bits).to(torch.int16).view(torch.bfloat16).to(x.dtype)  # sign-magnitude: one ulp toward 0


def pair_bf16(t: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The matrix-core kernels' tap pair in bfloat16: (th, tl) as float64."""
    t32 = torch.from_numpy(np.asarray(t, dtype=np.float64).astype(np.float32))
    th = t32.to(torch.bfloat16)
    tl = (t32 - th.to(torch.float32)).to(torch.bfloat16)
    return th.to(torch.float64).numpy(), tl.to(torch.float64).numpy()


def pair_bf16_err(t: np.ndarray) -> np.ndarray:
    """|t - (th + tl)| <= this: 2^-24 |t| for the cast to float, 2^-16 |t32| for the pair (module docstring)."""
    t = np.asarray(t, dtype=np.float64)
    assert np.all((t == 0) | (np.abs(t) > 2.0 ** -100))  # (no bf16 subnormal within reach)
    return R.U32 * np.abs(t) + 2.0 ** -16 * np.abs(t) * (1.0 + R.U32)


# storage 'bf16' / tap form 'pairbf16' are this module's; _probe_ref's own functions know 'f16' / 'pair16' only
VECBF16 = R.Arith("bf16 storage, f32 arithmetic", R.U32, "acc", lambda L: L, None, "bf16", torch.float32)
# two v_mfma_f32_32x32x16_bf16 per K-step (x . t_hi, then x . t_lo): 2 L non-structural products, each addition taken to err like a
# rounded f32 addition; the image between the passes is rounded to bf16 once, the output once
MFMABF16 = R.Arith("bf16 matrix cores", R.U32, "pairbf16", lambda L: 2 * L, "bf16", "bf16", torch.float32)


def hat(op: R.AxisOp, arith: R.Arith, flush_lo: bool = False, drop: Optional[Tuple[int, int]] = None):
    """``AxisOp.hat`` for this module's arithmetics: (addends of the operator as the kernel holds it, bound on |hat - M|, bound on |hat|)."""
    if arith.taps != "pairbf16":
        assert not flush_lo
        return op.hat(arith, drop=drop)
    key = (arith.name, flush_lo, drop)
    if key not in op._hat:
        lo, hi = op.lo.copy(), op.hi.copy()
        if drop is not None:
            lo[drop[0]] = 0.0
            hi[drop[1]] = 0.0
        (lh, ll), (hh, hl) = pair_bf16(lo), pair_bf16(hi)
        if flush_lo:
            ll, hl = 0 * ll, 0 * hl
        parts = [op.build(lh, hh), op.build(ll, hl)]
        err = op.build(pair_bf16_err(op.lo), pair_bf16_err(op.hi))
        mag = op.build(np.abs(lh) + np.abs(ll), np.abs(hh) + np.abs(hl))
        op._hat[key] = (parts, err, mag)
    return op._hat[key]


def axis_pass(st: R.State, op: R.AxisOp, arith: R.Arith, axis: int, store: Optional[str]) -> R.State:
    """``_probe_ref.axis_pass`` with a bf16 store: |M| |c - w| + |hat(M) - M| |c| + gamma_adds |hat(M)| |c|, then half the bf16 spacing
    at the bound of the result's magnitude."""
    dev = st.want.device
    _, e_np, mag_np = hat(op, arith)
    M = torch.from_numpy(op.M).to(dev)
    E = torch.from_numpy(e_np).to(dev)
    Mbar = torch.from_numpy(mag_np).to(dev)
    want = R._apply(M, st.want, axis)
    err = R._apply(M.abs(), st.err, axis) + R._apply(E + R.gamma(arith.adds(op.L), arith.u) * Mbar, st.mag, axis)
    if store == "bf16":
        err = err + half_spacing_bf16(want.abs() + err)
    else:
        assert store is None
    return R.State(want, err)


def level_2d(x: R.State, op_r: R.AxisOp, op_c: R.AxisOp, arith: R.Arith, rows_first: bool = False) -> R.State:
    first, second = ((op_r, -2), (op_c, -1)) if rows_first else ((op_c, -1), (op_r, -2))
    return axis_pass(axis_pass(x, first[0], arith, first[1], arith.inter), second[0], arith, second[1], arith.store)


def emulate_pass(x: torch.Tensor, op: R.AxisOp, arith: R.Arith, axis: int, store: Optional[str], *, drop=None, flush_lo=False,
                 trunc=False) -> torch.Tensor:
    """The pass in the kernel's number formats: products and sums in float32, the store rounded (mutation c: truncated) with
    ``.to(torch.bfloat16)`` where the kernel stores bf16."""
    parts, _, _ = hat(op, arith, flush_lo=flush_lo, drop=drop)
    xa = x.to(arith.torch_acc)
    y = None
    for p in parts:
        t = R._apply(torch.from_numpy(p).to(arith.torch_acc).to(x.device), xa, axis)
        y = t if y is None else y + t
    if store == "bf16":
        y = trunc_bf16(y) if trunc else round_bf16(y)
    return y.to(torch.float64)


def emulate_2d(x: torch.Tensor, op_r: R.AxisOp, op_c: R.AxisOp, arith: R.Arith, rows_first: bool = False, **mut) -> torch.Tensor:
    first, second = ((op_r, -2), (op_c, -1)) if rows_first else ((op_c, -1), (op_r, -2))
    mid = emulate_pass(x, first[0], arith, first[1], arith.inter, **mut)
    return emulate_pass(mid, second[0], arith, second[1], arith.store, **mut)


# --------------------------------------------------------------------------------------------------- the case table
@dataclass(frozen=True)
class Bf16Case(R.Case):
    """A row of ``_probe_ref.Case`` in bf16 storage (``dtype`` = 'bf16': ``_probe_ref.amplitude`` then feeds impulses of 1.0 — a power
    of two; bf16 has no range to guard)."""

    @property
    def arith(self) -> R.Arith:
        return MFMABF16 if self.family.startswith("mfma") else VECBF16

    @property
    def torch_dtype(self) -> torch.dtype:
        return torch.bfloat16


def cases() -> List[Bf16Case]:
    """The float16 rows of ``_probe_ref.cases()`` — same families, kernel ids, modes, seam planes and lengths — for the banks that
    take every code path: the shortest and the longest of the matrix-core envelope (db9: P = 16 is a multiple of 8, sym16: 32 taps),
    a short and the longest bank of the LDS tiles, and the 32-tap bank of the streaming inner-axis kernels."""
    t: List[Bf16Case] = []
    for w in ("db9", "sym16"):
        t.append(Bf16Case("mfma_fwd", (11,), 0, 2, "bf16", w, R.ALL_MODES, R._MFMA_SEAM))
        t.append(Bf16Case("mfma_inv", (23,), 1, 2, "bf16", w, R.ALL_MODES[:1], R._MFMA_SEAM))
    for w in ("db4", "sym16"):
        t.append(Bf16Case("tile_fwd", (7,), 0, 2, "bf16", w, R.ALL_MODES, R._TILE_SEAM))
        t.append(Bf16Case("tile_inv", (8,), 1, 2, "bf16", w, R.ALL_MODES[:1], R._TILE_SEAM))
    t.append(Bf16Case("axis_fwd", (3,), 0, 1, "bf16", "sym16", R.ALL_MODES, lengths=(301,)))
    t.append(Bf16Case("axis_inv", (4,), 1, 1, "bf16", "sym16", R.ALL_MODES[:1], lengths=(301,)))
    return t


def bound(job: R.Job, x: torch.Tensor) -> R.State:
    """``Job.bound`` in the case's bf16 arithmetic."""
    a = job.case.arith
    if job.op_r is None:
        return axis_pass(R.State(x), job.op_c, a, -1, a.store)
    return level_2d(R.State(x), job.op_r, job.op_c, a, rows_first=job.case.family == "tile_inv")


def emulate(job: R.Job, x: torch.Tensor, ops: Optional[Tuple[Optional[R.AxisOp], R.AxisOp]] = None, **mut) -> torch.Tensor:
    a = job.case.arith
    op_r, op_c = ops if ops is not None else (job.op_r, job.op_c)
    if op_r is None:
        return emulate_pass(x, op_c, a, -1, a.store, **mut)
    return emulate_2d(x, op_r, op_c, a, rows_first=job.case.family == "tile_inv", **mut)
