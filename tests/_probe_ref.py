"""Impulse probes, float64 operators, element-wise worst-case bounds and arithmetic emulators (host only).

The norm-wise metric of ``tests/_golden.py`` cannot see the outer taps of the 18..32-tap banks (a dropped end tap of db14 moves
it by 1.8e-7).  A transform is a linear map, so these helpers feed isolated impulses and compare EVERY output element with the
float64 operator against a bound that is derived from the kernel's arithmetic, term by term, with no empirical factor.

Reference.  The dense 1-D operators come from ``oracle.fwt_oracle`` alone: ``wavedec(eye(n), level=1)`` for the analysis
operator ``W`` ((2M) x n, rows of lo then hi) and ``waverec`` of unit coefficient vectors for the synthesis operator ``S``
(n_out x 2M, columns of lo then hi).  Applied to the identity the oracle's sums add exact zeros, so every entry is an exact sum
of taps.  A second, structural description of the same operator (``AxisOp.P``: which tap m reads which sample i for which
output k) is built from the oracle's own index map and must reproduce ``W`` exactly; it exists because a kernel rounds TAPS, not
operator entries (a mirrored border sample meets two taps), and because the mutations act on single taps.

Everything is torch float64 and device agnostic: the CPU tests run it on the host, the GPU tests on the device (plain matmul,
nothing of the library under test).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import fwt_oracle as O

U32 = 2.0 ** -24  # unit roundoff of float32
U64 = 2.0 ** -53  # unit roundoff of float64
ALL_MODES = ("reflect", "zero", "constant", "periodic", "symmetric")
OTHER_MIRROR = {"reflect": "symmetric", "symmetric": "reflect"}


def gamma(k: int, u: float) -> float:
    """Higham's gamma_k = k u / (1 - k u): the relative bound of k successive roundings (1 + d_1) ... (1 + d_k) - 1."""
    return k * u / (1.0 - k * u)


# --------------------------------------------------------------------------------------------------- f16 helpers
def f16_up(mag: torch.Tensor) -> torch.Tensor:
    """The magnitudes rounded UP to float16 (the larger f16 neighbour), as float64."""
    h = mag.to(torch.float16)
    bits = h.view(torch.int16).to(torch.int32)
    up = torch.where(h.to(torch.float64) < mag, bits + 1, bits).to(torch.int16).view(torch.float16)
    return up.to(torch.float64)


def half_spacing16(mag: torch.Tensor) -> torch.Tensor:
    """Half the float16 spacing at the larger f16 neighbour of ``mag`` (>= 0): the largest error of a round-to-nearest store of
    any value of at most that magnitude.  Equals ``np.spacing(np.float16(up)) / 2`` (subnormals, spacing 2^-24, included), and 0 at 0."""
    up = f16_up(mag)
    _, e = torch.frexp(up)  # up = m 2^e, m in [0.5, 1): the binade [2^(e-1), 2^e) has spacing 2^(e-11)
    e = torch.clamp(e.to(torch.float64) - 1.0, min=-14.0)
    return torch.where(up > 0, torch.exp2(e - 11.0), torch.zeros_like(up))  # (a zero is stored exactly)


def round16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float16).to(x.dtype)


def trunc16(x: torch.Tensor) -> torch.Tensor:
    """Mutation (c): a float16 store that truncates toward zero."""
    h = x.to(torch.float16)
    bits = h.view(torch.int16).to(torch.int32)
    over = h.to(torch.float64).abs() > x.to(torch.float64).abs()
    return torch.where(over, bits - 1, bits).to(torch.int16).view(torch.float16).to(x.dtype)  # sign-magnitude: one ulp toward 0


# --------------------------------------------------------------------------------------------------- taps in a kernel's arithmetic
def pair16(t: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The matrix-core kernels' tap pair (mifwt_dwt2_fwd_mfma.hip ``th = (_Float16)t; tl = (_Float16)(t - (float)th)`` with
    ``t`` the double tap cast to float): returns (th, tl) as float64."""
    t32 = np.asarray(t, dtype=np.float64).astype(np.float32)
    th = t32.astype(np.float16)
    tl = (t32 - th.astype(np.float32)).astype(np.float16)
    return th.astype(np.float64), tl.astype(np.float64)


def pair16_err(t: np.ndarray) -> np.ndarray:
    """|t - (th + tl)| <= this, for |t| < 1.  Derivation: t32 = fl32(t) costs 2^-24 |t|.  th = RN16(t32) leaves r = t32 - th with
    |r| <= 2^(e-11) for |t32| in [2^e, 2^(e+1)); r is a multiple of 2^(e-23), so 13 bits: exact in float.  tl = RN16(r): r is exact
    when |r| = 2^(e-11); otherwise it lies in a binade <= e - 12 and errs by at most 2^(e-23) while that binade is normal
    (e - 12 >= -14, i.e. |t32| >= 1/4), and by 2^-25 (half the f16 subnormal spacing) below.  So: 2^-24 for |t32| >= 1/2, else
    2^-25 — an ABSOLUTE accuracy: the pair is not f32-accurate for small taps (db14's end tap 1.8e-7: up to 17 % off)."""
    t = np.asarray(t, dtype=np.float64)
    assert np.all(np.abs(t) < 1.0)
    t32 = np.abs(t.astype(np.float32).astype(np.float64))
    return np.where(t == 0, 0.0, U32 * np.abs(t) + np.where(t32 >= 0.5, 2.0 ** -24, 2.0 ** -25))


@dataclass(frozen=True)
class Arith:
    """One kernel arithmetic.  ``u``: unit roundoff of the accumulation type.  ``taps``: 'exact' (double taps in a double
    kernel), 'acc' (double taps cast to the accumulation type: |dt| <= u |t|) or 'pair16' (f16 pairs, ``pair16_err``).
    ``adds(L)``: roundings of one output's sum in one axis pass.  ``inter``: storage of the image between the two passes of a
    fused 2-D level, ``store``: storage of a level's output ('f16', or None = the accumulation type, no further rounding)."""

    name: str
    u: float
    taps: str
    adds: Callable[[int], int]
    inter: Optional[str]
    store: Optional[str]
    torch_acc: torch.dtype


# Vector kernels: per output one multiply and L - 1 FMAs (or L FMAs onto 0), each rounded once: L roundings, whatever the order
# (two accumulators that are added at the end are no deeper); the tap's own rounding to the accumulation type is in ``taps``.
VEC64 = Arith("f64", U64, "exact", lambda L: L, None, None, torch.float64)
VEC32 = Arith("f32", U32, "acc", lambda L: L, None, None, torch.float32)
VEC16 = Arith("f16 storage, f32 arithmetic", U32, "acc", lambda L: L, None, "f16", torch.float32)
# Matrix-core kernels (ids 11 / 23): per K-step two v_mfma_f32_32x32x16_f16 (x . t_hi, then x . t_lo) onto an f32 accumulator.
# f16 x f16 products are exact in f32; of the 2 x 64 products of an output only 2 L are not structural zeros (adding 0 is exact),
# and every addition is taken to err like a rounded f32 addition at worst: 2 L roundings.  The image between the passes is
# rounded to f16 once, the output once.
MFMA16 = Arith("f16 matrix cores", U32, "pair16", lambda L: 2 * L, "f16", "f16", torch.float32)


# --------------------------------------------------------------------------------------------------- operators
class AxisOp:
    """A one-level, one-axis operator ``y = M x`` (analysis: M = W, (2m) x n; synthesis: M = S, n_out x (2m)).

    ``M``: the float64 reference from the oracle.  ``P``: tap structure of one band block, the list of incidences (shape of the block,
    tap index m, row, column) = "tap m reads that column for that row" (a dense P[m, row, column] of a 4101-column operator would
    hold 1.3 GB); ``M = [sum lo[m] P[m]; sum hi[m] P[m]]`` (analysis, bands stacked as rows) or ``[... | ...]`` (synthesis, columns)."""

    def __init__(self, kind: str, lo: np.ndarray, hi: np.ndarray, P: np.ndarray, M: np.ndarray):
        self.kind, self.lo, self.hi, self.P, self.M = kind, lo, hi, P, M
        self.L = len(lo)
        self._hat: dict = {}

    def build(self, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
        shape, taps, rows, cols = self.P
        a, b = np.zeros(shape), np.zeros(shape)
        np.add.at(a, (rows, cols), np.asarray(lo)[taps])
        np.add.at(b, (rows, cols), np.asarray(hi)[taps])
        return np.vstack([a, b]) if self.kind == "analysis" else np.hstack([a, b])

    def hat(self, arith: Arith, flush_lo: bool = False, drop: Optional[Tuple[int, int]] = None):
        """(operator with the taps as the kernel holds them [list of addends: one matrix, or (hi, lo) of the pair],
        entry-wise bound E on |hat - M|, entry-wise bound on |hat|).  ``drop`` = (index in lo, index in hi) of taps set to 0
        (mutation a); ``flush_lo``: the low halves of the pairs flushed to zero (mutation d)."""
        key = (arith.name, flush_lo, drop)
        if key not in self._hat:  # (once per arithmetic and mutation)
            self._hat[key] = self._hat_uncached(arith, flush_lo, drop)
        return self._hat[key]

    def _hat_uncached(self, arith: Arith, flush_lo: bool, drop: Optional[Tuple[int, int]]):
        lo, hi = self.lo.copy(), self.hi.copy()
        if drop is not None:
            lo[drop[0]] = 0.0
            hi[drop[1]] = 0.0
        if arith.taps == "exact":
            parts, err = [self.build(lo, hi)], self.build(0 * lo, 0 * hi)
            mag = self.build(np.abs(lo), np.abs(hi))
        elif arith.taps == "acc":
            assert arith.torch_acc == torch.float32
            l32, h32 = lo.astype(np.float32).astype(np.float64), hi.astype(np.float32).astype(np.float64)
            parts, err = [self.build(l32, h32)], self.build(U32 * np.abs(self.lo), U32 * np.abs(self.hi))
            mag = self.build(np.abs(l32), np.abs(h32))
        else:
            (lh, ll), (hh, hl) = pair16(lo), pair16(hi)
            if flush_lo:
                ll, hl = 0 * ll, 0 * hl
            parts, err = [self.build(lh, hh), self.build(ll, hl)], self.build(pair16_err(self.lo), pair16_err(self.hi))
            mag = self.build(np.abs(lh) + np.abs(ll), np.abs(hh) + np.abs(hl))
        return parts, err, mag


def _analysis_P(L: int, n: int, mode: str, last_tap_mode: Optional[str] = None):
    """The incidences (m, k, i) of c[k] = sum_j flip(h)[j] x_ext[2k + j - padl] (oracle.dwt_axis); ``last_tap_mode``: mutation (b), the last
    sample of every window (j = L - 1) is taken by the other mirror rule where it lies outside the signal."""
    padl, padr = O.get_pad(n, L)
    m_out = (n + padl + padr - L) // 2 + 1
    k = np.arange(m_out)
    taps, rows, cols = [], [], []
    for j in range(L):
        ext = 2 * k + j - padl
        src = O.ext_index(ext, n, last_tap_mode if (last_tap_mode and j == L - 1) else mode)
        ok = src >= 0
        taps.append(np.full(int(ok.sum()), L - 1 - j))
        rows.append(k[ok])
        cols.append(src[ok])
    return (m_out, n), np.concatenate(taps), np.concatenate(rows), np.concatenate(cols)


def analysis_axis(wavelet: str, n: int, mode: str, last_tap_mode: Optional[str] = None) -> AxisOp:
    lo, hi = O.filter_bank(wavelet)[:2]
    a, d = O.wavedec(np.eye(n), wavelet, mode=mode, level=1)
    M = np.vstack([a.T, d.T])
    op = AxisOp("analysis", lo, hi, _analysis_P(len(lo), n, mode, last_tap_mode), M)
    if last_tap_mode is None:
        # (an entry at a border is a sum of up to L taps — constant mode — which the oracle adds in another order)
        assert np.max(np.abs(op.build(lo, hi) - M)) <= 2 * len(lo) * U64, "tap structure != oracle"
    return op


def synthesis_axis(wavelet: str, m: int, trim: int = 0) -> AxisOp:
    """S (n_out x 2m), n_out = 2m - L + 2 - trim: ``waverec`` of the unit coefficient vectors; the trim drops the last sample,
    as the oracle does for a level whose finer detail band is one shorter."""
    lo, hi = O.filter_bank(wavelet)[2:]
    L = len(lo)
    n_out = 2 * m - L + 2 - trim
    eye, zero = np.eye(m), np.zeros((m, m))
    M = np.hstack([O.waverec([eye, zero], wavelet).T, O.waverec([zero, eye], wavelet).T])[:n_out]
    # y[i] = sum_k g[i + L - 2 - 2k] c[k]   (oracle.idwt_axis: u[2k + t] += g[t] c[k], crop L - 2)
    i, kk = np.meshgrid(np.arange(n_out), np.arange(m), indexing="ij")
    t = i + L - 2 - 2 * kk
    ok = (t >= 0) & (t < L)
    P = ((n_out, m), t[ok], i[ok], kk[ok])
    op = AxisOp("synthesis", lo, hi, P, M)
    assert np.array_equal(op.build(lo, hi), M), "tap structure != oracle"
    return op


def smallest_taps(op: AxisOp) -> Tuple[int, int]:
    return int(np.argmin(np.abs(op.lo))), int(np.argmin(np.abs(op.hi)))


# --------------------------------------------------------------------------------------------------- probes
def impulses_1d(n: int, amp: float, device="cpu") -> torch.Tensor:
    """A . I: one impulse per row of the batch — the complete operator."""
    return amp * torch.eye(n, dtype=torch.float64, device=device)


def impulses_2d(h: int, w: int, amp: float, device="cpu") -> torch.Tensor:
    """One impulse per image, at every position: (h w, h, w); image i * w + j has its impulse at (i, j)."""
    x = torch.zeros(h * w, h * w, dtype=torch.float64, device=device)
    x.fill_diagonal_(amp)
    return x.view(h * w, h, w)


def lattice_shifts(pitch: int) -> List[Tuple[int, int]]:
    s = [(k, 0) for k in range(pitch)] + [(0, k) for k in range(1, pitch)] + [(k, k) for k in range(1, pitch)]
    return s


def lattice_2d(h: int, w: int, pitch: int, amp: float, device="cpu") -> torch.Tensor:
    """A lattice of impulses of the given pitch in both directions, one image per shift (k, 0), (0, k), (k, k), k < pitch.  No
    window of pitch - 2 = L taps ever holds two impulses of a row or column."""
    shifts = lattice_shifts(pitch)
    x = torch.zeros(len(shifts), h, w, dtype=torch.float64, device=device)
    for b, (dr, dc) in enumerate(shifts):
        x[b, dr::pitch, dc::pitch] = amp
    return x


def f16_amplitude(max_unit_response: float) -> float:
    """The largest power of two A for which the reference output of A-impulses stays below 2^15 in magnitude."""
    a = 2.0 ** np.floor(np.log2(2.0 ** 15 / max_unit_response))
    while a * max_unit_response >= 2.0 ** 15:
        a /= 2
    return float(min(a, 2.0 ** 15))


# --------------------------------------------------------------------------------------------------- bound recurrence
class State:
    """want: the float64 reference; err: bound on |computed - want|; both (batch, rows, cols) or (batch, n)."""

    def __init__(self, want: torch.Tensor, err: Optional[torch.Tensor] = None):
        self.want = want
        self.err = torch.zeros_like(want) if err is None else err

    @property
    def mag(self) -> torch.Tensor:  # bound on |computed|
        return self.want.abs() + self.err


def _apply(mat: torch.Tensor, x: torch.Tensor, axis: int) -> torch.Tensor:
    """mat applied along ``axis`` (-1: x @ mat^T, -2: mat @ x)."""
    if axis == -1:
        return x @ mat.T
    if x.dim() == 2:
        return mat @ x
    return (x.transpose(-1, -2).contiguous() @ mat.T).transpose(-1, -2)  # (one GEMM over the whole batch, not one per image)


def axis_pass(st: State, op: AxisOp, arith: Arith, axis: int, store: Optional[str]) -> State:
    """One axis pass of a kernel: computed' = store(fl(hat(M) computed)).

      |hat(M) c - M w| <= |M| |c - w| + |hat(M) - M| |c|                       (c: computed input, w: its reference)
      the sum's roundings: gamma_adds(L) . |hat(M)| |c|                          (``Arith.adds``)
      a narrower store: half the f16 spacing at the bound of the result's magnitude.
    """
    dev = st.want.device
    _, e_np, mag_np = op.hat(arith)
    M = torch.from_numpy(op.M).to(dev)
    E = torch.from_numpy(e_np).to(dev)
    Mbar = torch.from_numpy(mag_np).to(dev)
    mag_in = st.mag
    want = _apply(M, st.want, axis)
    err = _apply(M.abs(), st.err, axis) + _apply(E + gamma(arith.adds(op.L), arith.u) * Mbar, mag_in, axis)
    if store == "f16":
        err = err + half_spacing16(want.abs() + err)
    else:
        assert store is None
    return State(want, err)


def level_2d(x: State, op_r: AxisOp, op_c: AxisOp, arith: Arith, rows_first: bool = False) -> State:
    """A fused 2-D level ``M_r X M_c^T`` in the kernel's own pass order.  Along the rows of memory (axis -1) first: the analysis
    kernels (LDS tiles id 7 and small planes id 20: horizontal pass in LDS, then the vertical one) and BOTH matrix-core kernels (ids
    11 / 23: along the rows, the transposed image rounded to f16, then along the columns).  ``rows_first`` (axis -2 first): the vector
    synthesis kernels (LDS tiles id 8, small planes id 21: vertical synthesis in LDS, then the horizontal one)."""
    first, second = ((op_r, -2), (op_c, -1)) if rows_first else ((op_c, -1), (op_r, -2))
    mid = axis_pass(x, first[0], arith, first[1], arith.inter)
    return axis_pass(mid, second[0], arith, second[1], arith.store)


# --------------------------------------------------------------------------------------------------- emulators
def emulate_pass(x: torch.Tensor, op: AxisOp, arith: Arith, axis: int, store: Optional[str], *, drop=None, flush_lo=False,
                 trunc=False) -> torch.Tensor:
    """The pass in the kernel's number formats: taps as the kernel holds them, products and sums in the accumulation type, the
    store rounded (mutation c: truncated) to f16 where the kernel stores f16.  x: float64 holding representable values."""
    parts, _, _ = op.hat(arith, flush_lo=flush_lo, drop=drop)
    acc = arith.torch_acc
    xa = x.to(acc)
    y = None
    for p in parts:  # (the pair: x . t_hi, then x . t_lo, added in the accumulation type)
        t = _apply(torch.from_numpy(p).to(acc).to(x.device), xa, axis)
        y = t if y is None else y + t
    if store == "f16":
        y = trunc16(y) if trunc else round16(y)
    return y.to(torch.float64)


def emulate_2d(x: torch.Tensor, op_r: AxisOp, op_c: AxisOp, arith: Arith, rows_first: bool = False, **mut) -> torch.Tensor:
    first, second = ((op_r, -2), (op_c, -1)) if rows_first else ((op_c, -1), (op_r, -2))
    mid = emulate_pass(x, first[0], arith, first[1], arith.inter, **mut)
    return emulate_pass(mid, second[0], arith, second[1], arith.store, **mut)


# --------------------------------------------------------------------------------------------------- judging
def worst(got: torch.Tensor, st: State):
    """(largest |got - want| / bound, its flat index, number of elements past their bound).  An element whose bound is 0 must be
    exact (ratio inf otherwise, 0 when it is)."""
    diff = (got - st.want).abs()
    ratio = torch.where(st.err > 0, diff / st.err, torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
    flat = ratio.reshape(-1)
    i = int(torch.argmax(flat))
    return float(flat[i]), i, int((flat > 1.0).sum())


def describe(idx: int, shape: Sequence[int], op_r: Optional[AxisOp], op_c: AxisOp) -> str:
    """Image, position and the operator rows an element corresponds to (failure messages)."""
    pos = np.unravel_index(idx, tuple(shape))
    if len(pos) == 2:
        b, k = pos
        return "probe %d (impulse at sample %d), output %d = operator entry (%d, %d) = %.3e" % (b, b, k, k, b, op_c.M[k, b] if op_c.M.shape[1] > b else float("nan"))
    b, p, k = pos
    return "image %d, output (%d, %d): operator rows %d (axis -2) and %d (axis -1)" % (b, p, k, p, k)


# --------------------------------------------------------------------------------------------------- the case table
@dataclass(frozen=True)
class Case:
    """One row of the table the CPU and the GPU tests share: a kernel family with one wavelet and one storage type."""

    family: str       # name of the family (test ids)
    kids: Tuple[int, ...]  # kernel ids that may serve it (the GPU test asserts that one of them served every level)
    direction: int    # 0 analysis, 1 synthesis
    ndim: int
    dtype: str        # 'f16' | 'f32' | 'f64'
    wavelet: str
    modes: Tuple[str, ...]
    seam: Tuple[int, int] = (70, 300)  # 2-D: the even-pitch seam plane; the odd-pitch one is one less / one more
    lengths: Tuple[int, ...] = ()      # 1-D: signal lengths besides 2 L + 1
    levels: int = 1

    @property
    def id(self) -> str:
        return "%s-%s-%s" % (self.family, self.wavelet, self.dtype)

    @property
    def flen(self) -> int:
        return len(O.filter_bank(self.wavelet)[0])

    @property
    def arith(self) -> Arith:
        if self.family.startswith("mfma"):
            return MFMA16
        return {"f16": VEC16, "f32": VEC32, "f64": VEC64}[self.dtype]

    @property
    def torch_dtype(self) -> torch.dtype:
        return {"f16": torch.float16, "f32": torch.float32, "f64": torch.float64}[self.dtype]

    def planes(self, mode: str) -> List[Tuple[int, int, str]]:
        """(rows, columns, probe kind) of a 2-D case.  'single': the smallest plane the kernels accept, one impulse per image at
        every position (odd pitch).  'lattice': seam planes that span more than two tiles / panels each way, ragged, lattice of
        pitch L + 2; one with an even and one with an odd pitch of the rows in memory.  Periodic: the extents are multiples of the
        pitch (even), so that the lattice wraps onto itself — otherwise the wrapped windows hold two impulses or none."""
        L = self.flen
        p = L + 2
        out = [(2 * L, 2 * L + 1, "single")]
        if mode == "periodic":
            out.append((-(-self.seam[0] // p) * p, -(-self.seam[1] // p) * p, "lattice"))
        else:
            out += [(self.seam[0], self.seam[1], "lattice"), (self.seam[0] - 1, self.seam[1] + 1, "lattice")]
        return out


_LONG5 = ("db9", "db10", "db12", "db14", "sym16")
# seam planes.  Matrix-core kernels: tiles of 16 x 64 coefficients (analysis) / 32 x 128 samples (synthesis): 70 x 300 gives 3 - 4
# stacked tiles and 3 column panels, the last ones ragged.  LDS-tile kernels: tiles of TR x 64 coefficients, TR up to 24: 100 x 300
# gives three tiles of 24 rows for every bank of the table, ragged.
_MFMA_SEAM, _TILE_SEAM = (70, 300), (100, 300)


def cases() -> List[Case]:
    t: List[Case] = []
    for w in _LONG5:
        t.append(Case("mfma_fwd", (11,), 0, 2, "f16", w, ALL_MODES, _MFMA_SEAM))
        t.append(Case("mfma_inv", (23,), 1, 2, "f16", w, ALL_MODES[:1], _MFMA_SEAM))
    for w in ("db4", "db10", "sym16"):
        t.append(Case("tile_fwd", (7,), 0, 2, "f16", w, ALL_MODES, _TILE_SEAM))
        t.append(Case("tile_inv", (8,), 1, 2, "f16", w, ALL_MODES[:1], _TILE_SEAM))
    for w in ("db9", "db10", "db12", "sym16"):
        t.append(Case("tile_fwd", (7,), 0, 2, "f32", w, ALL_MODES, _TILE_SEAM))
        t.append(Case("tile_inv", (8,), 1, 2, "f32", w, ALL_MODES[:1], _TILE_SEAM))
    for w in ("db14", "sym16"):  # (db14, 28 taps, is not instantiated in the streaming kernels: the generic kernel serves it)
        for dt in ("f16", "f32", "f64"):
            t.append(Case("axis_fwd", (3,) if w == "sym16" else (0,), 0, 1, dt, w, ALL_MODES, lengths=(301,)))
            t.append(Case("axis_inv", (4,) if w == "sym16" else (0,), 1, 1, dt, w, ALL_MODES[:1], lengths=(301,)))
    for dt in ("f64", "f32"):
        t.append(Case("generic_fwd", (0,), 0, 1, dt, "coif17", ("symmetric", "zero"), lengths=(205,)))
        t.append(Case("generic_inv", (0,), 1, 1, dt, "coif17", ("symmetric",), lengths=(205,)))
    return t


def case_ids(cs: Sequence[Case]) -> List[str]:
    return [c.id for c in cs]


# --------------------------------------------------------------------------------------------------- a case's operators and probes
_OPS: dict = {}


def fwd_op(wavelet: str, n: int, mode: str) -> AxisOp:
    key = ("fwd", wavelet, n, mode)
    if key not in _OPS:
        _OPS[key] = analysis_axis(wavelet, n, mode)
    return _OPS[key]


def inv_op(wavelet: str, m: int, trim: int = 0) -> AxisOp:
    key = ("inv", wavelet, m, trim)
    if key not in _OPS:
        _OPS[key] = synthesis_axis(wavelet, m, trim)
    return _OPS[key]


def coef_extent(n: int, L: int) -> int:
    return (n + L - 1) // 2


def amplitude(case: Case, *ops: AxisOp) -> float:
    """1 for f32 / f64; f16: the largest power of two that keeps the reference output below 2^15 (isolated impulses: the largest
    response is the product of the operators' largest entries)."""
    if case.dtype != "f16":
        return 1.0
    return f16_amplitude(float(np.prod([np.abs(op.M).max() for op in ops])))


def probes_2d(kind: str, h: int, w: int, pitch: int, amp: float, device="cpu") -> torch.Tensor:
    return impulses_2d(h, w, amp, device) if kind == "single" else lattice_2d(h, w, pitch, amp, device)


def band_probes_2d(kind: str, mh: int, mw: int, pitch: int, amp: float, device="cpu") -> torch.Tensor:
    """Synthesis: the stacked coefficient plane Z = [[aa, ad], [da, dd]] (2 mh x 2 mw).  'single': an impulse at every position of
    every band = at every position of Z.  'lattice': the lattice images in each band in turn, the other bands zero."""
    if kind == "single":
        return impulses_2d(2 * mh, 2 * mw, amp, device)
    lat = lattice_2d(mh, mw, pitch, amp, device)
    z = torch.zeros(4, lat.shape[0], 2 * mh, 2 * mw, dtype=torch.float64, device=device)
    for b in range(4):
        z[b, :, (b >> 1) * mh:(b >> 1) * mh + mh, (b & 1) * mw:(b & 1) * mw + mw] = lat
    return z.reshape(-1, 2 * mh, 2 * mw)


def chunks(n: int, size: int = 512):
    return [slice(i, min(i + size, n)) for i in range(0, n, size)]


class Job:
    """One probe batch of a case: the probes ``x`` (float64; 1-D: (B, n), 2-D: (B, rows, cols); synthesis: the stacked coefficient
    vector [a | d] / plane [[aa, ad], [da, dd]]), the operator(s), and what the bound, the emulator and the failure message need."""

    def __init__(self, case: Case, mode: str, label: str, x: torch.Tensor, op_c: AxisOp, op_r: Optional[AxisOp] = None, extra=None):
        self.case, self.mode, self.label, self.x, self.op_c, self.op_r, self.extra = case, mode, label, x, op_c, op_r, extra

    def bound(self, x: torch.Tensor) -> State:
        a = self.case.arith
        if self.op_r is None:
            return axis_pass(State(x), self.op_c, a, -1, a.store)
        return level_2d(State(x), self.op_r, self.op_c, a, rows_first=self.case.family == "tile_inv")

    def emulate(self, x: torch.Tensor, ops: Optional[Tuple[Optional[AxisOp], AxisOp]] = None, **mut) -> torch.Tensor:
        a = self.case.arith
        op_r, op_c = ops if ops is not None else (self.op_r, self.op_c)
        if op_r is None:
            return emulate_pass(x, op_c, a, -1, a.store, **mut)
        return emulate_2d(x, op_r, op_c, a, rows_first=self.case.family == "tile_inv", **mut)

    def where(self, idx: int, shape) -> str:
        """Image, position, and the operator entries the element is made of: the impulses of that image that the two operator rows
        reach (1-D: the entry itself)."""
        if self.op_r is None:
            return "%s %s %s: %s" % (self.case.id, self.mode, self.label, describe(idx, shape, self.op_r, self.op_c))
        b, p, k = (int(v) for v in np.unravel_index(idx, tuple(shape)))
        img = self.x[b] != 0
        rows = [int(i) for i in torch.nonzero(img.any(dim=1)).reshape(-1).tolist() if self.op_r.M[p, i] != 0]
        cols = [int(j) for j in torch.nonzero(img.any(dim=0)).reshape(-1).tolist() if self.op_c.M[k, j] != 0]
        ents = ["axis -2 entry (%d, %d) = %.3e" % (p, i, self.op_r.M[p, i]) for i in rows] + \
               ["axis -1 entry (%d, %d) = %.3e" % (k, j, self.op_c.M[k, j]) for j in cols]
        return "%s %s %s: image %d, output (%d, %d); operator entries: %s" % (
            self.case.id, self.mode, self.label, b, p, k, "; ".join(ents) if ents else "none (the element must be 0)")


def thin_single(x: torch.Tensor) -> torch.Tensor:
    """Of the one-impulse-per-image batch of an h x w plane, the images whose impulse lies in the middle row, the middle column or on
    the diagonal: every row and every column of the plane still carries an impulse (what the coverage of the 1-D operators needs) at
    a twentieth of the images.  The CPU tests use it (and the diagonal shifts of the lattices); the GPU tests run every position."""
    b, h, w = x.shape
    i, j = torch.arange(b) // w, torch.arange(b) % w
    return x[(i == h // 2) | (j == w // 2) | (j == (i * w) // h)]


def jobs(case: Case, mode: str, device="cpu", kinds: Sequence[str] = ("single", "lattice"), thin: bool = False) -> List[Job]:
    L, w = case.flen, case.wavelet
    pitch = L + 2
    out: List[Job] = []
    if case.ndim == 2:
        for (h, wd, kind) in case.planes(mode):
            if kind not in kinds:
                continue
            if case.direction == 0:
                op_r, op_c = fwd_op(w, h, mode), fwd_op(w, wd, mode)
                x = probes_2d(kind, h, wd, pitch, amplitude(case, op_r, op_c), device)
                out.append(Job(case, mode, "%dx%d %s" % (h, wd, kind), x, op_c, op_r))
            else:  # the coefficient extents of that plane; the trims give the plane back (one sample where its extent is odd)
                mh, mw = coef_extent(h, L), coef_extent(wd, L)
                op_r, op_c = inv_op(w, mh, 2 * mh - L + 2 - h), inv_op(w, mw, 2 * mw - L + 2 - wd)
                x = band_probes_2d(kind, mh, mw, pitch, amplitude(case, op_r, op_c), device)
                out.append(Job(case, mode, "%dx%d coefficients -> %dx%d %s" % (mh, mw, h, wd, kind), x, op_c, op_r, extra=(mh, mw, h, wd)))
        if thin:
            for j in out:
                if j.label.endswith("single"):
                    j.x = thin_single(j.x)
                else:  # the diagonal shifts (k, k) alone: every residue of the rows and of the columns still occurs
                    keep = [0] + list(range(2 * pitch - 1, 3 * pitch - 2))
                    j.x = j.x.reshape(-1, 3 * pitch - 2, *j.x.shape[1:])[:, keep].reshape(-1, *j.x.shape[1:])
    else:
        for n in (2 * L + 1,) + tuple(case.lengths):
            if case.direction == 0:
                op = fwd_op(w, n, mode)
                out.append(Job(case, mode, "n=%d" % n, impulses_1d(n, amplitude(case, op), device), op))
            else:
                m = coef_extent(n, L)
                op = inv_op(w, m, 2 * m - L + 2 - n)
                out.append(Job(case, mode, "m=%d -> n=%d" % (m, n), impulses_1d(2 * m, amplitude(case, op), device), op, extra=(m, n)))
    return out


def resolvable_entries(op: AxisOp, arith: Arith) -> np.ndarray:
    """The operator entries the coverage counts: those larger than the worst-case rounding error of their OWN sum of taps,
    |M| > E + gamma_adds(L) |hat(M)|.  Everywhere but in constant mode an entry is one tap (or two mirrored ones) and this holds for
    every nonzero entry.  In constant mode up to L - 1 taps meet the replicated border sample; the high-pass taps sum to zero, so a
    few border entries of the high-pass rows are cancelling sums (exactly 0 up to the float64 residue 1e-17 where the whole window
    lies on the border sample; 2e-6 .. 4e-6 for db14 against sum |t| = 3): no worst-case bound can tell them from zero, whatever
    the plane.  tests/test_probe_host.py asserts where they may occur and how many."""
    _, e, mag = op.hat(arith)
    return np.abs(op.M) > e + gamma(arith.adds(op.L), arith.u) * mag


def seen_mask(op: AxisOp, feed: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """Coverage of the operator applied along the LAST axis: zeroing the entry M[k, j] alone changes output column k of every image by
    |M[k, j]| . feed[..., j] (feed = |what the pass reads, carried through the other pass|, (B, rows, n)); the entry is SEEN when that
    change exceeds the bound (B, rows, outputs) at some element of some image.  Returns the boolean mask of the seen entries."""
    M = torch.from_numpy(np.abs(op.M)).to(feed.device)
    f_t = feed.reshape(-1, feed.shape[-1]).T.contiguous()     # (n, B rows)
    b_t = bound.reshape(-1, bound.shape[-1]).T.contiguous()   # (outputs, B rows)
    seen = torch.zeros_like(M, dtype=torch.bool)
    jj, pp = torch.nonzero(f_t > 0, as_tuple=True)            # the (column, position) pairs that carry anything: few, the probes are sparse
    if jj.numel() == 0:
        return seen
    nz = M > 0
    width = int(nz.sum(dim=0).max())
    if width == 0:
        return seen
    # per column its nonzero rows, padded to a common width (an entry of the padding is invalid)
    order = torch.argsort(nz.to(torch.int8), dim=0, descending=True, stable=True)[:width].T   # (n, width)
    valid = torch.gather(nz.T, 1, order)
    for sl in chunks(int(jj.numel()), 1 << 18):
        j, pos = jj[sl], pp[sl]
        k = order[j]                                            # (N, width)
        hit = (M[k, j.unsqueeze(1)] * f_t[j, pos].unsqueeze(1) > b_t[k, pos.unsqueeze(1)]) & valid[j]
        seen[k[hit], j.unsqueeze(1).expand_as(k)[hit]] = True
    return seen


# --------------------------------------------------------------------------------------------------- several levels in one launch
# The reference of a multi-level case is the oracle called with level=k on the probe batch itself.  Its own sums (a product and an
# addition per tap, float64) err by the same recurrence with 2 L roundings of u64 per level; that term is added to the bound of the
# float64 cases, where it is of the size of the kernel's own.
REF64 = Arith("the oracle's float64 sums", U64, "exact", lambda L: 2 * L, None, None, torch.float64)


def level_sizes(n: int, L: int, levels: int) -> List[int]:
    s = [n]
    for _ in range(levels):
        s.append(coef_extent(s[-1], L))
    return s


def _sl(o, idx):
    return State(o.want[idx], o.err[idx]) if isinstance(o, State) else o[idx]


def _cat(parts, dim=-1):
    if isinstance(parts[0], State):
        return State(torch.cat([p.want for p in parts], dim), torch.cat([p.err for p in parts], dim))
    return torch.cat(parts, dim)


def _flat(o):
    return State(o.want.flatten(1), o.err.flatten(1)) if isinstance(o, State) else o.flatten(1)


def _unflat(o, h, w):
    return State(o.want.reshape(-1, h, w), o.err.reshape(-1, h, w)) if isinstance(o, State) else o.reshape(-1, h, w)


class ChainJob:
    """A multi-level case (kernel ids 14 / 15, 17 / 18, 20 / 21): e_0 = 0, m_0 = |x|, then per level e_k = |W_k| e_{k-1} + (the
    per-level terms of ``axis_pass`` at m_{k-1}), m_k = |want_k| + e_k.  Between the levels these kernels keep the running
    approximation in their own precision (f32 / f64 in LDS, mifwt_dwt1_tail.hip, mifwt_dwt1_long.hip, mifwt_dwt2_fwd_small.hip): no
    storage rounding.  The coefficient set is a flat vector: 1-D [a_K | d_K | ... | d_1]; 2-D [aa_K | (ad, da, dd)_K | ... |
    (ad, da, dd)_1], every band flattened — the result of an analysis, the input of a synthesis."""

    def __init__(self, case: Case, mode: str, label: str, x: torch.Tensor, extents: Tuple[int, ...]):
        self.case, self.mode, self.label, self.x, self.extents = case, mode, label, x, extents
        L, w, K = case.flen, case.wavelet, case.levels
        self.sizes = [level_sizes(n, L, K) for n in extents]
        if case.direction == 0:
            self.ops = [[fwd_op(w, s[k], mode) for s in self.sizes] for k in range(K)]
        else:  # coarsest level first; the trim gives the next finer extent back
            # (the finest level is not trimmed: waverec returns 2 m - L + 2 samples, one more than an odd signal had)
            self.ops = [[inv_op(w, s[k], 2 * s[k] - L + 2 - s[k - 1] if k > 1 else 0) for s in self.sizes] for k in range(K, 0, -1)]
        self.op_c, self.op_r = self.ops[0][-1], (self.ops[0][0] if case.ndim == 2 else None)

    # -- the chain, on States (bound) or tensors (emulation); ``step(o, op, axis)`` is one axis pass
    def _chain(self, o, step):
        K = self.case.levels
        if self.case.ndim == 1 and self.case.direction == 0:
            outs = []
            for k in range(K):
                y = step(o, self.ops[k][0], -1)
                m = self.sizes[0][k + 1]
                outs.insert(0, _sl(y, (Ellipsis, slice(m, None))))
                o = _sl(y, (Ellipsis, slice(0, m)))
            return _cat([o] + outs)
        if self.case.ndim == 1:
            s = self.sizes[0]
            off, cur = s[K], _sl(o, (Ellipsis, slice(0, s[K])))
            for i, k in enumerate(range(K, 0, -1)):
                d = _sl(o, (Ellipsis, slice(off, off + s[k])))
                off += s[k]
                cur = step(_cat([cur, d]), self.ops[i][0], -1)
            return cur
        if self.case.direction == 1:  # 2-D synthesis: vertical pass first (mifwt_dwt2_inv_small.hip), coarsest level first
            sh, sw = self.sizes
            cur, off = _unflat(_sl(o, (Ellipsis, slice(0, sh[K] * sw[K]))), sh[K], sw[K]), sh[K] * sw[K]
            for i, k in enumerate(range(K, 0, -1)):
                n = sh[k] * sw[k]
                ad, da, dd = (_unflat(_sl(o, (Ellipsis, slice(off + b * n, off + (b + 1) * n))), sh[k], sw[k]) for b in range(3))
                off += 3 * n
                op_r, op_c = self.ops[i]
                cur = step(step(_cat([_cat([cur, ad], -1), _cat([da, dd], -1)], -2), op_r, -2), op_c, -1)
            return _flat(cur)
        outs = []
        for k in range(K):
            op_r, op_c = self.ops[k]
            y = step(step(o, op_c, -1), op_r, -2)
            mh, mw = self.sizes[0][k + 1], self.sizes[1][k + 1]
            bands = [_flat(_sl(y, (Ellipsis, slice(0, mh), slice(mw, None)))), _flat(_sl(y, (Ellipsis, slice(mh, None), slice(0, mw)))),
                     _flat(_sl(y, (Ellipsis, slice(mh, None), slice(mw, None))))]
            outs = bands + outs
            o = _sl(y, (Ellipsis, slice(0, mh), slice(0, mw)))
        return _cat([_flat(o)] + outs)

    def oracle(self, x: torch.Tensor) -> torch.Tensor:
        """The float64 reference: the oracle called with level=k on the probe batch."""
        xn, w, K = x.cpu().numpy(), self.case.wavelet, self.case.levels
        if self.case.ndim == 1 and self.case.direction == 0:
            flat = np.concatenate(O.wavedec(xn, w, mode=self.mode, level=K), axis=-1)
        elif self.case.ndim == 1:
            s = self.sizes[0]
            cuts = np.cumsum([s[K]] + [s[k] for k in range(K, 0, -1)])[:-1]
            flat = O.waverec(np.split(xn, cuts, axis=-1), w)
        elif self.case.direction == 1:
            sh, sw = self.sizes
            parts, off = [xn[:, : sh[K] * sw[K]].reshape(-1, sh[K], sw[K])], sh[K] * sw[K]
            for k in range(K, 0, -1):
                n = sh[k] * sw[k]
                ad, da, dd = (xn[:, off + b * n: off + (b + 1) * n].reshape(-1, sh[k], sw[k]) for b in range(3))
                off += 3 * n
                parts.append((da, ad, dd))
            flat = O.waverec2(tuple(parts), w).reshape(len(xn), -1)
        else:
            c = O.wavedec2(xn, w, mode=self.mode, level=K)
            flat = np.concatenate([c[0].reshape(len(xn), -1)] + [b.reshape(len(xn), -1) for lvl in c[1:] for b in (lvl[1], lvl[0], lvl[2])], axis=-1)
        return torch.from_numpy(np.ascontiguousarray(flat)).to(x.device)

    def bound(self, x: torch.Tensor) -> State:
        a = self.case.arith
        st = self._chain(State(x), lambda o, op, axis: axis_pass(o, op, a, axis, None))
        want = self.oracle(x)
        err = st.err + (want - st.want).abs()  # (the two float64 evaluations differ by their own rounding)
        if self.case.dtype == "f64":
            err = err + self._chain(State(x), lambda o, op, axis: axis_pass(o, op, REF64, axis, None)).err
        return State(want, err)

    def emulate(self, x: torch.Tensor, **mut) -> torch.Tensor:
        a = self.case.arith
        return self._chain(x, lambda o, op, axis: emulate_pass(o, op, a, axis, None, **mut))

    def where(self, idx: int, shape) -> str:
        b, k = np.unravel_index(idx, tuple(shape))
        return "%s %s %s: probe image %d, element %d of the flat result (levels %s)" % (self.case.id, self.mode, self.label, b, k, self.sizes)


def chain_cases() -> List[Case]:
    t: List[Case] = []
    three = ("reflect", "periodic", "zero")
    for dt in ("f32", "f64"):
        for w in ("sym16", "db10"):  # one workgroup per row, every level in LDS
            t.append(Case("tail_fwd", (14,), 0, 1, dt, w, three, lengths=(1001,), levels=3))
            t.append(Case("tail_inv", (15,), 1, 1, dt, w, three[:1], lengths=(1001,), levels=3))
    for w in ("db10", "sym10"):  # the shortest row the chunked route takes is 4096 samples; 4101 is no multiple of any chunk
        t.append(Case("long_fwd", (17,), 0, 1, "f32", w, three, lengths=(4101,), levels=3))
        t.append(Case("long_inv", (18,), 1, 1, "f32", w, three[:1], lengths=(4101,), levels=2))
        t.append(Case("small_fwd", (20,), 0, 2, "f32", w, ALL_MODES, levels=2))
        t.append(Case("small_inv", (21,), 1, 2, "f32", w, ALL_MODES[:1], levels=2))
    return t


# planes of the small-plane pyramid kernel at 20 taps, two levels, a lattice batch of 64 images: the route takes 20 x 21 .. 76 x 77
# (the engine's plan, queried on the host: tests/test_probe_host.py); periodic: the multiples of the pitch 22 inside that range
# (21 x 22 is the smallest plane whose SECOND level still passes the reference's reflect pad check: 20 samples > 18 + 0)
SMALL_PLANES = {False: ((21, 22), (76, 77)), True: ((22, 22), (66, 66))}


# ... and of the small-plane reconstruction (id 21): the two-level coefficient sets of 21 x 22 (as above) and of 85 x 86, the largest
# plane the route takes for the batch of 7 x 64 images (a lattice in each of the seven bands in turn)
SMALL_INV_PLANES = ((21, 22), (85, 86))


def band_lattices_flat(sh: Sequence[int], sw: Sequence[int], levels: int, pitch: int, device="cpu") -> torch.Tensor:
    """The flat two-level (K-level) coefficient sets with a lattice of impulses in one band at a time, the other bands zero: band
    order aa_K, (ad, da, dd)_K, ..., (ad, da, dd)_1; 3 pitch - 2 shifts per band."""
    bands = [(sh[levels], sw[levels])] + [(sh[k], sw[k]) for k in range(levels, 0, -1) for _ in range(3)]
    total = sum(h * w for h, w in bands)
    rows, off = [], 0
    for h, w in bands:
        lat = lattice_2d(h, w, pitch, 1.0, device).flatten(1)
        x = torch.zeros(lat.shape[0], total, dtype=torch.float64, device=device)
        x[:, off:off + h * w] = lat
        rows.append(x)
        off += h * w
    return torch.cat(rows, 0)


def chain_jobs(case: Case, mode: str, device="cpu") -> List[ChainJob]:
    L = case.flen
    if case.ndim == 1:
        out = []
        for n in case.lengths:
            s = level_sizes(n, L, case.levels)
            width = n if case.direction == 0 else s[-1] + sum(s[1:])
            out.append(ChainJob(case, mode, "n=%d, %d levels" % (n, case.levels), impulses_1d(width, 1.0, device), (n,)))
        return out
    if case.direction == 1:
        out = []
        for h, w in SMALL_INV_PLANES:
            sh, sw = level_sizes(h, L, case.levels), level_sizes(w, L, case.levels)
            x = band_lattices_flat(sh, sw, case.levels, L + 2, device)
            out.append(ChainJob(case, mode, "coefficients of %dx%d, lattice in each band, %d levels" % (h, w, case.levels), x, (h, w)))
        return out
    return [ChainJob(case, mode, "%dx%d lattice, %d levels" % (h, w, case.levels), lattice_2d(h, w, L + 2, 1.0, device), (h, w))
            for h, w in SMALL_PLANES[mode == "periodic"]]

