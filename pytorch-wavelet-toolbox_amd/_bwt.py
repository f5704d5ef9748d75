"""Host path of the boundary-wavelet levels (C ABI ``mifwt_bwt_*``, include/mifwt.h; kernels csrc/mifwt_bwt.hip).

A *bank* is what one direction of the transform applies: the two row filters ``f`` of ``_boundary.py`` and the boundary tables
built from them.  Two level maps exist,

    rows(bank, mode)        x [B, n..]              -> buffer [B, 2^d, M..]   c = B x          (analysis; adjoint of synthesis)
    transposed(bank, n..)   bands [B, M..] each     -> y [B, n..]             y = B^T c        (synthesis; adjoint of analysis)

each one fused launch per level (kernel ids 26 / 27) for float32 / float64, even ``L <= 20`` and axes of at least ``2 (L-1)``
samples; longer filters run one generic launch per axis (28 / 29); a level with an axis shorter than ``2 (L-1)`` — a few dozen
samples — is a dense ``torch.matmul`` with the small level matrix.  Three transformed axes have kernels of their own (ids 30 / 31,
csrc/mifwt_bwt3.hip: even ``L <= 8``); what they decline runs the axis passes width, height, depth — seven launches per level.  The tables are cached per bank and uploaded once per device;
after that a call allocates its outputs and enqueues launches, nothing else: no host round trip, capturable.

Packet trees (``packets.py``, ``mode="boundary"``) expand whole levels: ``rows_tree`` / ``transposed_tree`` compute two or more consecutive
levels of a 1-D tree in ONE launch (ids 32 / 33, csrc/mifwt_bwt_tree.hip: a row and its next level stay in LDS); ``tree_route`` splits a
range of levels into such runs and per-level launches.  No autograd: a tree that wants gradients runs level by level through ``rows`` /
``transposed``.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Set, Tuple

import numpy as np
import torch

from . import _boundary, _engine

KID_FWD, KID_INV, KID_AXIS_FWD, KID_AXIS_INV = 26, 27, 28, 29
KID_FWD3, KID_INV3 = 30, 31
KID_TREE_FWD, KID_TREE_INV = 32, 33

_ZERO, _REFLECT = _engine.MODE_IDS["zero"], _engine.MODE_IDS["reflect"]

# Tests and tools/boundary_bench.py set this to run a 3-D level through the composed axis passes although the fused kernel would take it.
FORCE_COMPOSED3 = False
# (direction, dtype, L) cells of the fused 3-D envelope that go to the composed passes all the same (direction 0 analysis, 1 synthesis).
# A cell belongs to the bricks only where `tools/boundary_bench.py --shape cells` has shown the fused median ahead of the composed one by
# more than the spread of its windows (EXPERIMENTS.md part B).  The synthesis bricks for 6 and 8 taps hold a CU alone (100 - 150 KB of
# LDS, csrc/mifwt_bwt3.hip) and have no such measurement: they are routed to the axis passes.
COMPOSED3_CELLS: Set[Tuple[int, torch.dtype, int]] = {(1, dt, flen) for dt in (torch.float32, torch.float64) for flen in (6, 8)}


# Tests and tools/boundary_bench.py set this to run a packet tree on per-level launches although a subtree launch (ids 32 / 33) would take it.
FORCE_PER_LEVEL_TREE = False
# (direction, dtype) cells of the subtree envelope that stay on per-level launches all the same (direction 0 analysis, 1 synthesis): the rule of
# COMPOSED3_CELLS — a cell is on the subtree kernels only where `tools/boundary_bench.py --shape packets` has shown their median ahead of the
# per-level one by more than the spread of its windows (EXPERIMENTS.md part B).  No cell has such a measurement yet: all four are listed, the
# subtree kernels run where a caller (the tests, the benchmark tool) empties this set.
PER_LEVEL_TREE_CELLS: Set[Tuple[int, torch.dtype]] = {(d, dt) for d in (0, 1) for dt in (torch.float32, torch.float64)}


def _composed3(direction: int, dtype: torch.dtype, flen: int) -> bool:
    return FORCE_COMPOSED3 or (direction, dtype, flen) in COMPOSED3_CELLS


class BwtTables(ctypes.Structure):
    """Mirror of ``mifwt_bwt_tables``."""

    _fields_ = [("rows", ctypes.c_void_p), ("n_top", ctypes.c_int32), ("n_bot", ctypes.c_int32)]


_ci, _i64, _vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
_dbl_p, _i64_p, _vpp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_i64), ctypes.POINTER(_vp)
_desc_p, _tab_p = ctypes.POINTER(_engine.LevelDesc), ctypes.POINTER(BwtTables)
_FWD, _INV = [_desc_p, _vp, _vp, _vpp, _dbl_p, _dbl_p, _tab_p, _vp], [_desc_p, _vp, _vpp, _vp, _dbl_p, _dbl_p, _tab_p, _vp]
_engine.register_entries({
    **{name: (_ci, [_desc_p, _ci]) for name in ("mifwt_bwt_supported", "mifwt_bwt_kernel_id", "mifwt_bwt3_supported", "mifwt_bwt3_kernel_id")},
    "mifwt_bwt_fwd": (_ci, _FWD), "mifwt_bwt_inv": (_ci, _INV), "mifwt_bwt3_fwd": (_ci, _FWD), "mifwt_bwt3_inv": (_ci, _INV),
    "mifwt_bwt_axis_fwd": (_ci, [_ci, _ci, _ci, _i64, _i64, _i64, _vp, _i64_p, _vp, _i64_p, _vp, _i64_p, _dbl_p, _dbl_p, _tab_p, _vp]),
    "mifwt_bwt_axis_inv": (_ci, [_ci, _ci, _i64, _i64, _i64, _vp, _i64_p, _vp, _i64_p, _vp, _i64_p, _dbl_p, _dbl_p, _tab_p, _vp]),
    "mifwt_bwt_tree_levels": (_ci, [_ci, _ci, _i64, _ci]),
    "mifwt_bwt_tree_fwd": (_ci, [_ci, _ci, _i64, _i64, _i64, _ci, _vp, _vpp, _dbl_p, _dbl_p, _tab_p, _vp]),
    "mifwt_bwt_tree_inv": (_ci, [_ci, _ci, _i64, _i64, _ci, _vp, _vpp, _dbl_p, _dbl_p, _tab_p, _vp]),
})
_lib = _engine.load_library


class Bank:
    """Row filters + boundary tables of one direction ("analysis" / "synthesis") of a filter bank; device copies are made once per
    device and kept."""

    def __init__(self, taps: Tuple[Tuple[float, ...], ...], method: str, which: str):
        self.taps, self.method, self.which = taps, method, which
        f_lo, f_hi = _boundary.row_filters(taps, which)
        self.filt_len = len(f_lo)
        self.f_lo, self.f_hi = tuple(float(v) for v in f_lo), tuple(float(v) for v in f_hi)
        self.r_lo, self.r_hi = self.f_lo[::-1], self.f_hi[::-1]
        self.n_top, self.n_bot = _boundary.boundary_rows(self.filt_len)
        self._host_tab = _boundary.kernel_tables(taps, method, which)
        self._dev: Dict[torch.device, Tuple[torch.Tensor, BwtTables]] = {}
        self._dense: dict = {}

    def tables(self, device: torch.device) -> BwtTables:
        hit = self._dev.get(device)
        if hit is None:
            t = torch.from_numpy(np.ascontiguousarray(self._host_tab)).to(device)
            hit = self._dev[device] = (t, BwtTables(t.data_ptr(), self.n_top, self.n_bot))
        return hit[1]

    def dense(self, n: int, device: torch.device, dtype: torch.dtype) -> torch.Tensor:
        """The rows of this bank for an even length ``n`` as a dense [n, n] matrix on the device (short levels)."""
        key = (n, device, dtype)
        m = self._dense.get(key)
        if m is None:
            a = _boundary.level_matrix(self.taps, n, self.method, self.which)
            a = a if self.which == "analysis" else a.T
            m = self._dense[key] = torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
        return m


_banks: dict = {}


def bank(taps, method: str, which: str) -> Bank:
    key = (taps, which)  # (both methods give the same tables, _boundary.py)
    b = _banks.get(key)
    if b is None:
        if len(_banks) > 256:
            _banks.clear()
        b = _banks[key] = Bank(taps, method, which)
    return b


def virtual_source(n: int, mode_id: int) -> int:
    """Index of the sample the virtual sample of an odd extent copies (-1: it is zero) — one sample of the reference's _fwt_pad."""
    return {0: -1, 1: n - 1, 2: n - 2, 3: 0, 4: n - 1}[mode_id]


def is_short(extents: Sequence[int], flen: int) -> bool:
    return any(n + (n & 1) < 2 * (flen - 1) for n in extents)


_plans: dict = {}
_engine._routing_caches.append(_plans)


_desc, _unit_last = _engine._desc, _engine._unit_last


def _launch(direction: int, kid: int, extent, anchor: torch.Tensor, entry, *args) -> None:
    _engine._run(("bwt_fwd", "bwt_inv")[direction], kid, extent, anchor, entry, args)


def _axis_strides(t: torch.Tensor):
    """(outer, axis, inner) strides of an [outer, n, inner] view, as the axis passes 28 / 29 take them."""
    return _engine._arr(ctypes.c_int64, 3)(*t.stride())


def _outer_axis_inner(t: torch.Tensor, axis: int) -> torch.Tensor:
    """A [B, d0(, d1(, d2))] tensor as the [outer, n, inner] view whose middle axis is ``axis`` (1 .. 3)."""
    return t.reshape(int(np.prod(t.shape[:axis])), t.shape[axis], int(np.prod(t.shape[axis + 1:])))


def _route(direction: int, key, ndim: int, dtype: torch.dtype, flen: int, desc):
    """(reference to the level descriptor, kernel id) of a level; -2: no fused kernel takes it, it runs the composed axis passes.
    The descriptor ``desc()`` builds and the kernel's answer are cached under ``key``."""
    def build():
        lib, d = _lib(), desc()
        kid = (lib.mifwt_bwt3_kernel_id if ndim == 3 else lib.mifwt_bwt_kernel_id)(ctypes.byref(d), direction)
        if kid < 0 and kid != -2:
            _engine._check(kid)
        return d, ctypes.byref(d), kid

    _, ref, kid = _engine._plan(key, build, _plans)
    if kid == (KID_FWD3, KID_INV3)[direction] and _composed3(direction, dtype, flen):
        kid = -2
    return ref, kid


def _composed_setup(t: torch.Tensor, ndim: int):
    """What the composed axis passes need before their first launch: the dtype id, and the refusals."""
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"Input dtype {t.dtype} not supported by the boundary-wavelet transforms (float32 / float64)")
    if ndim > 3:
        raise NotImplementedError("boundary-wavelet levels exist for one, two and three transformed axes")
    return _engine._DTYPE_IDS[t.dtype]


# ---- the two level maps (no autograd) ---------------------------------------------------------------------------------------------
def rows_level(x: torch.Tensor, bk: Bank, mode_id: int) -> torch.Tensor:
    """x [B, n0(, n1(, n2))] -> buffer [B, 2^d, M0(, M1(, M2))], plane s = band s (bit (d-1-a) of s set <=> high-pass along axis a)."""
    _engine._require_gpu(x)
    ndim = x.dim() - 1
    sig = [int(n) for n in x.shape[1:]]
    coef = [(n + 1) // 2 for n in sig]
    L = bk.filt_len
    if mode_id == _REFLECT and 1 in sig:
        # (an odd extent of one sample has nothing to reflect: torch's reflection padding, which the reference uses, refuses it too)
        raise ValueError("odd_coeff_padding_mode='reflect' needs at least two samples along every transformed axis")
    if is_short(sig, L):
        return _rows_dense(x, bk, mode_id)
    x = _unit_last(x)
    b = x.shape[0]
    buf = torch.empty((b, 1 << ndim, *coef), dtype=x.dtype, device=x.device)
    if buf.numel() == 0:
        return buf
    lib = _lib()
    st = [buf.stride(0), *buf.stride()[2:]]
    ref, kid = _route(0, (0, x.shape, x.stride(), x.dtype, mode_id, L), ndim, x.dtype, L,
                      lambda: _desc(ndim, x.dtype, mode_id, L, b, sig, x.stride(), coef, st, st))
    tab = bk.tables(x.device)
    lo, hi = _engine._taps_array(bk.f_lo), _engine._taps_array(bk.f_hi)
    if kid in (KID_FWD, KID_FWD3):
        base, xp = buf.data_ptr(), x.data_ptr()
        ptrs = _engine._band_ptrs(base, buf.stride(1) * x.element_size(), (1 << ndim) - 1)
        _launch(0, kid, sig, x, lib.mifwt_bwt3_fwd if kid == KID_FWD3 else lib.mifwt_bwt_fwd, ref, xp, base, ptrs, lo, hi, ctypes.byref(tab))
        return buf
    dt = _composed_setup(x, ndim)
    if ndim > 1:
        x = x.contiguous()
    # One pass per axis, last axis first: 1 (+ 2 (+ 4)) launches.  Stage k holds 2^k planes; the pass over plane p writes its low band
    # to plane p and its high band to plane p + 2^k; the planes of the last stage are the bands of `buf`.
    cur = [x]
    for axis in range(ndim, 0, -1):
        npl = len(cur)
        if axis == 1:
            out = [buf[:, s] for s in range(2 * npl)]
        else:
            out = torch.empty((2 * npl, b, *sig[:axis - 1], *coef[axis - 1:]), dtype=x.dtype, device=x.device)
        n, outer, inner = sig[axis - 1], b * int(np.prod(sig[:axis - 1])), int(np.prod(coef[axis:]))
        for pl in range(npl):
            src, o_lo, o_hi = (_outer_axis_inner(t, axis) for t in (cur[pl], out[pl], out[npl + pl]))
            _launch(0, KID_AXIS_FWD, (n,), src, lib.mifwt_bwt_axis_fwd, dt, L, mode_id, outer, n, inner, src.data_ptr(), _axis_strides(src),
                    o_lo.data_ptr(), _axis_strides(o_lo), o_hi.data_ptr(), _axis_strides(o_hi), lo, hi, ctypes.byref(tab))
        cur = out
    return buf


def transposed_level(bands: Sequence[torch.Tensor], bk: Bank, out_extent: Sequence[int]) -> torch.Tensor:
    """bands (2^d tensors [B, M0(, M1(, M2))], band order as above) -> y [B, n0(, n1(, n2))], n in {2 M, 2 M - 1} per axis."""
    a0 = bands[0]
    _engine._require_gpu(a0)
    ndim = a0.dim() - 1
    coef = [int(m) for m in a0.shape[1:]]
    sig = [int(n) for n in out_extent]
    L = bk.filt_len
    if is_short(sig, L):
        return _transposed_dense(bands, bk, sig)
    bands = [_unit_last(t) for t in bands]
    bands = [bands[0], *_engine._share_strides(bands[1:])[0]]
    b = a0.shape[0]
    y = torch.empty((b, *sig), dtype=a0.dtype, device=a0.device)
    if y.numel() == 0:
        return y
    lib = _lib()
    ref, kid = _route(1, (1, a0.shape, tuple(sig), bands[0].stride(), bands[1].stride(), a0.dtype, L), ndim, a0.dtype, L,
                      lambda: _desc(ndim, a0.dtype, _ZERO, L, b, sig, y.stride(), coef, bands[0].stride(), bands[1].stride()))
    tab = bk.tables(a0.device)
    # (the C entries take the filters in rec order and reverse them into row filters)
    lo, hi = _engine._taps_array(bk.r_lo), _engine._taps_array(bk.r_hi)
    if kid in (KID_INV, KID_INV3):
        _launch(1, kid, sig, a0, lib.mifwt_bwt3_inv if kid == KID_INV3 else lib.mifwt_bwt_inv, ref, bands[0].data_ptr(), _engine._ptr_array(bands[1:]),
                y.data_ptr(), lo, hi, ctypes.byref(tab))
        return y
    dt = _composed_setup(a0, ndim)
    if ndim == 3:
        bands = [t.contiguous() for t in bands]
    # The mirror of the analysis passes, first axis first: (4 +) (2 +) 1 launches.  The pass that leaves 2^k planes takes the low band
    # from plane p and the high band from plane p + 2^k; the last one writes `y`.
    cur = bands
    for axis in range(1, ndim + 1):
        npl = len(cur) // 2
        out = [y] if axis == ndim else torch.empty((npl, b, *sig[:axis], *coef[axis:]), dtype=a0.dtype, device=a0.device)
        n, outer, inner = sig[axis - 1], b * int(np.prod(sig[:axis - 1])), int(np.prod(coef[axis:]))
        for pl in range(npl):
            c_lo, c_hi, dst = (_outer_axis_inner(t, axis) for t in (cur[pl], cur[npl + pl], out[pl]))
            _launch(1, KID_AXIS_INV, (n,), c_lo, lib.mifwt_bwt_axis_inv, dt, L, outer, n, inner, c_lo.data_ptr(), _axis_strides(c_lo),
                    c_hi.data_ptr(), _axis_strides(c_hi), dst.data_ptr(), _axis_strides(dst), lo, hi, ctypes.byref(tab))
        cur = out
    return y


# ---- packet trees: a run of levels per launch (no autograd) ---------------------------------------------------------------------------------
_tree_levels: dict = {}
_engine._routing_caches.append(_tree_levels)


def tree_levels(dtype: torch.dtype, flen: int, n: int, max_levels: int) -> int:
    """How many consecutive levels ONE subtree launch takes from a node of ``n`` samples (0: none) — ``mifwt_bwt_tree_levels``, cached."""
    key = (dtype, flen, n, max_levels)
    k = _tree_levels.get(key)
    if k is None:
        dt = _engine._DTYPE_IDS.get(dtype, -1)
        k = _tree_levels[key] = int(_lib().mifwt_bwt_tree_levels(dt, flen, n, max_levels)) if dt >= 0 and max_levels >= 2 else 0
    return k


def tree_route(n: int, flen: int, dtype: torch.dtype, first: int, last: int, assigned: Sequence[int] = (), direction: int = 0,
               node_len: Optional[int] = None) -> List[Tuple[int, int]]:
    """Split the expansion of levels ``first`` .. ``last`` of a 1-D packet tree over a root of ``n`` samples (``last`` > ``first``: the
    deepest level produced) into launches: a list of (input level, number of levels); 1 = a per-level launch, >= 2 = one subtree launch.
    A node of ``h`` samples has children of ``ceil(h / 2)``.  A level outside the subtree envelope (node too long, odd, short) is a
    per-level launch, every maximal run of at least two levels inside it one subtree launch; a run does not go past a level listed in
    ``assigned`` (levels that hold nodes set by the user: they are gathered before they are expanded), which may only be its input or
    its last output.  ``node_len``: the node length at ``first`` where it is not the one the root implies.  Pure: no device, no tensors."""
    h = n
    for _ in range(first):
        h = (h + 1) // 2
    if node_len is not None:
        h = node_len
    fused = not FORCE_PER_LEVEL_TREE and (direction, dtype) not in PER_LEVEL_TREE_CELLS
    steps: List[Tuple[int, int]] = []
    s = first
    while s < last:
        stop = min([last] + [t for t in assigned if t > s])
        k = tree_levels(dtype, flen, h, stop - s) if fused and stop - s >= 2 else 0
        if k < 2:
            k = 1
        steps.append((s, k))
        for _ in range(k):
            h = (h + 1) // 2
        s += k
    return steps


def tree_route_up(m: int, flen: int, dtype: torch.dtype, kmax: int, direction: int = 1) -> int:
    """Synthesis counterpart of :func:`tree_route`: from leaves of ``m`` samples whose ``kmax`` levels above double exactly, how many
    levels the next launch rebuilds — the longest subtree run (>= 2) inside the envelope, else 1."""
    if FORCE_PER_LEVEL_TREE or (direction, dtype) in PER_LEVEL_TREE_CELLS:
        return 1
    for k in range(kmax, 1, -1):
        if tree_levels(dtype, flen, m << k, k) == k:
            return k
    return 1


def rows_tree(x: torch.Tensor, bk: Bank, k: int) -> List[torch.Tensor]:
    """``k`` >= 2 analysis levels of a packet tree below every row of x [R, n] in one launch (id 32): the list of the level buffers
    [R, 2^i, n / 2^i], i = 1 .. k (node order = natural order of the paths).  (n, k) must be inside ``tree_levels``."""
    _engine._require_gpu(x)
    x = _unit_last(x)
    r, n = int(x.shape[0]), int(x.shape[1])
    if r > 1 and x.stride(0) < n:
        x = x.contiguous()
    out = [torch.empty((r, n), dtype=x.dtype, device=x.device) for _ in range(k)]
    if r:
        dt = _engine._DTYPE_IDS[x.dtype]
        tab, xs = bk.tables(x.device), x.stride(0) if r > 1 else n
        _launch(0, KID_TREE_FWD, (n,), x, _lib().mifwt_bwt_tree_fwd, dt, bk.filt_len, r, n, xs, k, x.data_ptr(), _engine._ptr_array(out),
                _engine._taps_array(bk.f_lo), _engine._taps_array(bk.f_hi), ctypes.byref(tab))
    return [out[i].view(r, 1 << (i + 1), n >> (i + 1)) for i in range(k)]


def transposed_tree(leaves: torch.Tensor, bk: Bank, k: int) -> List[torch.Tensor]:
    """``k`` >= 2 synthesis levels in one launch (id 33): leaves [R, 2^k, n / 2^k] -> the list of the level buffers [R, 2^i, n / 2^i],
    i = 0 .. k - 1 (entry 0 = the rebuilt rows [R, 1, n])."""
    _engine._require_gpu(leaves)
    leaves = leaves.contiguous()
    r = int(leaves.shape[0])
    n = int(leaves.shape[1] * leaves.shape[2])
    out = [torch.empty((r, n), dtype=leaves.dtype, device=leaves.device) for _ in range(k)]
    if r:
        dt = _engine._DTYPE_IDS[leaves.dtype]
        tab = bk.tables(leaves.device)
        # (the C entry takes the filters in rec order and reverses them into row filters)
        _launch(1, KID_TREE_INV, (n,), leaves, _lib().mifwt_bwt_tree_inv, dt, bk.filt_len, r, n, k, leaves.data_ptr(), _engine._ptr_array(out),
                _engine._taps_array(bk.r_lo), _engine._taps_array(bk.r_hi), ctypes.byref(tab))
    return [out[i].view(r, 1 << i, n >> i) for i in range(k)]


# ---- short levels: dense matrices, plain torch (differentiable as it stands, no host synchronisation) ----------------------------
def _with_virtual(x: torch.Tensor, dim: int, mode_id: int) -> torch.Tensor:
    n = x.shape[dim]
    if n % 2 == 0:
        return x
    src = virtual_source(n, mode_id)
    extra = x.narrow(dim, src, 1) if src >= 0 else torch.zeros_like(x.narrow(dim, 0, 1))
    return torch.cat([x, extra], dim)


def _rows_dense(x: torch.Tensor, bk: Bank, mode_id: int) -> torch.Tensor:
    ndim = x.dim() - 1
    for a in range(ndim):
        x = _with_virtual(x, 1 + a, mode_id)
    if ndim == 1:
        c = x @ bk.dense(x.shape[1], x.device, x.dtype).T
        return c.reshape(x.shape[0], 2, -1)
    if ndim == 3:
        m_d, m_r, m_c = (bk.dense(x.shape[1 + a], x.device, x.dtype) for a in range(3))
        c = m_r @ x @ m_c.T
        c = (m_d @ c.transpose(1, 2)).transpose(1, 2)
        d, h, w = (n // 2 for n in c.shape[1:])
        return c.reshape(x.shape[0], 2, d, 2, h, 2, w).permute(0, 1, 3, 5, 2, 4, 6).reshape(x.shape[0], 8, d, h, w)
    m_r = bk.dense(x.shape[1], x.device, x.dtype)
    m_c = bk.dense(x.shape[2], x.device, x.dtype)
    c = m_r @ x @ m_c.T
    h, w = c.shape[1] // 2, c.shape[2] // 2
    return c.reshape(x.shape[0], 2, h, 2, w).permute(0, 1, 3, 2, 4).reshape(x.shape[0], 4, h, w)


def _transposed_dense(bands: Sequence[torch.Tensor], bk: Bank, sig: Sequence[int]) -> torch.Tensor:
    a0 = bands[0]
    ndim = a0.dim() - 1
    if ndim == 1:
        c = torch.cat([bands[0], bands[1]], -1)
        y = c @ bk.dense(c.shape[-1], a0.device, a0.dtype)
        return y[:, : sig[0]]
    if ndim == 3:
        halves = [torch.cat([torch.cat([bands[q], bands[q + 1]], -1), torch.cat([bands[q + 2], bands[q + 3]], -1)], -2) for q in (0, 4)]
        c = torch.cat(halves, -3)
        m_d, m_r, m_c = (bk.dense(c.shape[1 + a], a0.device, a0.dtype) for a in range(3))
        y = m_r.T @ c @ m_c
        y = (m_d.T @ y.transpose(1, 2)).transpose(1, 2)
        return y[:, : sig[0], : sig[1], : sig[2]]
    c = torch.cat([torch.cat([bands[0], bands[1]], -1), torch.cat([bands[2], bands[3]], -1)], -2)
    y = bk.dense(c.shape[1], a0.device, a0.dtype).T @ c @ bk.dense(c.shape[2], a0.device, a0.dtype)
    return y[:, : sig[0], : sig[1]]


# ---- autograd: each map's backward is the other map with the same bank ---------------------------------------------------------------
def _fold_virtual(t: torch.Tensor, dim: int, n: int, src: int) -> torch.Tensor:
    """Gradient of appending the virtual sample along ``dim``: drop entry n, add it onto entry ``src``."""
    if t.shape[dim] == n:
        return t
    main = t.narrow(dim, 0, n)
    if src < 0:
        return main
    parts = [main.narrow(dim, 0, src), main.narrow(dim, src, 1) + t.narrow(dim, n, 1), main.narrow(dim, src + 1, n - src - 1)]
    return torch.cat(parts, dim)


class _Rows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bk, mode_id):
        ctx.meta = (bk, mode_id, tuple(x.shape[1:]))
        return rows_level(x, bk, mode_id)

    @staticmethod
    def backward(ctx, g):
        bk, mode_id, sig = ctx.meta
        full = [n + (n & 1) for n in sig]
        g_x = _Transposed.apply(bk, tuple(full), *[g[:, s] for s in range(g.shape[1])])
        for a, n in enumerate(sig):
            g_x = _fold_virtual(g_x, 1 + a, n, virtual_source(n, mode_id))
        return g_x, None, None


class _Transposed(torch.autograd.Function):
    @staticmethod
    def forward(ctx, bk, out_extent, *bands):
        ctx.bk = bk
        return transposed_level(bands, bk, out_extent)

    @staticmethod
    def backward(ctx, g_y):
        g = _Rows.apply(g_y, ctx.bk, _ZERO)
        return (None, None, *[g[:, s] for s in range(g.shape[1])])


def rows(x: torch.Tensor, bk: Bank, mode_id: int) -> torch.Tensor:
    if is_short(x.shape[1:], bk.filt_len) or not (torch.is_grad_enabled() and x.requires_grad):
        return rows_level(x, bk, mode_id)
    return _Rows.apply(x, bk, mode_id)


def transposed(bands: Sequence[torch.Tensor], bk: Bank, out_extent: Sequence[int]) -> torch.Tensor:
    if is_short(out_extent, bk.filt_len) or not (torch.is_grad_enabled() and any(t.requires_grad for t in bands)):
        return transposed_level(bands, bk, out_extent)
    return _Transposed.apply(bk, tuple(out_extent), *bands)


# ---- the level matrices as sparse tensors (sparse_fwt_operator / sparse_ifwt_operator) ------------------------------------------------
def sparse_level(bk: Bank, n: int, device, dtype) -> torch.Tensor:
    """Rows of the bank for an even length ``n`` as a torch sparse COO matrix [n, n] (assembled on the host from the tables)."""
    r, c, v = _boundary.level_coo(bk.taps, n, bk.method, bk.which)  # (analysis: A;  synthesis: S, already transposed)
    t = torch.sparse_coo_tensor(np.stack([r, c]), v, size=(n, n), dtype=torch.float64)
    return t.to(device=device, dtype=dtype).coalesce()
