"""Best basis of a wavelet packet tree (Coifman-Wickerhauser; MATLAB's ``wentropy`` / ``besttree``): the additive cost of every node of
every level in ONE HIP launch (C ABI ``mifwt_cost_*``, include/mifwt.h; kernels csrc/mifwt_cost.hip, ids 61 / 62), the pruning as a
few float64 torch operations per level, and a reconstruction from exactly the chosen nodes.

    wp = ptwt_amd.WaveletPacket2D(x, "db4", mode="periodization", maxlevel=3)
    basis = wp.best_basis("shannon")                 # one basis for the batch: a list of keys
    for key in basis:
        wp[key] = ptwt_amd.threshold(wp[key], 0.1, "soft")
    y = wp.reconstruct_basis(basis)[""]

All nodes of a level live in one buffer ``[B, nb, .., nb, extents..]`` (packets.py), so the costs of a level are a segmented reduction
over contiguous nodes of one length, and a tree is one segment table.  Terms are evaluated and accumulated in float64 for float32 and
float64 data, in an order fixed by dtype and shapes: two calls give the same bits.  Nothing is read back except by
``best_basis(joint=True)``; everything else can be captured.

:func:`_composed_costs` states the same closed forms as float64 torch operations.  It serves calls that want a gradient (any order; the
gradient at an element that is exactly 0 is 0), CPU tensors, sizes beyond the kernel's guards, the cells of ``COMPOSED_CELLS``, and the
benchmark (tools/best_basis_bench.py) as the emulation the kernel is measured against.
"""
from __future__ import annotations

import ctypes
import math
import numbers
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _engine
from . import estimators as _est
from . import packets as _packets

__all__ = ["wentropy"]

KID_COST_NODES, KID_COST_FINISH = 61, 62
#: ``functional`` of the C ABI (MIFWT_COST_*)
COSTS = {"shannon": 0, "logenergy": 1, "norm": 2, "threshold": 3, "sure": 4}
#: (dtype, transformed axes of the tree — 0 for :func:`wentropy` —, "short" / "long") cells whose costs come from the torch composition
#: instead of the kernel: a cell belongs here only where tools/best_basis_bench.py has shown the kernel's median behind the
#: composition's by more than the spread of its windows at every measured size.  Empty: see EXPERIMENTS part G.
COMPOSED_CELLS: set = set()
_COUNT_LIMIT = 1 << 31
_DTYPES = (torch.float32, torch.float64)

_entries = None


def _lib():
    global _entries
    if _entries is None:
        _entries = _engine.private_entries(_engine.COST_ENTRIES)
    return _entries


def max_segments() -> int:
    """Segments (tree levels) one cost launch takes (``mifwt_cost_max_segments``)."""
    return int(_lib().mifwt_cost_max_segments())


def short_limit(dtype: torch.dtype) -> int:
    """The longest node, in elements, that the short-node regime takes (``mifwt_cost_short_limit``)."""
    return int(_lib().mifwt_cost_short_limit(_engine._DTYPE_IDS[dtype]))


def chunk(dtype: torch.dtype) -> int:
    """Elements per unit of a long node (``mifwt_cost_chunk``)."""
    return int(_lib().mifwt_cost_chunk(_engine._DTYPE_IDS[dtype]))


# ---- arguments -----------------------------------------------------------------------------------------------------------------------
def _param(cost: str, p, value, what: str) -> float:
    """The one number the functional takes (0.0 where it takes none), after the checks."""
    if cost not in COSTS:
        raise ValueError(f"{what}: unknown cost {cost!r}; the costs are {', '.join(COSTS)}")

    def number(v, name):
        if not isinstance(v, numbers.Real) or isinstance(v, bool):
            raise ValueError(f"{what}: {name} must be a number, got {v!r}")
        return float(v)

    if cost == "norm":
        if value is not None:
            raise ValueError(f"{what}: cost 'norm' takes p, not value")
        if p is None:
            raise ValueError(f"{what}: cost 'norm' needs p >= 1")
        if not number(p, "p") >= 1.0 or math.isinf(p):
            raise ValueError(f"{what}: cost 'norm' needs a finite p >= 1, got {p!r}")
        return float(p)
    if p is not None:
        raise ValueError(f"{what}: cost {cost!r} takes no p")
    if cost in ("threshold", "sure"):
        if value is None:
            raise ValueError(f"{what}: cost {cost!r} needs value >= 0")
        if not number(value, "value") >= 0.0 or math.isinf(value):
            raise ValueError(f"{what}: cost {cost!r} needs a finite value >= 0, got {value!r}")
        return float(value)
    if value is not None:
        raise ValueError(f"{what}: cost {cost!r} takes no value")
    return 0.0


def _check_dtype(t: torch.Tensor, what: str) -> None:
    if t.dtype not in _DTYPES:
        raise ValueError(f"{what}: float32 and float64 data only, got {t.dtype}")


# ---- the composition -----------------------------------------------------------------------------------------------------------------
def _composed_costs(buf: torch.Tensor, nodes: int, cost: str, p=None, value=None) -> torch.Tensor:
    """The cost of each of the ``nodes`` equal parts of ``buf`` (in memory order) as float64 torch operations, shape ``[nodes]``.  The
    zero conventions are explicit — ``torch.where`` on an argument that is safe for the logarithm — so neither a value nor a gradient
    is NaN at an element that is exactly 0 (its gradient is 0, the limit of ``-2 t (ln t^2 + 1)``)."""
    t = buf.to(torch.float64).reshape(nodes, -1)
    if cost == "norm":
        terms = t.abs() if p == 1 else t * t if p == 2 else t.abs().pow(float(p))
        return terms.sum(-1)
    if cost == "threshold":
        return (t.abs() > value).sum(-1).to(torch.float64)
    t2 = t * t
    if cost == "sure":
        return (t.abs() > value).sum(-1).to(torch.float64) + torch.clamp(t2, max=float(value) * float(value)).sum(-1)
    nz = t2 > 0
    safe = torch.where(nz, t2, torch.ones_like(t2))
    if cost == "shannon":
        return -torch.where(nz, t2 * torch.log(safe), torch.zeros_like(t2)).sum(-1)
    if cost == "logenergy":
        return torch.where(nz, torch.log(safe), torch.zeros_like(t2)).sum(-1)
    raise ValueError(f"unknown cost {cost!r}")


# ---- the launch ------------------------------------------------------------------------------------------------------------------------
def _regime(dtype: torch.dtype, count: int) -> str:
    return "short" if count <= short_limit(dtype) else "long"


def _wants_grad(t: torch.Tensor) -> bool:
    return torch.is_grad_enabled() and t.requires_grad


def _costs_of(bufs: Sequence[torch.Tensor], leads: Sequence[int], ndim: int, cost: str, p, value, param: float) -> List[torch.Tensor]:
    """Per tensor of ``bufs`` one float64 tensor ``[nodes]``, a node being one index of the tensor's ``leads[i]`` leading axes.  Every
    tensor the kernel takes is a segment of ONE call (of one per ``max_segments()`` tensors); the others are composed."""
    outs: List[Optional[torch.Tensor]] = [None] * len(bufs)
    work = []
    for i, (t, lead) in enumerate(zip(bufs, leads)):
        nodes = math.prod(t.shape[:lead])
        count = t.numel() // nodes if nodes else 0
        if nodes == 0 or count == 0:  # nothing to launch: no nodes, or nodes that cost nothing
            outs[i] = torch.zeros(nodes, dtype=torch.float64, device=t.device)
            continue
        band = None
        if t.is_cuda and not _wants_grad(t) and (t.dtype, ndim, _regime(t.dtype, count)) not in COMPOSED_CELLS:
            band = _est._band(t.detach(), lead)
        if band is None:
            outs[i] = _composed_costs(t, nodes, cost, p, value)
        else:
            work.append((i, band, nodes))
    cap = max_segments() if work else 1
    for c0 in range(0, len(work), cap):
        run = work[c0:c0 + cap]
        k = len(run)
        anchor = run[0][1][0]
        dt = _engine._DTYPE_IDS[anchor.dtype]
        arr = (_engine.EstimBand * k)()
        res = torch.empty(sum(n for _, _, n in run), dtype=torch.float64, device=anchor.device)
        ptrs = (ctypes.c_void_p * k)()
        at = 0
        for j, (i, band, n) in enumerate(run):
            _est._fill(arr[j], band)
            outs[i] = res[at:at + n]
            ptrs[j] = res.data_ptr() + 8 * at
            at += n
        units = int(_lib().mifwt_cost_plan(dt, arr, k, None))
        if units < 0:
            _engine._check(units)
        _engine._run("cost_nodes", KID_COST_NODES, (k, at), anchor, _lib().mifwt_cost_nodes, (dt, COSTS[cost], param, arr, k, ptrs),
                     ws_bytes=8 * units)
    return outs  # type: ignore[return-value]


def wentropy(data: torch.Tensor, cost: str = "shannon", *, p=None, value=None, lead: int = 0) -> torch.Tensor:
    """The additive cost of ``data`` per index of its first ``lead`` axes (MATLAB's ``wentropy``): a float64 tensor of shape
    ``data.shape[:lead]`` on the data's device.  With ``t`` over the elements of one leading index, on the value converted to float64:

    ``"shannon"``    ``-sum t^2 ln t^2``; an element ``t == 0`` contributes 0.
    ``"logenergy"``  ``sum ln t^2``; an element ``t == 0`` contributes 0 (MATLAB's convention).
    ``"norm"``       ``sum |t|^p``, ``p >= 1``.
    ``"threshold"``  ``#{|t| > value}``, ``value >= 0``: an exact count, as float64.
    ``"sure"``       ``n - #{|t| <= value} + sum min(t^2, value^2)``.

    ``p`` and ``value`` are Python numbers.  float32 / float64 tensors; a view with a unit innermost stride is read as it is.  On a ROCm
    device the costs are one HIP launch (plus a small one that adds the chunks of long rows), summed in float64 in a fixed order — the
    same bits every time — with no host read, so a call can be captured.  A call on data that requires grad (while grad is enabled), on
    a CPU tensor, or beyond the kernel's index range is composed from float64 torch operations; the gradient at an exact 0 is 0.  An
    empty leading shape gives an empty result, an empty image 0.  Non-finite inputs are unspecified.  ``ValueError`` for an unknown
    cost, a missing, superfluous or out-of-range ``p`` / ``value``, complex, 16-bit, integer or bool data, ``lead`` outside
    ``[0, data.dim()]``, and 2^31 elements per leading index or more."""
    if not isinstance(data, torch.Tensor):
        raise TypeError(f"wentropy: expected a tensor, got {type(data).__name__}")
    param = _param(cost, p, value, "wentropy")
    _check_dtype(data, "wentropy")
    if not isinstance(lead, numbers.Integral) or isinstance(lead, bool) or not 0 <= lead <= data.dim():
        raise ValueError(f"wentropy: lead must be in [0, {data.dim()}], got {lead!r}")
    lead = int(lead)
    shape = tuple(data.shape[:lead])
    images = math.prod(shape)
    count = math.prod(data.shape[lead:])
    if count >= _COUNT_LIMIT:
        raise ValueError(f"wentropy: fewer than 2^31 elements per leading index, got {count}")
    return _costs_of([data], [lead], 0, cost, p, value, param)[0].reshape(shape)


# ---- trees -----------------------------------------------------------------------------------------------------------------------------
def _flat_levels(tree, maxlevel: Optional[int], what: str) -> Tuple[List[torch.Tensor], int]:
    """The level buffers 0 .. ``maxlevel`` of ``tree`` as ``[B, nb^s, extents..]``, expanded through ``__getitem__`` where missing."""
    if tree.maxlevel is None:
        tree[""]  # raises the reference's ValueError for an uninitialised tree
    top = tree.maxlevel if maxlevel is None else maxlevel
    if not isinstance(top, numbers.Integral) or isinstance(top, bool) or not 0 <= top <= tree.maxlevel:
        raise ValueError(f"{what}: maxlevel must be in [0, {tree.maxlevel}], got {maxlevel!r}")
    top = int(top)
    nd = tree._ndim
    bufs = []
    for s in range(top + 1):
        tree[tree._keys_of_level(s)[0]]
        buf = tree._level_buffer(s)
        bufs.append(buf.reshape(buf.shape[0], -1, *buf.shape[buf.dim() - nd:]))
    return bufs, top


def _level_costs(tree, cost, p, value, maxlevel, what: str) -> List[torch.Tensor]:
    """``[B, nb^s]`` float64 per level ``s = 0 .. maxlevel``: ONE call into the cost entry for all of them."""
    param = _param(cost, p, value, what)
    bufs, top = _flat_levels(tree, maxlevel, what)
    for b in bufs:
        _check_dtype(b, what)
    flat = _costs_of(bufs, [2] * len(bufs), tree._ndim, cost, p, value, param)
    return [c.reshape(b.shape[0], b.shape[1]) for c, b in zip(flat, bufs)]


def node_costs(self, cost: str = "shannon", *, p=None, value=None, maxlevel: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The cost (:func:`ptwt_amd.wentropy`) of every node of levels ``0 .. maxlevel`` (default: ``self.maxlevel``), the root ``""``
    included: ``{key: float64 tensor of the leading shape}`` — the input's shape without its transformed axes.  The tree is expanded
    down to ``maxlevel`` first; nodes assigned by the user count as assigned.  On a ROCm device the costs of ALL levels are one HIP
    launch, every level a segment of its table; the entries of the dict are views of one ``[B, nb^s]`` tensor per level.  No host
    read: the call can be captured.  On a tree whose nodes require grad the costs are composed and differentiable."""
    costs = _level_costs(self, cost, p, value, maxlevel, "node_costs")
    lead = list(self._layout.lead)
    out: Dict[str, torch.Tensor] = {}
    for s, c in enumerate(costs):  # (one unbind per level: a deep 1-D level has hundreds of nodes)
        out.update(zip(self._keys_of_level(s), c.reshape(lead + [c.shape[-1]]).unbind(-1)))
    return out


def _prune(costs: Sequence[torch.Tensor]) -> Tuple[List[torch.Tensor], List[torch.Tensor]]:
    """The Coifman-Wickerhauser search on cost tables ``costs[s]`` of shape ``[.., nb^s]``, ``s = 0 .. J`` (the children of node ``j``
    of level ``s`` are nodes ``nb j .. nb j + nb - 1`` of level ``s + 1``): (the bool masks of the selected nodes per level, the cost
    of the best basis below every node per level).  Bottom-up a parent is kept where its cost is no larger than the sum of its
    children's best costs — a tie keeps the parent —, the children added left to right; top-down a node is selected where it is kept
    and no ancestor was.  Plain torch operations on any device, no host read."""
    top = len(costs) - 1
    nb = costs[1].shape[-1] // costs[0].shape[-1] if top else 1
    best: List[Optional[torch.Tensor]] = [None] * (top + 1)
    keep: List[Optional[torch.Tensor]] = [None] * (top + 1)
    best[top] = costs[top]
    keep[top] = torch.ones_like(costs[top], dtype=torch.bool)
    for s in range(top - 1, -1, -1):
        ch = best[s + 1].reshape(*costs[s].shape, nb)
        sumc = ch[..., 0] + ch[..., 1]
        for j in range(2, nb):
            sumc = sumc + ch[..., j]
        keep[s] = costs[s] <= sumc
        best[s] = torch.where(keep[s], costs[s], sumc)
    sel: List[torch.Tensor] = []
    opened = torch.ones_like(keep[0])
    for s in range(top + 1):
        sel.append(opened & keep[s])
        if s < top:
            opened = (opened & ~keep[s]).repeat_interleave(nb, -1)
    return sel, best  # type: ignore[return-value]


def best_basis(self, cost: str = "shannon", *, p=None, value=None, maxlevel: Optional[int] = None, joint: bool = True):
    """The basis of the tree that minimises the additive ``cost`` (:func:`ptwt_amd.wentropy`) among all bases of levels
    ``0 .. maxlevel``: a parent is kept wherever it is no more expensive than the best basis of its children.  Every path from the root
    to a node of ``maxlevel`` holds exactly one selected node.

    ``joint=True``: ONE basis for the whole batch, on the node costs summed over all leading indices; returns the list of its keys in
    depth-first band order.  This form copies the selection masks (a few bytes per node) to the host — the only host read of the
    feature — and therefore synchronises and cannot be captured.

    ``joint=False``: one basis per leading index; returns a list of bool device tensors, ``masks[s]`` of shape ``[*lead, nb^s]`` for
    ``s = 0 .. maxlevel``, a node being selected where its entry is true.  The node order is that of the level buffer: the keys over the
    alphabet in band order, which is ``get_level(s, "natural")`` for ``WaveletPacket`` and for ``WaveletPacket2D(separable=True)``
    (``get_natural_order(s)``); a non-separable ``WaveletPacket2D`` orders its alphabet ``a, v, h, d`` (``basis_keys(s)`` names the
    order in every case).  No host read: the call can be captured."""
    costs = _level_costs(self, cost, p, value, maxlevel, "best_basis")
    if not joint:
        sel, _ = _prune(costs)
        lead = list(self._layout.lead)
        return [m.reshape(lead + [m.shape[-1]]) for m in sel]
    sel, _ = _prune([c.sum(0) for c in costs])
    chosen = [m.tolist() for m in torch.cat(sel).cpu().split([m.shape[0] for m in sel])]
    chars = sorted(self._bands, key=self._bands.get)
    nb = len(chars)
    keys: List[str] = []

    def walk(key: str, j: int) -> None:
        if chosen[len(key)][j]:
            keys.append(key)
        elif len(key) < len(chosen) - 1:
            for i, c in enumerate(chars):
                walk(key + c, nb * j + i)

    walk("", 0)
    return keys


def basis_keys(self, level: int) -> List[str]:
    """The keys of ``level`` in the order of the masks of ``best_basis(joint=False)``: the order of the level buffer."""
    return self._keys_of_level(level)


def _check_cover(self, keys: Sequence[str]) -> int:
    """``keys`` must be an admissible cover: every path from the root to the deepest level meets exactly one key.  Returns that level."""
    if len(keys) == 0:
        raise ValueError("reconstruct_basis: an empty basis covers no path")
    for k in keys:
        if not isinstance(k, str) or any(c not in self._filter_keys for c in k):
            raise ValueError(f"reconstruct_basis: invalid key {k!r}; all chars of a key must be of the set {self._filter_keys}")
    have = set(keys)
    if len(have) != len(keys):
        dup = next(k for k in keys if list(keys).count(k) > 1)
        raise ValueError(f"reconstruct_basis: the path {dup!r} meets the key {dup!r} twice")
    top = max(len(k) for k in keys)
    for k in keys:
        for cut in range(len(k)):
            if k[:cut] in have:
                raise ValueError(f"reconstruct_basis: the path {k!r} meets two keys, {k[:cut]!r} and {k!r}")
    chars = sorted(self._bands, key=self._bands.get)

    def walk(key: str) -> None:
        if key in have:
            return
        if len(key) == top:
            raise ValueError(f"reconstruct_basis: the path {key!r} meets no key of the basis")
        for c in chars:
            walk(key + c)

    walk("")
    return top


def reconstruct_basis(self, basis):
    """Rebuild the root from exactly the nodes of ``basis`` as the tree holds them, values assigned by the user included; whatever lies
    below a basis node is ignored.  Returns ``self``, as ``reconstruct()`` does; the root is ``self[""]``, and every inner node above
    the basis is rebuilt on the way.

    ``basis`` is a list of keys — an admissible cover: every path from the root to the deepest key meets exactly one key, or
    ``ValueError`` names the offending path — or the list of masks of ``best_basis(joint=False)``.  Masks live on the device and are
    NOT validated: a list that is no cover gives a root that mixes nodes and rebuilt values.

    The level-by-level synthesis of ``reconstruct()`` runs bottom-up from the deepest level of the basis, one launch per level over
    all nodes; after a level is rebuilt the basis nodes of that level take the place of their rebuilt counterparts (index assignment
    for keys, ``torch.where`` for masks) before the next level is formed.  Levels below the basis that the tree does not hold yet are
    expanded first; their values do not matter.  Differentiable wherever ``reconstruct()`` is.  A root that comes out one sample
    longer than the input (odd extents outside ``mode="periodization"``, as in ``reconstruct()``) is cropped to the input's extents
    where the masks select the root for some images."""
    if self.maxlevel is None:
        self[""]  # raises the reference's ValueError for an uninitialised tree
    if not isinstance(basis, (list, tuple)):
        raise TypeError(f"reconstruct_basis: expected a list of keys or of masks, got {type(basis).__name__}")
    masks = len(basis) > 0 and all(isinstance(m, torch.Tensor) for m in basis)
    top = len(basis) - 1 if masks else _check_cover(self, basis)
    if top > self.maxlevel:
        raise KeyError(f"The requested level {top} is too large! This wavelet packet tree is initialized with maximum level {self.maxlevel}.")
    nd, lead = self._ndim, len(self._layout.lead)
    by_level: Dict[int, List[str]] = {}
    if masks:
        for s, m in enumerate(basis):
            if m.dtype != torch.bool or m.dim() != lead + 1 or m.shape[-1] != len(self._bands) ** s:
                raise ValueError(f"reconstruct_basis: mask {s} must be a bool tensor [*lead, {len(self._bands) ** s}], got {m.dtype} "
                                 f"{tuple(m.shape)}")
    else:
        for k in basis:
            by_level.setdefault(len(k), []).append(k)
    for s in range(top + 1):
        self[self._keys_of_level(s)[0]]
    # the basis nodes as the tree holds them now: the synthesis replaces the levels it rebuilds
    held = {s: self._level_buffer(s) for s in range(top) if masks or s in by_level}

    def override(level: int, buf: torch.Tensor) -> torch.Tensor:
        if level not in held:
            return buf
        mine = held[level]
        if masks:
            if mine.shape != buf.shape:  # (the root, one sample longer than the input)
                buf = buf[tuple(slice(0, n) for n in mine.shape)]
            m = basis[level].reshape(buf.shape[0], *buf.shape[1:1 + level], *([1] * nd))
            return torch.where(m, mine, buf)
        if level == 0:
            return mine
        buf = buf.clone()
        for k in by_level[level]:
            idx = (slice(None),) + self._band_path(k)
            buf[idx] = mine[idx]
        return buf

    if top == 0:
        return self
    if self._banks is not None:
        return self._reconstruct_boundary(top, override)
    if self._periodized:
        return self._reconstruct_periodized(top, override)
    return self._reconstruct_padded(top, override)


_packets._PacketTree.node_costs = node_costs
_packets._PacketTree.best_basis = best_basis
_packets._PacketTree.basis_keys = basis_keys
_packets._PacketTree.reconstruct_basis = reconstruct_basis
