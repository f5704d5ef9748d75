"""Float64 reference of the best-basis feature (ptwt_amd/best_basis.py), written from the formulas and from nothing of the package:

    terms / cost / cost_bound      the five additive functionals on one node: float64 terms, summed with ``math.fsum``, and the bound
                                   ``(n + 64) 2^-53 sum |term_i|`` a float64 evaluation in any order must stay inside
    prune                          the Coifman-Wickerhauser pruning with Python loops over nodes: (selection masks, best costs)
    bases / basis_total / brute    every admissible basis of a tree of depth <= 2 (5 in 1-D, 17 in 2-D), its total, the minimum
    partial_synthesis              the root rebuilt from exactly the nodes of a basis, recursively, on the level maps of
                                   tests/_packet_ref.py (padded modes), tests/_per_ref.py and tests/_boundary_ref.py

A cost table is a list ``c[s]`` of ``nb^s`` numbers; the children of node ``j`` of level ``s`` are ``nb j .. nb j + nb - 1`` of level
``s + 1``.  A tie keeps the parent; children are added left to right."""
import math

import numpy as np
import torch

from tests import _packet_ref as R

COSTS = ("shannon", "logenergy", "norm", "threshold", "sure")
U = 2.0 ** -53


def terms(x, cost, p=None, value=None):
    """(the float64 terms that are summed, the integer part that is counted) of the node ``x``."""
    t = np.asarray(x, dtype=np.float64).reshape(-1)
    t2 = t * t
    nz = t2 > 0
    safe = np.where(nz, t2, 1.0)
    if cost == "shannon":
        return np.where(nz, -t2 * np.log(safe), 0.0), 0
    if cost == "logenergy":
        return np.where(nz, np.log(safe), 0.0), 0
    if cost == "norm":
        a = np.abs(t)
        return (a if p == 1 else t2 if p == 2 else a ** float(p)), 0
    if cost == "threshold":
        return np.zeros(0), int((np.abs(t) > value).sum())
    if cost == "sure":
        return np.minimum(t2, float(value) * float(value)), int((np.abs(t) > value).sum())
    raise ValueError(cost)


def cost(x, cost_name, p=None, value=None):
    s, c = terms(x, cost_name, p, value)
    return math.fsum(s.tolist()) + c


def cost_bound(x, cost_name, p=None, value=None):
    """``(n + 64) 2^-53 sum |term_i|``: 0 for the exact count of ``"threshold"``; ``"sure"`` counts its indicator terms in."""
    s, c = terms(x, cost_name, p, value)
    if cost_name == "threshold":
        return 0.0
    return (np.asarray(x).size + 64) * U * (math.fsum(np.abs(s).tolist()) + c)


def costs(x, cost_name, p=None, value=None, lead=1):
    """(costs, bounds) per index of the first ``lead`` axes of ``x`` (numpy float64 arrays of the leading shape)."""
    x = np.asarray(x)
    shape = x.shape[:lead]
    flat = x.reshape(int(np.prod(shape, dtype=np.int64)), -1)
    c = np.array([cost(r, cost_name, p, value) for r in flat], dtype=np.float64).reshape(shape)
    b = np.array([cost_bound(r, cost_name, p, value) for r in flat], dtype=np.float64).reshape(shape)
    return c, b


# ---- pruning ---------------------------------------------------------------------------------------------------------------------------
def prune(table):
    """``table[s]``: ``nb^s`` floats.  Returns (sel, best): lists per level of bools / floats."""
    top = len(table) - 1
    nb = len(table[1]) // len(table[0]) if top else 1
    best = [None] * (top + 1)
    keep = [None] * (top + 1)
    best[top] = [float(v) for v in table[top]]
    keep[top] = [True] * len(table[top])
    for s in range(top - 1, -1, -1):
        best[s], keep[s] = [], []
        for j, c in enumerate(table[s]):
            sumc = best[s + 1][nb * j] + best[s + 1][nb * j + 1]
            for i in range(2, nb):
                sumc = sumc + best[s + 1][nb * j + i]
            k = float(c) <= sumc
            keep[s].append(k)
            best[s].append(float(c) if k else sumc)
    sel = []
    opened = [True]
    for s in range(top + 1):
        sel.append([o and k for o, k in zip(opened, keep[s])])
        opened = [o and not k for o, k in zip(opened, keep[s]) for _ in range(nb)]
    return sel, best


def bases(nb, depth):
    """Every admissible basis of a full tree of ``depth`` levels: lists of (level, index)."""
    def below(s, j):
        out = [[(s, j)]]
        if s < depth:
            parts = [[]]
            for i in range(nb):
                parts = [a + b for a in parts for b in below(s + 1, nb * j + i)]
            out += parts
        return out
    return below(0, 0)


def basis_total(table, basis):
    return math.fsum(float(table[s][j]) for s, j in basis)


def tree_total(table, basis):
    """The total of a basis added in the order of the tree: a node of the basis counts itself, any other node the totals of its
    children, left to right — the order of :func:`prune`, so the chosen basis' total is ``best[0][0]`` to the bit."""
    have = set(basis)
    nb = len(table[1]) // len(table[0]) if len(table) > 1 else 1

    def below(s, j):
        if (s, j) in have:
            return float(table[s][j])
        tot = below(s + 1, nb * j) + below(s + 1, nb * j + 1)
        for i in range(2, nb):
            tot = tot + below(s + 1, nb * j + i)
        return tot
    return below(0, 0)


def brute(table):
    """(the smallest total over every admissible basis, the number of bases)."""
    nb = len(table[1]) // len(table[0]) if len(table) > 1 else 1
    all_ = bases(nb, len(table) - 1)
    return min(basis_total(table, b) for b in all_), len(all_)


def is_cover(sel):
    """Every root-to-leaf path of the mask lists ``sel`` holds exactly one selected node."""
    top = len(sel) - 1
    nb = len(sel[1]) // len(sel[0]) if top else 1
    for leaf in range(len(sel[top])):
        if sum(bool(sel[s][leaf // nb ** (top - s)]) for s in range(top + 1)) != 1:
            return False
    return True


# ---- partial-tree synthesis -------------------------------------------------------------------------------------------------------------
def _crop(ext, held):
    """A parent that comes out one sample longer than the node the tree holds for it loses its last sample; the root (``held`` None)
    is taken as it comes out (the rule of ``_packet_ref.reconstruct``)."""
    if held is not None:
        for a in range(len(ext)):
            if ext[a] != held[a]:
                assert ext[a] == held[a] + 1, "padding error"
                ext[a] = int(held[a])
    return ext


def padded_inv(bank, ndim, separable=False):
    """One synthesis level of the padded modes on the level maps of tests/_packet_ref.py: ({char: child}, held extents) -> parent."""
    bank, table = R.bank_of(bank), R.key_table(ndim, separable)
    flen = len(bank[2])

    def inv(kids, held):
        ext = _crop([2 * m - flen + 2 for m in kids["a"].shape[-ndim:]], held)
        return R.level_inv({table[c]: t for c, t in kids.items()}, bank, ndim, ext)
    return inv


def periodized_inv(bank, ndim, band_of):
    """The same on tests/_per_ref.py; ``band_of``: key char -> band index of the level buffer."""
    from tests import _per_ref as P

    def inv(kids, held):
        ext = _crop([2 * m for m in kids["a"].shape[-ndim:]], held)
        return P.level_inv([kids[c] for c in sorted(kids, key=band_of.get)], bank, ndim, ext)
    return inv


def boundary_inv(taps):
    """The same for a 1-D boundary-wavelet tree on tests/_boundary_ref.py (float64)."""
    from tests import _boundary_ref as B

    def inv(kids, held):
        ext = _crop([2 * kids["a"].shape[-1]], held)
        return B.transposed_level([kids["a"], kids["d"]], taps, "synthesis", tuple(ext))
    return inv


def partial_synthesis(tree, basis, inv, chars, ndim):
    """The root rebuilt, recursively, from exactly the nodes ``tree[key]`` for ``key`` in ``basis`` (tensors ``[batch, extents..]``; the
    arithmetic runs in their dtype).  ``tree`` also holds every inner node above the basis, for the crops; nothing else of it is read."""
    have = set(basis)

    def build(key):
        if key in have:
            return tree[key]
        kids = {c: build(key + c) for c in chars}
        return inv(kids, None if key == "" else tuple(tree[key].shape[-ndim:]))

    return build("")


def keys_of(sel, keys_of_level):
    """The keys a mask list selects, level by level."""
    return [k for s, m in enumerate(sel) for k, on in zip(keys_of_level(s), m) if on]


def as_table(level_costs):
    """A list of 1-D float64 tensors / arrays as a table of Python floats."""
    return [[float(v) for v in (c.tolist() if isinstance(c, torch.Tensor) else c)] for c in level_costs]
