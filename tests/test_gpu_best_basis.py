"""GPU tests (``-m gpu``) of ``wentropy`` and of ``node_costs`` / ``best_basis`` / ``reconstruct_basis`` of the packet trees: the cost kernels
(ids 61 / 62, csrc/mifwt_cost.hip) against the ``math.fsum`` reference of tests/_best_basis_ref.py in both regimes and at every node
length at which the kernel takes another path, the trees key by key, the pruning against the reference pruning of the device's own
costs and against a brute force over every basis, the reconstruction from a basis against the reference's recursive partial-tree
synthesis, gradients, graph capture, reproducibility, canaries around ``out`` and the workspace, and one cell past 2^31 elements.

Tolerance of a cost (derived, not tuned): ``|got - ref| <= (n + 64) 2^-53 sum |term_i|`` per node of ``n`` elements.  A float64 sum in
any order errs by at most ``(n - 1) u sum |term|``; the products by a few ``u``; ``log`` and ``pow`` by OpenCL's 3 and 16 ulp, which the
ROCm device library is to meet; the reference's terms are rounded themselves: 64 covers them.  ``"threshold"`` must match exactly;
``"sure"`` is held to the bound with its indicator terms counted in, and to exactness where ``value = 0`` leaves only the count.

Reconstruction: norm-wise 1e-12 in float64; in float32 ``max(1e-6, 10 e_ref32)``, e_ref32 the deviation of the reference's float32 run
from its float64 run on the same values (the rule of tests/test_gpu_packets.py).

Measured on an MI355X (a record, not a bound; ``check`` prints the ratio of every comparison): the worst cost error is 0.035 of its
bound (a level of the 1-D boundary tree; 0.030 for ``"norm"`` at n = 1 and 2, where the bound is tightest).  118 tests: 3.7 s."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, best_basis as BB
from ptwt_amd._wavelets import host_taps
from tests import _best_basis_ref as R
from tests import _packet_ref as PR

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
PARAMS = {"shannon": {}, "logenergy": {}, "norm": {"p": 1.5}, "threshold": {"value": 0.7}, "sure": {"value": 0.7}}


def dev():
    return torch.device("cuda:0")


def tag(v):
    return str(v).split(".")[-1] if isinstance(v, torch.dtype) else str(v)


def lengths(dtype):
    lim, ch = BB.short_limit(dtype), BB.chunk(dtype)
    return [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, lim - 1, lim, lim + 1, ch, ch + 1, 2 * ch + 3]


@functools.lru_cache(maxsize=None)
def node_data(dtype, n):
    """7 nodes of ``n`` elements with exact zeros sprinkled in: for odd ``n`` the node starts visit every 4-byte phase of a 16-byte line."""
    g = torch.Generator().manual_seed(1000 + n)
    x = torch.randn(7, n, generator=g, dtype=F64).to(dtype)
    x[torch.rand(7, n, generator=g) < 0.1] = 0.0
    x[3, 0] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def node_ref(dtype, n, cost):
    return R.costs(node_data(dtype, n).double().numpy(), cost, **PARAMS[cost])


def check(got, want, bound, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    err = np.abs(got - want)
    print("%s: worst error / bound %.3f" % (what, float((err / np.where(bound > 0, bound, 1.0)).max())))
    assert np.all(err <= bound), (what, float(err.max()), float(bound.min()))


# ---- the kernel against the reference --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", R.COSTS)
@pytest.mark.parametrize("dtype", [F32, F64], ids=tag)
def test_kernel_against_the_reference(dtype, cost):
    for n in lengths(dtype):
        x = node_data(dtype, n)
        want, bound = node_ref(dtype, n, cost)
        check(ptwt_amd.wentropy(x.to(dev()), cost, lead=1, **PARAMS[cost]), want, bound, "%s %s n=%d" % (cost, tag(dtype), n))


@pytest.mark.parametrize("dtype", [F32, F64], ids=tag)
def test_norms_without_pow_and_the_exact_counts(dtype):
    for n in (5, 257, BB.short_limit(dtype) + 1):
        x = node_data(dtype, n)
        for p in (1, 2, 3):
            want, bound = R.costs(x.double().numpy(), "norm", p=p)
            check(ptwt_amd.wentropy(x.to(dev()), "norm", p=p, lead=1), want, bound, "norm p=%d n=%d" % (p, n))
        got = ptwt_amd.wentropy(x.to(dev()), "sure", value=0.0, lead=1)  # only the count is left: exact
        assert got.cpu().tolist() == [float((r != 0).sum()) for r in x]
        got = ptwt_amd.wentropy(x.to(dev()), "threshold", value=0.0, lead=1)
        assert got.cpu().tolist() == [float((r != 0).sum()) for r in x]


@pytest.mark.parametrize("cost", R.COSTS)
@pytest.mark.parametrize("dtype", [F32, F64], ids=tag)
def test_planes_pitched_views_and_leads(dtype, cost):
    g = torch.Generator().manual_seed(77)
    x = torch.randn(5, 33, 35, generator=g, dtype=F64).to(dtype)
    x[:, ::4, ::3] = 0.0
    want, bound = R.costs(x.double().numpy(), cost, **PARAMS[cost])
    check(ptwt_amd.wentropy(x.to(dev()), cost, lead=1, **PARAMS[cost]), want, bound, "plane")
    buf = torch.randn(5, 9, 40, generator=g, dtype=F64).to(dtype)
    view = buf.to(dev())[:, :, :33]
    assert not view.is_contiguous()
    want, bound = R.costs(buf[:, :, :33].double().numpy(), cost, **PARAMS[cost])
    check(ptwt_amd.wentropy(view, cost, lead=1, **PARAMS[cost]), want, bound, "pitched view")
    want2, bound2 = R.costs(buf[:, :, :33].double().numpy(), cost, lead=2, **PARAMS[cost])
    check(ptwt_amd.wentropy(view, cost, lead=2, **PARAMS[cost]), want2, bound2, "pitched view, lead=2")
    want0, bound0 = R.costs(buf[:, :, :33].double().numpy(), cost, lead=0, **PARAMS[cost])
    check(ptwt_amd.wentropy(view, cost, **PARAMS[cost]), want0, bound0, "pitched view, lead=0")
    t = buf.to(dev()).transpose(1, 2)  # no unit innermost stride: read from a contiguous copy
    want, bound = R.costs(buf.transpose(1, 2).double().numpy(), cost, **PARAMS[cost])
    check(ptwt_amd.wentropy(t, cost, lead=1, **PARAMS[cost]), want, bound, "transposed")


def test_empty_shapes_on_the_device():
    assert ptwt_amd.wentropy(torch.zeros(0, 5, device=dev()), lead=1).shape == (0,)
    e = ptwt_amd.wentropy(torch.zeros(3, 0, device=dev()), "sure", value=1.0, lead=1)
    assert e.device.type == "cuda" and e.cpu().tolist() == [0.0, 0.0, 0.0]


# ---- trees ---------------------------------------------------------------------------------------------------------------------------------
#: (name, ndim, shape, wavelet, mode, depth, keyword arguments of the class)
TREES = [
    ("haar64", 1, (3, 64), "haar", "zero", 6, {}),  # leaves of one sample
    ("sym67", 1, (3, 67), "db2", "symmetric", 3, {}),
    ("per50", 1, (3, 50), "db2", "periodization", 3, {}),  # nodes of 25 / 13 / 7
    ("bnd64", 1, (3, 64), "db2", "boundary", 3, {}),
    ("reflect2d", 2, (3, 33, 35), "db2", "reflect", 2, {"separable": False}),
    ("reflect2d-sep", 2, (3, 33, 35), "db2", "reflect", 2, {"separable": True}),
    ("per2d", 2, (3, 33, 35), "db2", "periodization", 2, {"separable": False}),
]
TREE_IDS = [t[0] for t in TREES]


def make_tree(t, dtype, seed=0, requires_grad=False):
    _, ndim, shape, wavelet, mode, depth, kw = t
    g = torch.Generator().manual_seed(500 + seed)
    x = torch.randn(*shape, generator=g, dtype=F64).to(dtype).to(dev())
    x.requires_grad_(requires_grad)
    cls = ptwt_amd.WaveletPacket if ndim == 1 else ptwt_amd.WaveletPacket2D
    return cls(x, wavelet, mode=mode, maxlevel=depth, **kw), x


def level_table(wp, costs, depth):
    """node_costs as [B, nb^s] float64 CPU tensors in the order of the level buffer."""
    return [torch.stack([costs[k] for k in wp._keys_of_level(s)], -1).cpu() for s in range(depth + 1)]


@pytest.mark.parametrize("cost", ["shannon", "sure"])
@pytest.mark.parametrize("dtype", [F32, F64], ids=tag)
@pytest.mark.parametrize("t", TREES, ids=TREE_IDS)
def test_node_costs_of_trees(t, dtype, cost):
    wp, x = make_tree(t, dtype)
    depth = t[5]
    _engine.level_events = []
    try:
        costs = wp.node_costs(cost, **PARAMS[cost])
        seen = [e[1] for e in _engine.level_events if e[0] == "cost_nodes"]
    finally:
        _engine.level_events = None
    assert seen == [61], "the costs of all levels are one call"
    keys = [k for s in range(depth + 1) for k in wp._keys_of_level(s)]
    assert list(costs) == keys and len(keys) == sum(len(wp._bands) ** s for s in range(depth + 1))
    for s in range(depth + 1):  # one stacked comparison per level: the nodes the tree itself returns
        ks = wp._keys_of_level(s)
        nodes = torch.stack([wp[k] for k in ks], 1).double().cpu().numpy()  # [B, nodes, extents..]
        want, bound = R.costs(nodes, cost, lead=2, **PARAMS[cost])
        got = torch.stack([costs[k] for k in ks], 1)
        assert all(costs[k].shape == (3,) and costs[k].dtype == F64 for k in ks)
        check(got, want, bound, "%s level %d" % (t[0], s))
    # a part of the tree: the same values
    part = wp.node_costs(cost, maxlevel=1, **PARAMS[cost])
    assert list(part) == keys[:1 + len(wp._bands)] and all(torch.equal(part[k], costs[k]) for k in part)


@pytest.mark.parametrize("t", [TREES[1], TREES[4], TREES[5]], ids=[TREES[1][0], TREES[4][0], TREES[5][0]])
def test_mask_order_is_the_documented_key_order(t):
    wp, _ = make_tree(t, F32)
    depth, ndim = t[5], t[1]
    for s in range(depth + 1):
        if ndim == 1:
            assert wp.basis_keys(s) == wp.get_level(s, "natural")
        elif wp.separable:
            assert wp.basis_keys(s) == wp.get_level(s, "natural") == wp.get_natural_order(s)
        else:
            assert wp.basis_keys(s) == ["".join(p) for p in itertools.product("avhd", repeat=s)]
    # the masks, read through that key order, select the nodes the reference pruning selects by key
    costs = wp.node_costs("norm", p=2)
    keys = wp.basis_keys(depth)
    masks = wp.best_basis("norm", p=2, joint=False)
    table = level_table(wp, costs, depth)
    for i in range(3):
        sel = R.prune(R.as_table([c[i] for c in table]))[0]
        for s in range(depth + 1):
            got = {k for k, on in zip(wp.basis_keys(s), masks[s][i].cpu().tolist()) if on}
            assert got == {k for k, on in zip(wp.basis_keys(s), sel[s]) if on}
    assert len(keys) == masks[depth].shape[-1]


@pytest.mark.parametrize("t", [TREES[1], TREES[4]], ids=[TREES[1][0], TREES[4][0]])
def test_an_assigned_node_changes_exactly_its_own_cost(t):
    wp, _ = make_tree(t, F32)
    depth = t[5]
    before = wp.node_costs("shannon")
    key = wp._keys_of_level(depth - 1)[1]
    wp[key] = 3.0 * wp[key]
    after = wp.node_costs("shannon")
    for k in before:
        assert torch.equal(before[k], after[k]) == (k != key), k
    want, bound = R.costs(wp[key].double().cpu().numpy(), "shannon", lead=1)
    check(after[key], want, bound, "assigned node")


# ---- pruning on the device -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", ["shannon", "norm", "threshold"])
@pytest.mark.parametrize("t", TREES, ids=TREE_IDS)
def test_masks_are_the_reference_pruning_of_the_device_costs(t, cost):
    wp, _ = make_tree(t, F32)
    depth = t[5]
    table = level_table(wp, wp.node_costs(cost, **PARAMS[cost]), depth)
    masks = wp.best_basis(cost, joint=False, **PARAMS[cost])
    assert [tuple(m.shape) for m in masks] == [(3, len(wp._bands) ** s) for s in range(depth + 1)]
    assert all(m.dtype == torch.bool and m.is_cuda for m in masks)
    for i in range(3):
        sel, _ = R.prune(R.as_table([c[i] for c in table]))
        got = [m[i].cpu().tolist() for m in masks]
        assert got == sel, (t[0], i)
        assert R.is_cover(got)


@pytest.mark.parametrize("cost", ["shannon", "logenergy", "norm"])
@pytest.mark.parametrize("t", [("d2-1d", 1, (3, 67), "db2", "symmetric", 2, {}), ("d2-2d", 2, (3, 33, 35), "db2", "reflect", 2, {})],
                         ids=["1d", "2d"])
def test_the_chosen_basis_is_optimal(t, cost):
    wp, _ = make_tree(t, F32)
    nb = len(wp._bands)
    table = level_table(wp, wp.node_costs(cost, **PARAMS[cost]), 2)
    masks = wp.best_basis(cost, joint=False, **PARAMS[cost])
    all_bases = R.bases(nb, 2)
    assert len(all_bases) == (5 if nb == 2 else 17)
    for i in range(3):
        tab = R.as_table([c[i] for c in table])
        chosen = [(s, j) for s, m in enumerate(masks) for j, on in enumerate(m[i].cpu().tolist()) if on]
        # totals in the order of the tree (children left to right, level by level): float64 addition is monotone, so no basis is
        # cheaper than the chosen one — with no slack
        assert all(R.tree_total(tab, chosen) <= R.tree_total(tab, b) for b in all_bases), (t[0], i)
    keys = wp.best_basis(cost, **PARAMS[cost])
    joint = R.as_table([c.sum(0) for c in table])
    index = {k: (s, j) for s in range(3) for j, k in enumerate(wp._keys_of_level(s))}
    slack = 1e-12 * sum(abs(v) for row in joint for v in row)
    assert all(R.basis_total(joint, [index[k] for k in keys]) <= R.basis_total(joint, b) + slack for b in all_bases)
    assert BB._check_cover(wp, keys) <= 2  # the joint basis is an admissible cover, in depth-first band order
    order = sorted(wp._bands, key=wp._bands.get)
    assert keys == sorted(keys, key=lambda k: [order.index(c) for c in k])


# ---- reconstruct_basis ---------------------------------------------------------------------------------------------------------------------
#: (name, ndim, shape, wavelet, mode, depth, class keywords): odd extents, the three mode families
REC = [
    ("sym1d", 1, (2, 67), "db2", "symmetric", 3, {}),
    ("per1d", 1, (2, 51), "db2", "periodization", 3, {}),
    ("bnd1d", 1, (2, 67), "db2", "boundary", 3, {}),
    ("sym2d", 2, (2, 33, 35), "db2", "symmetric", 2, {"separable": False}),
    ("per2d", 2, (2, 33, 35), "db2", "periodization", 2, {"separable": True}),
]
REC_IDS = [t[0] for t in REC]


def some_bases(wp, depth):
    """A few admissible bases: the root's children, the leaves, and two mixed ones."""
    chars = sorted(wp._bands, key=wp._bands.get)
    mixed = [chars[0] + c for c in chars] + chars[1:]  # the first child split once
    out = [list(chars), wp._keys_of_level(depth), mixed]
    if depth >= 3:
        out.append([chars[0]] + [chars[1] + c for c in chars[:1]] + [chars[1] + chars[1] + c for c in chars])  # a, da, dda, ddd
    return out


def ref_inv(t, wp, dtype):
    _, ndim, _, wavelet, mode, _, kw = t
    if mode == "boundary":
        return R.boundary_inv(host_taps(wavelet))
    if mode == "periodization":
        return R.periodized_inv(host_taps(wavelet), ndim, wp._bands)
    return R.padded_inv(wavelet, ndim, kw.get("separable", False))


def rel(got, want):
    got, want = got.double().cpu(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).norm() / want.norm())


def held_nodes(wp, depth):
    """Every node of levels 0 .. depth as the tree holds it, folded to [B, extents..], on the CPU."""
    wp[wp._keys_of_level(depth)[0]]
    return {k: wp._layout.fold(wp[k]).detach().cpu() for s in range(depth + 1) for k in wp._keys_of_level(s)}


def synth_tol(tree64, basis, t, wp, chars, want):
    """float32 bound of a partial-tree synthesis: ``max(1e-6, 10 e_ref32)``, e_ref32 the reference's own float32 run against ``want``."""
    tree32 = {k: v.float() for k, v in tree64.items()}
    return max(1e-6, 10 * rel(R.partial_synthesis(tree32, basis, ref_inv(t, wp, F32), chars, t[1]), want))


@pytest.mark.parametrize("dtype", [F32, F64], ids=tag)
@pytest.mark.parametrize("t", REC, ids=REC_IDS)
def test_untouched_tree_round_trips_from_any_basis(t, dtype):
    """float64: the input comes back at 1e-12 from every basis.  float32, padded modes: at the bound tests/test_gpu_packets.py has for
    the root after ``reconstruct()``, ``max(1e-6, 10 e_ref32)``; the other two families, whose references have no float32 tree, against
    the float64 synthesis of the nodes the device's tree holds, at the float32 bound of that synthesis."""
    _, ndim, shape, wavelet, mode, depth, kw = t
    wp, x = make_tree(t, dtype)
    chars = sorted(wp._bands, key=wp._bands.get)
    padded = mode not in ("periodization", "boundary")
    if dtype == F32 and padded:
        e32 = PR.e_ref32(x.cpu(), wavelet, mode, depth, ndim, kw.get("separable", False))["inv0"][0][0]
    masks = wp.best_basis("shannon", joint=False)
    for basis in some_bases(wp, depth) + [[""], masks]:
        wp, x = make_tree(t, dtype)
        held = held_nodes(wp, depth)
        assert wp.reconstruct_basis(basis) is wp
        root = wp[""]
        assert all(0 <= a - b <= 1 for a, b in zip(root.shape, x.shape))  # (an odd extent may come back one sample longer)
        crop = root[tuple(slice(0, n) for n in x.shape)]
        if dtype == F64:
            assert rel(crop, x.cpu()) <= 1e-12, (t[0], basis)
        elif padded:
            assert rel(crop, x.cpu()) <= max(1e-6, 10 * e32), (t[0], basis, rel(crop, x.cpu()), e32)
        elif basis is not masks and basis != [""]:
            tree64 = {k: v.double() for k, v in held.items()}
            want = R.partial_synthesis(tree64, basis, ref_inv(t, wp, F64), chars, ndim)
            assert rel(wp._layout.fold(root), want) <= synth_tol(tree64, basis, t, wp, chars, want), (t[0], basis)


@pytest.mark.parametrize("dtype", [F32, F64], ids=tag)
@pytest.mark.parametrize("t", REC, ids=REC_IDS)
def test_assigned_basis_nodes_and_nan_below_them(t, dtype):
    """Fresh values on the basis nodes, NaN on every node below them: the root is finite and is the reference's partial-tree synthesis."""
    _, ndim, shape, wavelet, mode, depth, kw = t
    g = torch.Generator().manual_seed(31)
    for basis in some_bases(make_tree(t, dtype)[0], depth):
        wp, x = make_tree(t, dtype)
        chars = sorted(wp._bands, key=wp._bands.get)
        held = held_nodes(wp, depth)
        fresh = {k: torch.randn(held[k].shape, generator=g, dtype=F64).to(dtype) for k in basis}
        for k in basis:
            wp[k] = wp._layout.unfold(fresh[k].to(dev()))
        for s in range(depth + 1):
            for k in wp._keys_of_level(s):
                if any(k.startswith(b) and k != b for b in basis):
                    wp[k] = torch.full_like(wp[k], float("nan"))
        wp.reconstruct_basis(basis)
        got = wp._layout.fold(wp[""])
        assert torch.isfinite(got).all(), (t[0], basis)
        tree64 = {k: (fresh[k] if k in fresh else held[k]).double() for k in held}
        want = R.partial_synthesis(tree64, basis, ref_inv(t, wp, F64), chars, ndim)
        tol = 1e-12 if dtype == F64 else synth_tol(tree64, basis, t, wp, chars, want)
        e = rel(got, want)
        assert e <= tol, (t[0], basis, e, tol)


@pytest.mark.parametrize("t", REC, ids=REC_IDS)
def test_per_image_masks_that_select_different_bases(t):
    _, ndim, shape, wavelet, mode, depth, kw = t
    wp, x = make_tree(t, F64)
    chars = sorted(wp._bands, key=wp._bands.get)
    nb = len(chars)
    bases = some_bases(wp, depth)[1:3]  # image 0: the leaves; image 1: a mixed basis
    wp[wp._keys_of_level(depth)[0]]
    g = torch.Generator().manual_seed(32)
    held = {}
    for s in range(depth + 1):
        for k in wp._keys_of_level(s):
            if s > 0:
                wp[k] = wp._layout.unfold(torch.randn(wp._layout.fold(wp[k]).shape, generator=g, dtype=F64).to(dev()))
            held[k] = wp._layout.fold(wp[k]).cpu()
    masks = [torch.zeros(2, nb ** s, dtype=torch.bool) for s in range(depth + 1)]
    for i, basis in enumerate(bases):
        for k in basis:
            masks[len(k)][i, wp._keys_of_level(len(k)).index(k)] = True
    wp.reconstruct_basis([m.to(dev()) for m in masks])
    got = wp._layout.fold(wp[""])
    for i, basis in enumerate(bases):
        one = {k: v[i:i + 1] for k, v in held.items()}
        want = R.partial_synthesis(one, basis, ref_inv(t, wp, F64), chars, ndim)
        want = want[tuple(slice(0, n) for n in got[i:i + 1].shape)]  # (masks crop a longer root to the input's extents)
        assert rel(got[i:i + 1], want) <= 1e-12, (t[0], i)


def test_a_key_list_that_is_no_cover_raises():
    wp, _ = make_tree(REC[0], F32)
    with pytest.raises(ValueError, match="'d' meets no key"):
        wp.reconstruct_basis(["a"])
    with pytest.raises(ValueError, match="meets two keys"):
        wp.reconstruct_basis(["a", "d", "da"])


# ---- gradients -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", ["shannon", "logenergy", "norm"])
def test_gradients_against_float64_autograd_of_the_reference(cost):
    t = ("grad", 1, (3, 67), "db2", "symmetric", 2, {})
    wp, x = make_tree(t, F64, requires_grad=True)
    wp.node_costs(cost, **PARAMS[cost])["ad"].sum().backward()
    xr = x.detach().cpu().clone().requires_grad_(True)
    node = PR.nodes(xr, "db2", "symmetric", 2, ndim=1)["ad"]
    tt = node * node
    ref = {"shannon": lambda: -(tt * torch.log(tt)).sum(), "logenergy": lambda: torch.log(tt).sum(),
           "norm": lambda: node.abs().pow(1.5).sum()}[cost]()
    ref.backward()
    assert rel(x.grad, xr.grad) <= 1e-12
    # a second tree reconstructs differentiably from a basis
    wp, x = make_tree(t, F64, requires_grad=True)
    wp.reconstruct_basis(["aa", "ad", "d"])[""].square().sum().backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0


# ---- capture, reproducibility --------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_on_new_data():
    g = torch.Generator().manual_seed(41)
    a = torch.randn(7, 300, generator=g).to(dev())
    b = torch.randn(7, 300, generator=g).to(dev())
    x = a.clone()
    lim = BB.short_limit(F32)
    y = torch.randn(3, lim + 5, generator=g).to(dev())
    y2 = torch.randn(3, lim + 5, generator=g).to(dev())
    ybuf = y.clone()
    tree_in = torch.randn(3, 64, generator=g).to(dev())
    tree_new = torch.randn(3, 64, generator=g).to(dev())
    tbuf = tree_in.clone()

    def run():
        wp = ptwt_amd.WaveletPacket(tbuf, "db2", mode="periodization", maxlevel=3)
        return ptwt_amd.wentropy(x, "shannon", lead=1), ptwt_amd.wentropy(ybuf, "norm", p=1.5, lead=1), wp.best_basis("shannon", joint=False)

    eager = run()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()  # (warm-up on the side stream: allocations)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1]) and all(torch.equal(p, q) for p, q in zip(out[2], eager[2]))
    x.copy_(b), ybuf.copy_(y2), tbuf.copy_(tree_new)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], ptwt_amd.wentropy(b, "shannon", lead=1)) and not torch.equal(out[0], eager[0])
    assert torch.equal(out[1], ptwt_amd.wentropy(y2, "norm", p=1.5, lead=1))
    fresh = ptwt_amd.WaveletPacket(tree_new, "db2", mode="periodization", maxlevel=3).best_basis("shannon", joint=False)
    assert all(torch.equal(p, q) for p, q in zip(out[2], fresh))


@pytest.mark.parametrize("dtype", [F32, F64], ids=tag)
def test_the_same_call_twice_gives_the_same_bits(dtype):
    for n in (25, 300, BB.short_limit(dtype), BB.short_limit(dtype) + 1, 3 * BB.chunk(dtype) + 5):
        x = torch.randn(37, n, generator=torch.Generator().manual_seed(n)).to(dtype).to(dev())
        for cost in ("shannon", "sure"):
            a = ptwt_amd.wentropy(x, cost, lead=1, **PARAMS[cost])
            b = ptwt_amd.wentropy(x.clone(), cost, lead=1, **PARAMS[cost])
            assert torch.equal(a, b), (n, cost)


# ---- canaries ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["short", "long"])
def test_nothing_outside_out_and_the_workspace_changes(regime):
    lib = BB._lib()
    lim = BB.short_limit(F32)
    shapes = [(7, 25), (5, 300), (3, lim)] if regime == "short" else [(3, lim + 1), (2, 2 * BB.chunk(F32) + 3), (7, 25)]
    g = torch.Generator().manual_seed(51)
    xs = [torch.randn(*s, generator=g).to(dev()) for s in shapes]
    k = len(xs)
    arr = (_engine.EstimBand * k)()
    for b, x in zip(arr, xs):
        b.x = x.data_ptr()
        b.extent[:] = [1, x.shape[0], x.shape[1]]
        b.stride[:] = [x.numel(), x.shape[1], 1]
        b.rows_per_index = 1
    units = lib.mifwt_cost_plan(0, arr, k, None)
    assert units > 0
    pad = 64
    sentinel = -12345.678
    nodes = sum(s[0] for s in shapes)
    out = torch.full((pad + nodes + pad,), sentinel, dtype=F64, device=dev())
    ws = torch.full((pad + units + pad,), sentinel, dtype=F64, device=dev())
    ptrs = (ctypes.c_void_p * k)()
    at = pad
    for j, s in enumerate(shapes):
        ptrs[j] = out.data_ptr() + 8 * at
        at += s[0]
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.mifwt_cost_nodes(0, 0, 0.0, arr, k, ptrs, ws.data_ptr() + 8 * pad, 8 * units, stream)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((out[:pad] == sentinel).all()) and bool((out[pad + nodes:] == sentinel).all())
    assert bool((ws[:pad] == sentinel).all()) and bool((ws[pad + units:] == sentinel).all())
    got = out[pad:pad + nodes].cpu().numpy()
    want = np.concatenate([R.costs(x.double().cpu().numpy(), "shannon")[0] for x in xs])
    bound = np.concatenate([R.costs(x.double().cpu().numpy(), "shannon")[1] for x in xs])
    assert np.all(np.abs(got - want) <= bound)
    if regime == "short":
        assert bool((ws == sentinel).all()), "short nodes take no workspace slot"
        rc = lib.mifwt_cost_nodes(0, 0, 0.0, arr, k, ptrs, None, 0, stream)  # ... and no workspace at all
        torch.cuda.synchronize()
        assert rc == 0
    else:
        assert lib.mifwt_cost_nodes(0, 0, 0.0, arr, k, ptrs, ws.data_ptr(), 8 * units - 1, stream) == -3  # MIFWT_ERR_WORKSPACE


# ---- past 2^31 elements --------------------------------------------------------------------------------------------------------------------
def test_rows_past_2_to_the_31_elements():
    """``wentropy(lead=1)`` on [2^19 + 1, 4096] float32: 2^31 + 4096 elements, 8 GiB; the first, the last and a dozen sampled nodes
    against float64 of those rows."""
    free = torch.cuda.mem_get_info()[0]
    if free < 10 << 30:
        pytest.skip(f"wentropy past 2^31: 10 GiB needed, {free / 2 ** 30:.1f} GiB free")
    rows, n = (1 << 19) + 1, 4096
    x = torch.empty((rows, n), dtype=F32, device=dev())
    gen = torch.Generator(device=dev()).manual_seed(61)
    x.normal_(generator=gen)
    got = ptwt_amd.wentropy(x, "shannon", lead=1)
    got_n = ptwt_amd.wentropy(x, "threshold", value=1.0, lead=1)
    assert got.shape == (rows,)
    pick = [0, rows - 1] + [int(v) for v in torch.randint(1, rows - 1, (12,), generator=torch.Generator().manual_seed(62))]
    sample = x[pick].double().cpu().numpy()
    want, bound = R.costs(sample, "shannon")
    check(got[pick], want, bound, "rows past 2^31")
    assert got_n[pick].cpu().tolist() == [float((np.abs(r) > 1.0).sum()) for r in sample]
    del x
    small = torch.zeros(4, device=dev())
    with pytest.raises(ValueError, match=r"fewer than 2\^31 elements per leading index, got 2147483648"):
        ptwt_amd.wentropy(small.as_strided((2, 1 << 16, 1 << 15), (0, 0, 0)), lead=1)
