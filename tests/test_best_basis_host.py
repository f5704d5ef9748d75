"""wentropy / node_costs / best_basis / reconstruct_basis without a GPU: the reference pruning of tests/_best_basis_ref.py against a brute
force over every admissible basis, ``_prune`` against the reference bit for bit, the float64 composition against the ``math.fsum``
reference, every error raised before a launch, the guards and the regime choice of the unit plan, the C ABI surface, and a CPU tree on
the oracle level engine."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine, best_basis as BB
from tests import _best_basis_ref as R
from tests._oracle_engine import OracleLevelEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = {"shannon": {}, "logenergy": {}, "norm": {"p": 1.5}, "threshold": {"value": 0.7}, "sure": {"value": 0.7}}


@pytest.fixture()
def oracle_engine(monkeypatch):
    monkeypatch.setattr(_engine, "ENGINE", OracleLevelEngine())


def _table(rng, nb, depth, ties=False):
    if ties:  # small integers: sums are exact, and parents often equal the sum of their children
        return [rng.integers(1, 4, nb ** s).astype(np.float64) * (nb ** (depth - s)) / 2 for s in range(depth + 1)]
    return [rng.random(nb ** s) * (nb ** (depth - s)) for s in range(depth + 1)]


# ---- pruning ---------------------------------------------------------------------------------------------------------------------------
def test_reference_counts_the_bases():
    assert len(R.bases(2, 2)) == 5 and len(R.bases(4, 2)) == 17 and len(R.bases(2, 0)) == 1 and len(R.bases(2, 1)) == 2


@pytest.mark.parametrize("nb", [2, 4])
def test_reference_pruning_is_the_brute_force_minimum(nb):
    rng = np.random.default_rng(11 + nb)
    for trial in range(200):
        t = _table(rng, nb, 1 + trial % 2, ties=trial % 4 == 3)
        sel, best = R.prune(t)
        assert R.is_cover(sel)
        total = R.basis_total(t, [(s, j) for s, m in enumerate(sel) for j, on in enumerate(m) if on])
        lowest, count = R.brute(t)
        assert count == len(R.bases(nb, len(t) - 1))
        assert abs(total - lowest) <= 1e-15 * sum(float(np.abs(c).sum()) for c in t), (trial, total, lowest)
        assert abs(best[0][0] - lowest) <= 1e-15 * sum(float(np.abs(c).sum()) for c in t)


def test_a_tie_keeps_the_parent():
    sel, best = R.prune([[3.0], [1.0, 2.0]])
    assert sel == [[True], [False, False]] and best[0] == [3.0]
    sel, _ = R.prune([[3.0], [1.0, 2.0], [0.25, 0.75, 5.0, 5.0]])  # "a" ties with its children, "d" beats them: the root still ties
    assert sel == [[True], [False, False], [False] * 4]
    s, b = BB._prune([torch.tensor([3.0], dtype=torch.float64), torch.tensor([1.0, 2.0], dtype=torch.float64)])
    assert s[0].tolist() == [True] and s[1].tolist() == [False, False] and b[0].tolist() == [3.0]


@pytest.mark.parametrize("nb", [2, 4])
@pytest.mark.parametrize("ties", [False, True])
def test_prune_equals_the_reference_bit_for_bit(nb, ties):
    rng = np.random.default_rng(5 + nb + 10 * ties)
    for depth in (0, 1, 2, 3, 4):
        batch = [_table(rng, nb, depth, ties) for _ in range(6)]
        costs = [torch.from_numpy(np.stack([t[s] for t in batch])) for s in range(depth + 1)]
        sel, best = BB._prune(costs)
        assert [m.dtype for m in sel] == [torch.bool] * (depth + 1) and [b.dtype for b in best] == [torch.float64] * (depth + 1)
        for i, t in enumerate(batch):
            rs, rb = R.prune(t)
            for s in range(depth + 1):
                assert sel[s][i].tolist() == rs[s], (depth, i, s)
                assert best[s][i].numpy().tobytes() == np.array(rb[s], dtype=np.float64).tobytes(), (depth, i, s)
        # a batch of shape [2, 3, nb^s] gives the same masks
        sel2, _ = BB._prune([c.reshape(2, 3, -1) for c in costs])
        assert all(torch.equal(a.reshape(6, -1), b) for a, b in zip(sel2, sel))
    if ties:
        assert any(R.prune(_table(rng, nb, 2, True))[0][0][0] for _ in range(50))  # (ties do occur in these tables)


# ---- the composition -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", R.COSTS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_composed_costs_against_the_reference(cost, dtype):
    g = torch.Generator().manual_seed(3)
    for n in (1, 2, 5, 17, 300):
        x = torch.randn(7, n, generator=g, dtype=torch.float64).to(dtype)
        x[::2, ::3] = 0.0
        want, bound = R.costs(x.double().numpy(), cost, **PARAMS[cost])
        got = BB._composed_costs(x, 7, cost, **PARAMS[cost])
        assert got.dtype == torch.float64 and got.shape == (7,)
        assert np.all(np.abs(got.numpy() - want) <= bound), (cost, n, np.abs(got.numpy() - want).max())
        via = ptwt_amd.wentropy(x, cost, lead=1, **PARAMS[cost])  # (a CPU tensor takes the composed route)
        assert torch.equal(via, got)
    for p in (1, 2, 3.5):
        x = torch.randn(3, 40, generator=g, dtype=dtype)
        want, bound = R.costs(x.double().numpy(), "norm", p=p)
        assert np.all(np.abs(BB._composed_costs(x, 3, "norm", p=p).numpy() - want) <= bound)


def test_zero_conventions_and_the_gradient_at_zero():
    z = torch.zeros(2, 5, dtype=torch.float64)
    assert ptwt_amd.wentropy(z, "shannon", lead=1).tolist() == [0.0, 0.0]
    assert ptwt_amd.wentropy(z, "logenergy", lead=1).tolist() == [0.0, 0.0]
    assert ptwt_amd.wentropy(z, "sure", value=0.0).item() == 0.0 and ptwt_amd.wentropy(z, "threshold", value=0.0).item() == 0.0
    x = torch.tensor([0.0, 0.5, -2.0, 0.0], dtype=torch.float64, requires_grad=True)
    for cost, want in (("shannon", lambda t: -2 * t * (torch.log(t * t) + 1)), ("logenergy", lambda t: 2 / t),
                       ("norm", lambda t: 1.5 * t.abs() ** 0.5 * t.sign())):
        c = ptwt_amd.wentropy(x, cost, **PARAMS[cost])
        (g,) = torch.autograd.grad(c, x, create_graph=True)
        assert torch.isfinite(g).all() and g[0] == 0 and g[3] == 0
        assert torch.allclose(g[1:3], want(x.detach()[1:3]), rtol=1e-14, atol=0)
        (gg,) = torch.autograd.grad(g.sum(), x)  # gradients of any order exist (the second one is unbounded at 0 itself)
        assert torch.isfinite(gg[1:3]).all()


def test_empty_shapes_launch_nothing():
    assert ptwt_amd.wentropy(torch.zeros(0, 5), lead=1).shape == (0,)
    e = ptwt_amd.wentropy(torch.zeros(3, 0), "sure", value=1.0, lead=1)
    assert e.dtype == torch.float64 and e.tolist() == [0.0, 0.0, 0.0]
    assert ptwt_amd.wentropy(torch.zeros(2, 3, 4), lead=2).shape == (2, 3) and ptwt_amd.wentropy(torch.ones(4)).shape == ()


# ---- errors ----------------------------------------------------------------------------------------------------------------------------
BAD = [
    (dict(cost="entropy"), "unknown cost"), (dict(cost="norm"), "needs p"), (dict(cost="norm", p=0.5), "p >= 1"),
    (dict(cost="norm", p=float("nan")), "p >= 1"), (dict(cost="norm", p=2, value=1.0), "not value"), (dict(cost="norm", p="2"), "number"),
    (dict(cost="shannon", p=2), "takes no p"), (dict(cost="shannon", value=1.0), "takes no value"), (dict(cost="logenergy", p=1), "takes no p"),
    (dict(cost="threshold"), "needs value"), (dict(cost="threshold", value=-1.0), "value >= 0"), (dict(cost="sure"), "needs value"),
    (dict(cost="sure", value=1.0, p=2), "takes no p"), (dict(cost="sure", value=torch.tensor(1.0)), "number"),
    (dict(lead=3), "lead must be"), (dict(lead=-1), "lead must be"), (dict(lead=True), "lead must be"),
]


@pytest.mark.parametrize("kw,match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_wentropy_value_errors(kw, match):
    with pytest.raises(ValueError, match=match):
        ptwt_amd.wentropy(torch.ones(4, 4), **kw)


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128, torch.float16, torch.bfloat16, torch.bool, torch.int32])
def test_wentropy_refuses_other_dtypes(dtype):
    with pytest.raises(ValueError, match="float32 and float64"):
        ptwt_amd.wentropy(torch.zeros(8).to(dtype))


def test_2_to_the_31_elements_per_leading_index_are_refused():
    small = torch.zeros(4)
    past = small.as_strided((2, 1 << 16, 1 << 15), (0, 0, 0))
    with pytest.raises(ValueError, match=r"fewer than 2\^31 elements per leading index, got 2147483648"):
        ptwt_amd.wentropy(past, lead=1)
    with pytest.raises(ValueError, match=r"fewer than 2\^31"):
        ptwt_amd.wentropy(torch.empty((46341, 46341), device="meta"))


# ---- the unit plan ---------------------------------------------------------------------------------------------------------------------
def _band(ext, rp=0, last=1):
    b = _engine.EstimBand()
    b.extent[:] = ext
    b.stride[:] = [ext[1] * ext[2], ext[2], last]
    b.rows_per_index = rp
    return b


def _plan(dt, *bands, starts=False):
    arr = (_engine.EstimBand * max(1, len(bands)))(*bands)
    us = (ctypes.c_int64 * (len(bands) + 1))()
    n = BB._lib().mifwt_cost_plan(dt, arr, len(bands), us)
    return (n, list(us)) if starts else n


def test_api_surface_and_limits():
    assert "wentropy" in ptwt_amd.__all__ and ptwt_amd.wentropy is BB.wentropy
    assert (BB.KID_COST_NODES, BB.KID_COST_FINISH) == (61, 62) and BB.COSTS == {c: i for i, c in enumerate(R.COSTS)}
    for cls in (ptwt_amd.WaveletPacket, ptwt_amd.WaveletPacket2D):
        for name in ("node_costs", "best_basis", "reconstruct_basis"):
            assert getattr(cls, name) is getattr(BB, name)
    with open(os.path.join(ROOT, "include", "mifwt.h")) as f:
        header = f.read()
    for name, v in (("MIFWT_KID_COST_NODES", 61), ("MIFWT_KID_COST_FINISH", 62), ("MIFWT_COST_SHANNON", 0), ("MIFWT_COST_LOGENERGY", 1),
                    ("MIFWT_COST_NORM", 2), ("MIFWT_COST_THRESHOLD", 3), ("MIFWT_COST_SURE", 4), ("MIFWT_ABI_VERSION", 3)):
        assert re.search(rf"#define {name} {v}\b", header), name
    lib = _engine.load_library()
    for sym in _engine.COST_ENTRIES:
        assert getattr(lib, sym) is not None and sym not in _engine._ENTRIES
        assert re.search(rf"\b{sym}\(", header), sym
    assert _engine.ABI_VERSION == 3 and lib.mifwt_abi_version() == 3
    assert BB.max_segments() == 24
    for dt in (torch.float32, torch.float64):
        assert 0 < BB.short_limit(dt) < BB.chunk(dt)
    assert BB._lib().mifwt_cost_short_limit(2) == -1 and BB._lib().mifwt_cost_chunk(3) == -1  # 16-bit storage: MIFWT_ERR_BADARG
    assert "host" in BB.best_basis.__doc__ and "NOT validated" in BB.reconstruct_basis.__doc__


def test_regime_at_the_short_limit():
    """Short nodes share workgroups (fewer units than nodes), a long node has units of its own: one per chunk."""
    for dt, dtype in ((0, torch.float32), (1, torch.float64)):
        lim, chunk = BB.short_limit(dtype), BB.chunk(dtype)
        nodes = 64
        assert _plan(dt, _band([1, nodes, lim], 1)) < nodes and _plan(dt, _band([1, nodes, lim + 1], 1)) == nodes
        assert _plan(dt, _band([1, nodes, 5], 1)) == 1  # 4 lanes a node: 64 nodes are one pass of one workgroup
        assert BB._regime(dtype, lim) == "short" and BB._regime(dtype, lim + 1) == "long"
        # the node length decides, not the row length: 2 rows of lim / 2 + 1 elements are one long node
        assert _plan(dt, _band([1, 2 * nodes, lim // 2 + 1], 2)) == nodes and _plan(dt, _band([1, 2 * nodes, lim // 2], 2)) < nodes
        assert _plan(dt, _band([1, 3, 4 * chunk], 1)) in (3 * 4, 3 * 5)  # (a slot more per row for misaligned starts)
        n, starts = _plan(dt, _band([1, 7, 25], 1), _band([1, 7, lim + 1], 1), _band([1, 1, 1], 0), starts=True)
        assert starts == [0, 1, 8, 9] and n == 9


#: the guards: (what, extents, rows per node, the answer of mifwt_cost_plan: a unit count > 0 or the error) — the last accepted and the
#: first refused value of every one; no data pointer, nothing is launched
GUARDS = [
    ("n = 2^30", [1, 1, 1 << 30], 0, 1), ("n = 2^30 + 1", [1, 1, (1 << 30) + 1], 0, -2),
    ("e1 = 2^30", [1, 1 << 30, 1], 1, 1), ("e1 = 2^30 + 1", [1, (1 << 30) + 1, 1], 1, -2),
    ("rows = 2^31 - 1", [(1 << 31) - 1, 1, 1], 1, 1), ("rows = 2^31", [2, 1 << 30, 1], 1, -2),
    ("node = 2^31 - 2", [1, 2, (1 << 30) - 1], 0, 1), ("node = 2^31", [1, 2, 1 << 30], 0, -2),
    ("node = 2^31, short rows", [2, 1 << 30, 1], 0, -2),
]


@pytest.mark.parametrize("what,ext,rp,want", GUARDS, ids=[g[0] for g in GUARDS])
def test_guards_of_the_cost_plan(what, ext, rp, want):
    lib = BB._lib()
    for dt in (0, 1):
        got = _plan(dt, _band(ext, rp))
        assert (got > 0) if want > 0 else got == want, (what, dt, got)
        out = (ctypes.c_void_p * 1)()
        rc = lib.mifwt_cost_nodes(dt, 0, 0.0, (_engine.EstimBand * 1)(_band(ext, rp)), 1, out, None, 0, None)
        assert rc == (want if want < 0 else -1), (what, dt, rc)  # (inside the guards: no data pointer)


def test_bad_arguments_of_the_cost_entries():
    lib = BB._lib()
    ok = _band([1, 6, 5], 2)
    assert _plan(0, ok) == 1
    assert _plan(0) == -1 and _plan(0, *[ok] * 25) == -1 and _plan(0, *[ok] * 24) == 24  # nseg
    assert _plan(2, ok) == -1  # 16-bit storage
    assert _plan(0, _band([1, 6, 5], last=2)) == -1  # a non-unit innermost stride
    assert _plan(0, _band([1, 6, 5], 4)) == -1  # rows_per_index does not divide the rows
    assert _plan(0, _band([1, 0, 5], 1)) == -1  # an empty segment
    assert _plan(0, ok, _band([1, 1 << 31, 1], 1)) == -2
    many = _band([(1 << 31) - 1, 1, 1], 1)  # one unit per 256 nodes of one element ...
    assert _plan(0, many) == -(-((1 << 31) - 1) // 512)  # (4 lanes a node, 8 passes)
    arr, out = (_engine.EstimBand * 1)(ok), (ctypes.c_void_p * 1)()
    assert lib.mifwt_cost_nodes(0, 5, 0.0, arr, 1, out, None, 0, None) == -1  # unknown functional
    assert lib.mifwt_cost_nodes(0, -1, 0.0, arr, 1, out, None, 0, None) == -1
    assert lib.mifwt_cost_nodes(0, 0, 0.0, arr, 1, None, None, 0, None) == -1
    # a long node and a workspace that is too small: refused before any pointer is read (the pointers below are never dereferenced)
    long_ = _band([1, 3, BB.short_limit(torch.float32) + 1], 1)
    long_.x = 256
    out[0] = 256
    assert lib.mifwt_cost_nodes(0, 0, 0.0, (_engine.EstimBand * 1)(long_), 1, out, None, 0, None) == -3
    assert lib.mifwt_cost_nodes(0, 0, 0.0, (_engine.EstimBand * 1)(long_), 1, out, 256, 8 * 3 - 1, None) == -3  # MIFWT_ERR_WORKSPACE


# ---- key lists ---------------------------------------------------------------------------------------------------------------------------
def test_key_lists_are_validated(oracle_engine):
    wp = ptwt_amd.WaveletPacket(torch.randn(2, 32, dtype=torch.float64), "db2", mode="symmetric", maxlevel=2)
    for basis, match in ((["a"], "'d' meets no key"), (["aa", "d"], "'ad' meets no key"), (["a", "aa", "ad", "d"], "meets two keys"),
                         (["", "a", "d"], "meets two keys"), (["a", "d", "d"], "twice"), (["a", "x"], "invalid key"), ([], "empty basis"),
                         (["a", "h"], "invalid key")):
        with pytest.raises(ValueError, match=match):
            wp.reconstruct_basis(basis)
    with pytest.raises(KeyError):
        wp.reconstruct_basis(["a", "da", "ddd", "dda"])  # deeper than maxlevel
    wp2 = ptwt_amd.WaveletPacket2D(torch.randn(2, 16, 16, dtype=torch.float64), "haar", mode="zero", maxlevel=1)
    with pytest.raises(ValueError, match="'d' meets no key"):
        wp2.reconstruct_basis(["a", "h", "v"])
    with pytest.raises(TypeError):
        wp.reconstruct_basis("a")


# ---- a CPU tree on the oracle engine ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndim", [1, 2])
def test_cpu_tree_best_basis_round_trip(oracle_engine, ndim):
    g = torch.Generator().manual_seed(9)
    x = torch.randn(*((3, 64) if ndim == 1 else (2, 32, 32)), generator=g, dtype=torch.float64)
    cls = ptwt_amd.WaveletPacket if ndim == 1 else ptwt_amd.WaveletPacket2D
    wp = cls(x, "db2", mode="zero", maxlevel=2)
    costs = wp.node_costs("shannon")
    assert set(costs) == {k for s in range(3) for k in wp._keys_of_level(s)}
    for k, c in costs.items():
        want, bound = R.costs(wp[k].numpy(), "shannon", lead=1)
        assert c.dtype == torch.float64 and c.shape == (x.shape[0],) and np.all(np.abs(c.numpy() - want) <= bound), k
    keys = wp.best_basis("shannon")
    masks = wp.best_basis("shannon", joint=False)
    assert [tuple(m.shape) for m in masks] == [(x.shape[0], (2 ** ndim) ** s) for s in range(3)]
    table = [torch.stack([costs[k] for k in wp._keys_of_level(s)], -1) for s in range(3)]
    sel, _ = R.prune(R.as_table([t.sum(0) for t in table]))
    assert keys == sorted(R.keys_of(sel, wp._keys_of_level), key=lambda k: [wp._bands[c] for c in k])
    for i in range(x.shape[0]):
        assert [m[i].tolist() for m in masks] == R.prune(R.as_table([t[i] for t in table]))[0]
    for basis in (keys, masks, [""], wp._keys_of_level(1), wp._keys_of_level(2)):
        wp = cls(x, "db2", mode="zero", maxlevel=2)
        assert wp.reconstruct_basis(basis) is wp
        assert torch.allclose(wp[""], x, rtol=0, atol=1e-12)
