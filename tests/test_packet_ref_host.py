"""CPU companion of tests/test_gpu_packets.py: the check of the checker.

  * tests/_packet_ref.py reproduces every case of tests/golden/ptwt_ref_packets.npz — trees of the reference's own packet classes: odd
    lengths and their crops, ``axis`` / ``axes``, both values of ``separable``, unbatched inputs — to 1e-12, nodes and the reconstruction
    after the leaves were halved; its tree model does too.
  * The tree logic of ``packets.py`` on the oracle level engine (tests/_oracle_engine.py) equals the reference to 1e-12 on every float64
    row of the GPU module's table and on its assignment / lazy-expansion scenarios: a wrong tree logic fails here, before any GPU run.
  * Three wrong engines — wrappers of the oracle engine, each invisible to a round trip with a named orthogonal wavelet — fail the
    independent-bank rows: detail bands 1 and 2 exchanged (in both directions), the odd-length crop taken from the front, and a level
    buffer that is reused although nodes of it were assigned.
  * The reference's own float32 run passes, against its float64 run, the two checks a kernel has to pass (norm-wise inside the bound —
    true by construction — and max-abs inside ten times it — not by construction), and its deviation stays below the a-priori
    rounding bound of the levels it passed: no row is badly conditioned (cancellation would lift it above that), no bound is vacuous.
  * The table reaches what it claims: ``_engine.kernel_id`` (a host query of the library) puts the ids a row was written for among its
    launches, and the union covers the module's list.
"""
import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine
from tests import _golden as G
from tests import _packet_ref as R
from tests import test_gpu_packets as T
from tests._oracle_engine import OracleLevelEngine

f32, f64 = torch.float32, torch.float64


@pytest.fixture()
def engine():
    """Puts an engine in place of the HIP one for the test; the engine and the routing memos are restored afterwards."""
    keep = _engine.ENGINE

    def use(e):
        _engine.ENGINE = e

    use(OracleLevelEngine())
    yield use
    _engine.ENGINE = keep
    for memo in _engine._routing_caches:
        memo.clear()


def _golden_cases():
    z, idx = G.load("ptwt_ref_packets.npz")
    for case in idx:
        kw = dict(case["kw"])
        axes = kw.pop("axis", None)
        axes = kw.pop("axes", axes)
        yield z, case, dict(ndim=case["dim"], separable=kw.pop("separable", False), axes=tuple(axes) if isinstance(axes, list) else axes)
        assert not kw


def test_reference_reproduces_the_goldens_of_the_reference_classes():
    worst, count = 0.0, 0
    for z, case, kw in _golden_cases():
        k, depth = case["key"], case["maxlevel"]
        x = torch.from_numpy(z[k + "_x"])
        assert R.keys_of_level(depth, kw["ndim"], kw["separable"]) == case["keys"]
        tree = R.nodes(x, case["wavelet"], case["mode"], depth, **kw)
        model = R.Tree(x, case["wavelet"], case["mode"], depth, **kw)
        for key in case["keys"]:
            want = z["%s_n_%s" % (k, key)]
            for got in (tree[key], model[key]):
                assert tuple(got.shape) == want.shape, (case, key)
                worst = max(worst, G.relerr(got.numpy(), want))
        for key in case["keys"]:
            tree[key] = 0.5 * tree[key]
            model[key] = 0.5 * model[key]
        want = z[k + "_rec"]
        for got in (R.reconstruct(tree, case["wavelet"], depth, **kw)[""], model.reconstruct()[""]):
            assert tuple(got.shape) == want.shape, case
            worst = max(worst, G.relerr(got.numpy(), want))
        count += 1
    assert count == 29 and worst < 1e-12, worst


def test_key_tables_are_the_two_maps_of_the_reference():
    """h of the non-separable tree filters the ROWS' axis with the high-pass (``wavedec2``'s horizontal detail), h of the separable tree
    the columns' (``fswavedec2``'s "ad"); the goldens hold both, and exchanging the tables breaks them."""
    assert R.KEYS_2D[False]["h"] == R.KEYS_2D[True]["v"] == (1, 0) and R.KEYS_2D[False]["v"] == R.KEYS_2D[True]["h"] == (0, 1)
    z, idx = G.load("ptwt_ref_packets.npz")
    for key, sep in (("p002", False), ("p004", True)):
        case = next(c for c in idx if c["key"] == key)
        x = torch.from_numpy(z[key + "_x"])
        wrong = R.nodes(x, case["wavelet"], case["mode"], 1, 2, separable=not sep)
        right = R.nodes(x, case["wavelet"], case["mode"], 2, 2, separable=sep)
        assert G.relerr(right["hv"].numpy(), z[key + "_n_hv"]) < 1e-12
        assert G.relerr(wrong["h"].numpy(), right["h"].numpy()) > 0.1


def test_rounded_rounds_every_node_after_every_level():
    x = torch.randn(2, 30, 34, generator=torch.Generator().manual_seed(3), dtype=f64).to(torch.bfloat16).double()
    for dt in (torch.float16, torch.bfloat16):
        r = R.rounded(dt)
        tree = r.nodes(x, "db2", "symmetric", 2, 2)
        plain = R.nodes(x, "db2", "symmetric", 2, 2)
        for k, t in tree.items():
            assert torch.equal(t, t.to(dt).double()), k
        assert torch.equal(tree["a"], plain["a"].float().to(dt).double())
        assert torch.equal(r.nodes(tree["a"], "db2", "symmetric", 1, 2)["v"], tree["av"])  # (level 2 starts from the ROUNDED level 1)
        rec = r.reconstruct(tree, "db2", 2, 2)
        assert all(torch.equal(rec[k], rec[k].to(dt).double()) for k in R.all_keys(1, 2))
        assert 0 < G.relerr(rec[""].numpy()[..., :30, :34], x.numpy()) < 4 * r.per_level


F64_CASES = [c for c in T.CASES if c.dtype == f64]


@pytest.mark.parametrize("c", F64_CASES, ids=T.case_id)
def test_tree_logic_on_the_oracle_engine(engine, c):
    T.run_case(c, device="cpu")


@pytest.mark.parametrize("ndim,shape", T.SEMANTICS, ids=["2d", "1d"])
def test_tree_semantics_on_the_oracle_engine(engine, ndim, shape):
    T.run_semantics(ndim, shape, device="cpu")


class WrongEngine(OracleLevelEngine):
    """The oracle engine with one mistake of a level route or of the buffer handling around it."""

    def __init__(self, kind):
        self.kind, self.held = kind, {}

    def analysis(self, x, dec_lo, dec_hi, mode_id):
        if self.kind == "stale":  # the flattened buffer this engine wrote is read again, whatever the caller gathered since
            x = self.held.get(tuple(x.shape), x)
        out = super().analysis(x, dec_lo, dec_hi, mode_id)
        if self.kind == "swap" and out.shape[1] == 4:
            out = out[:, [0, 2, 1, 3]].contiguous()
        self.held[(out.shape[0] * out.shape[1], *out.shape[2:])] = out.reshape(-1, *out.shape[2:]).clone()
        return out

    def synthesis(self, approx, details, rec_lo, rec_hi, out_extent):
        if self.kind == "swap" and len(details) == 3:
            details = [details[1], details[0], details[2]]
        if self.kind == "stale":
            nb = 1 + len(details)
            old = self.held.get((approx.shape[0] * nb, *approx.shape[1:]))
            if old is not None:
                old = old.reshape(approx.shape[0], nb, *approx.shape[1:])
                approx, details = old[:, 0], [old[:, s] for s in range(1, nb)]
        if self.kind == "front":
            flen = len(rec_lo)
            full = [2 * m - flen + 2 for m in approx.shape[1:]]
            y = super().synthesis(approx, details, rec_lo, rec_hi, full)
            for a, n in enumerate(out_extent):
                y = y.narrow(1 + a, full[a] - n, n)
            return y.contiguous()
        return super().synthesis(approx, details, rec_lo, rec_hi, out_extent)


KINDS = ("swap", "front", "stale")
RANDOM_F64 = [c for c in F64_CASES if c.name == "random"]


@pytest.mark.parametrize("kind", KINDS)
def test_wrong_engines_pass_a_round_trip_with_an_orthogonal_wavelet(engine, kind):
    """The blind spot: a tree of a named orthogonal wavelet whose leaves go back unchanged comes back as the input under each of them
    (haar on 32 x 32 and on 64 samples: no level is odd, so nothing is cropped)."""
    engine(WrongEngine(kind))
    for cls, shape in ((ptwt_amd.WaveletPacket2D, (2, 32, 32)), (ptwt_amd.WaveletPacket, (3, 64))):
        x = torch.randn(*shape, generator=torch.Generator().manual_seed(9), dtype=f64)
        wp = cls(x, "haar", mode="symmetric", maxlevel=3)
        wp.initialize(wp.get_level(3, "natural"))
        wp.reconstruct()
        assert G.relerr(wp[""].numpy(), x.numpy()) < 1e-12, (kind, shape)


@pytest.mark.parametrize("kind", KINDS)
def test_wrong_engines_fail_the_independent_bank_rows(engine, kind):
    """Every wrong engine fails the node check of the rows with four independent filters (the band exchange: the 2-D rows, it has no
    1-D form), by far: the comparison that fails is off by more than 1e-2.  (The stale buffer shows already in ``reconstruct()`` of the
    untouched tree: the rebuilt level is not what the analysis wrote, there being no perfect reconstruction with such a bank.)"""
    rows = [c for c in RANDOM_F64 if c.ndim == 2 or kind != "swap"]
    assert len(rows) >= 3
    for c in rows:
        engine(WrongEngine(kind))
        with pytest.raises(AssertionError) as info:
            T.run_case(c, device="cpu")
        args = info.value.args
        assert info.type is T.Mismatch and args[0] == T.case_id(c) and args[1] == ("fwd" if kind == "swap" else "inv0"), args
        assert args[3] == "norm-wise" and args[4] > 1e-2, args
    engine(OracleLevelEngine())
    for c in RANDOM_F64:
        T.run_case(c, device="cpu")


F32_CASES = [c for c in T.CASES if c.dtype == f32]


def a_priori(c, passed):
    """Worst-case rounding of a float32 tap-by-tap run, relative to the magnitudes that enter the sums: L additions of products per
    axis pass (gamma_L ~ L 2^-24), ``ndim`` passes per level, amplified by at most (sum |taps|)^ndim per level pass — summed over the
    ``passed`` levels (s for a node of level s, 2 x depth - s for one rebuilt by ``reconstruct()``).  A deviation above it means cancellation: a badly
    conditioned row."""
    bank = R.bank_of(T.wavelet_of(c))
    amp = max(1.0, max(sum(abs(v) for v in f) for f in bank)) ** c.ndim
    return passed * c.ndim * len(bank[0]) * 2.0 ** -24 * amp


@pytest.mark.parametrize("c", F32_CASES, ids=T.case_id)
def test_float32_reference_stays_inside_its_own_bound_rule(c):
    x = T.make_input(c, "cpu")[1]
    depth, fail = T.depth_of(c)
    e = R.e_ref32(x, T.wavelet_of(c), c.mode, depth, c.ndim, c.separable, c.axes, inverse=fail is None)
    for direction, levels in e.items():
        assert sorted(levels) == list(range(1, depth + 1) if direction == "fwd" else range(depth))
        for level, (norm, maxabs) in levels.items():
            bound, passed = max(1e-6, 10 * norm), level if direction == "fwd" else 2 * depth - level
            print(T.case_id(c), direction, level, f"norm-wise {norm:.3e} max-abs {maxabs:.3e} bound {bound:.3e} a priori {a_priori(c, passed):.3e}")
            assert 0 < norm <= bound and norm < a_priori(c, passed), (direction, level, norm, bound, a_priori(c, passed))
            assert maxabs < 10 * bound, (direction, level, maxabs, bound)


def test_the_table_reaches_what_it_claims():
    """No GPU work: per row, ``_engine.kernel_id`` puts the ids the row was written for among its launches; the union covers the list
    of the module's closing test; the reflect rows on (2, 20, 22) are refused at level 5, no other row is refused; ids are unique."""
    ids = [T.case_id(c) for c in T.CASES]
    assert len(ids) == len(set(ids))
    reached = set()
    for c in T.CASES:
        fwd, inv = T.expected_launches(c)
        depth, fail = T.depth_of(c)
        got = {k for k, _ in fwd} | ({k for k, _ in inv} if fail is None else set())
        assert c.want <= got, (T.case_id(c), sorted(c.want), fwd, inv)
        assert len(fwd) == len(inv) == depth
        reached |= got
        if c.name == "short" and c.ndim == 2:  # nodes shorter than the filter
            flen = T.flen_of(c)
            assert (fail == 5) == (c.mode == "reflect") and (fail or any(min(e) < flen for _, e in fwd)), (T.case_id(c), fail, fwd)
        elif c.name != "short":
            assert fail is None, T.case_id(c)
        if c.name == "short16":
            assert all(min(e) < T.flen_of(c) for _, e in fwd)
        if c.name == "short" and c.ndim == 1:
            assert sum(e[0] < T.flen_of(c) for _, e in fwd) == 2
    assert T.MUST_REACH <= reached, sorted(T.MUST_REACH - reached)
    assert {c.dtype for c in T.CASES} == {f32, f64, torch.float16, torch.bfloat16}
    assert {c.mode for c in T.CASES} == {"zero", "constant", "reflect", "periodic", "symmetric"}
    assert any(c.separable for c in T.CASES) and any(c.layout == "permuted" for c in T.CASES) and any(c.layout == "slice" for c in T.CASES)
    b = T.wavelet_of(RANDOM_F64[0])
    assert len(b) == 4 and len({tuple(f) for f in b}) == 4
    assert [round(R.weight(i), 3) for i in range(3)] == [round(0.75 + 0.5 * np.cos(1.0 + i), 3) for i in range(3)]
