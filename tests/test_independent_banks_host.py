"""CPU companion of tests/test_gpu_independent_banks.py: the check of the checker.  The harness of tests/_grad_ref.py runs on the CPU
against three DELIBERATELY WRONG level engines (wrappers of tests/_oracle_engine.py that know the bank):

(a) the analysis adjoint computed as the synthesis with the bank's ``rec_*`` filters (plus the correct border fold);
(b) the high-pass rebuilt from the low-pass by the quadrature-mirror relation, in analysis and synthesis;
(c) the synthesis run with ``flip(dec_*)``.

With ``db4`` / ``sym5`` every one of them passes the harness at the GPU module's bounds — the blind spot of a suite that knows named
orthogonal wavelets only, pinned; with that module's banks of four independent filters each fails by orders of magnitude.  The
correct engine passes both, the two references (numpy oracle, differentiable torch reference) agree with such banks to 1e-12
(measured: 1.2e-15), and the table of the GPU module covers what it claims."""
import numpy as np
import pytest
import torch

from oracle import fwt_oracle as O
from oracle import torch_autograd_ref as R
from ptwt_amd import _engine
from tests import _golden as G
from tests import _grad_ref as D
from tests import test_gpu_independent_banks as T
from tests._oracle_engine import OracleLevelEngine

f32, f64 = torch.float32, torch.float64
MODES5 = T.MODES5


def qmf_dec(lo):
    """dec_hi of an orthogonal bank from its dec_lo (exact for every committed orthogonal bank)."""
    lo = np.asarray(lo, dtype=np.float64)
    return -((-1.0) ** np.arange(len(lo))) * lo[::-1]


def qmf_rec(lo):
    lo = np.asarray(lo, dtype=np.float64)
    return ((-1.0) ** np.arange(len(lo))) * lo[::-1]


class WrongEngine(OracleLevelEngine):
    """The oracle engine with one filter relation of an orthogonal bank used where the bank's own filter is meant."""

    def __init__(self, kind, wavelet):
        self.kind = kind
        self.bank = [np.asarray(f, dtype=np.float64) for f in O.filter_bank(wavelet)]

    def analysis(self, x, dec_lo, dec_hi, mode_id):
        if self.kind == "b":
            dec_hi = qmf_dec(dec_lo)
        return super().analysis(x, dec_lo, dec_hi, mode_id)

    def analysis_adjoint(self, g_buf, sig_shape, dec_lo, dec_hi, mode_id):
        if self.kind == "a":  # the synthesis with rec_*: the adjoint's index arithmetic with the flipped rec taps in place of the dec taps
            dec_lo, dec_hi = self.bank[2][::-1], self.bank[3][::-1]
        if self.kind == "b":
            dec_hi = qmf_dec(dec_lo)
        return super().analysis_adjoint(g_buf, sig_shape, dec_lo, dec_hi, mode_id)

    def synthesis(self, approx, details, rec_lo, rec_hi, out_extent):
        if self.kind == "b":
            rec_hi = qmf_rec(rec_lo)
        if self.kind == "c":
            rec_lo, rec_hi = self.bank[0][::-1], self.bank[1][::-1]
        return super().synthesis(approx, details, rec_lo, rec_hi, out_extent)

    def synthesis_adjoint(self, g_y, coef_shape, rec_lo, rec_hi):
        if self.kind == "b":
            rec_hi = qmf_rec(rec_lo)
        if self.kind == "c":
            rec_lo, rec_hi = self.bank[0][::-1], self.bank[1][::-1]
        return super().synthesis_adjoint(g_y, coef_shape, rec_lo, rec_hi)


# what each wrong engine spoils: the tensors of a run whose error must exceed 1e-2 with an independent bank
# (c: the gradients of the leaves come from the synthesis adjoint or, in 1-D, from a zero-mode analysis with the reversed rec taps —
# wrong or right by the route, so nothing is said about them)
SPOILS = {"a": ("gx",), "b": ("coeffs", "gx", "rec", "gleaves"), "c": ("rec",)}
UNSAID = {"a": (), "b": (), "c": ("gleaves",)}
SHAPES = [("wavedec", (3, 64), 2), ("wavedec2", (2, 30, 33), 2), ("fswavedec2", (2, 31, 30), 1), ("wavedec3", (1, 20, 21, 22), 1)]


@pytest.fixture()
def harness():
    """The harness on the CPU at the GPU module's bounds; the engine is put back and the routing memos are dropped afterwards."""
    keep = _engine.ENGINE
    h = D.Harness(T.BOUNDS, device="cpu")
    yield h
    _engine.ENGINE = keep
    for memo in _engine._routing_caches:
        memo.clear()


def errors(h, case):
    """Norm-wise error per tensor group of the harness's last run against the case's reference."""
    want, got = h.reference(case)[1], h.last

    def rel(a, b):
        return float(G.relerr(a.double().numpy(), b.double().numpy()))

    return {"coeffs": max(rel(a, b) for a, b in zip(got["coeffs"], want["coeffs"])), "gx": rel(got["gx"], want["gx"]),
            "rec": rel(got["rec"], want["rec"]), "gleaves": max(rel(a, b) for a, b in zip(got["gleaves"], want["gleaves"]))}


def cases_of(wavelet_of):
    out = []
    for i, (fn, shape, level) in enumerate(SHAPES):
        for j, mode in enumerate(MODES5):
            if (i + j) % 2 == 0 or mode == "zero":  # (every mode on every other shape; zero mode everywhere)
                out.append(D.Case(fn, shape, wavelet_of(i, j), mode, level, f64, None, 10 * i + j))
    return out


def test_orthogonal_relations_are_exact_for_the_named_banks():
    """rec = flip(dec) and the quadrature-mirror relation hold bit for bit in the committed orthogonal banks: what makes the three wrong
    engines right for them."""
    for name in ("haar", "db4", "sym5", "coif5", "db10"):
        lo, hi, rlo, rhi = O.filter_bank(name)
        assert np.array_equal(rlo, lo[::-1]) and np.array_equal(rhi, hi[::-1]), name
        assert np.array_equal(hi, qmf_dec(lo)) and np.array_equal(rhi, qmf_rec(rlo)), name


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_wrong_engines_pass_with_orthogonal_wavelets(harness, kind):
    """The blind spot: with db4 / sym5 each wrong engine passes every comparison of the harness at the float64 bounds."""
    for case in cases_of(lambda i, j: ("db4", "sym5")[(i + j) % 2]):
        _engine.ENGINE = WrongEngine(kind, case.wavelet)
        harness.run(case)
        assert max(errors(harness, case).values()) < T.F64_BOUNDS["norm"], (kind, case[:2], case[3:])
    assert not harness.raised


@pytest.mark.parametrize("kind", ["a", "b", "c"])
def test_wrong_engines_fail_with_independent_banks(harness, kind):
    """With four independent filters (the banks of the GPU module) each wrong engine fails the harness, by more than 1e-2 on every tensor
    it spoils — and is exact on the tensors it does not touch."""
    for case in cases_of(lambda i, j: T.bank((2, 4, 6, 8, 10)[(i + j) % 5], 50 + 7 * i + j)):
        _engine.ENGINE = WrongEngine(kind, case.wavelet)
        with pytest.raises(AssertionError):
            harness.run(case)
        err = errors(harness, case)
        for key, v in err.items():
            if key in SPOILS[kind]:
                assert v > 1e-2, (kind, key, v, case[:2], case[3:])
            elif key not in UNSAID[kind]:
                assert v < T.F64_BOUNDS["norm"], (kind, key, v, case[:2], case[3:])


def test_the_correct_engine_passes_with_independent_banks(harness):
    """The harness itself, the library's host logic and the oracle engine are right with such banks (lengths 2 .. 20)."""
    _engine.ENGINE = OracleLevelEngine()
    for case in cases_of(lambda i, j: T.bank((2, 4, 6, 8, 10, 16, 20)[(3 * i + j) % 7], 90 + 7 * i + j)):
        harness.run(case)
    assert not harness.raised and len(harness.ran) == len(cases_of(lambda i, j: "db4"))


def _flat(c):
    return [np.asarray(t.detach().numpy() if hasattr(t, "detach") else t) for _, t in G.flatten_coeffs(c)]


@pytest.mark.parametrize("fn,shape", [("wavedec", (2, 47)), ("wavedec2", (2, 46, 45)), ("fswavedec2", (1, 45, 46)), ("wavedec3", (1, 24, 25, 26)),
                                      ("fswavedec3", (1, 25, 24, 26))])
def test_the_two_references_agree_with_independent_banks(fn, shape):
    """oracle/fwt_oracle.py (numpy) against oracle/torch_autograd_ref.py (torch conv) with independent banks: analysis and synthesis,
    1-D to 3-D and the separable containers, five modes, 2 .. 20 taps, to 1e-12 (measured 1.2e-15)."""
    rec = D.FNS[fn][0]
    worst = 0.0
    for i, flen in enumerate((2, 4, 6, 8, 10, 16, 20)):
        wavelet = T.bank(flen, 200 + i)
        x = D.gaussian(shape, 300 + i, f64)
        for mode in MODES5:
            level = 2 if min(shape[1:]) >= 4 * flen else 1
            a = getattr(O, fn)(x.numpy(), wavelet, mode=mode, level=level)
            b = getattr(R, fn)(x, wavelet, mode=mode, level=level)
            for u, v in zip(_flat(a), _flat(b)):
                assert u.shape == v.shape
                worst = max(worst, float(G.relerr(v, u)))
            ya, yb = getattr(O, rec)(a, wavelet), getattr(R, rec)(b, wavelet)
            worst = max(worst, float(G.relerr(yb.numpy(), np.asarray(ya))))
    assert worst < 1e-12, worst


def test_the_table_covers_what_it_claims():
    T.test_the_table_covers_what_it_claims()


def test_the_float32_yardstick_lists_every_float32_row_once():
    cases = T.f32_cases()
    assert len(cases) == len(set(cases)) and all(c.dtype == f32 for c in cases)
    assert set(cases) == {r.case for r in T.ROWS if r.case.dtype == f32}
    assert T.F32_BOUNDS == {k: 10 * v for k, v in T.F32_REF.items()} and T.F64_BOUNDS == T.G.F64_BOUNDS
    w = T.measure_f32_reference([D.Case("wavedec2", (2, 20, 22), T.bank(4, 1), "symmetric", 1, f32)], verbose=False)
    assert set(w) == set(D.MEASURES) and all(1e-9 < v < 5e-6 for v in w.values()), w
