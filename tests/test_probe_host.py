"""CPU tests of the impulse-probe helpers (tests/_probe_ref.py) over the case table the GPU module imports.

What they establish, without a GPU: the element-wise bounds hold for an honest emulation of each kernel arithmetic at EVERY element
(nothing is masked out); every nonzero entry of every 1-D operator of the table is observable (zeroing it alone moves some element
of some probe image past its bound); each of the four mutations — a dropped end tap, a last tap that reads the other mirror rule's
sample, a truncating f16 store, flushed low halves of the matrix-core tap pairs — violates the bound, while the norm-wise metric of
the existing tests (tests/_golden.py relerr) stays under its limit for the dropped tap.  That last assertion states the gap.
"""
import numpy as np
import pytest
import torch

from oracle import fwt_oracle as O
from tests import _golden as G
from tests import _probe_ref as R

CASES = R.cases()
IDS = R.case_ids(CASES)


def test_half_spacing_is_numpy_spacing_of_the_larger_f16_neighbour():
    rng = np.random.default_rng(1)
    v = np.concatenate([np.exp(rng.uniform(np.log(1e-9), np.log(6e4), 4000)), [0.0, 2.0 ** -24, 2.0 ** -14, 1.0, 1.0 - 2.0 ** -12, 1024.0, 1024.5]])
    up = v.astype(np.float16)
    up = np.where(up.astype(np.float64) < v, np.nextafter(up, np.float16(np.inf)), up)
    want = np.where(v > 0, np.spacing(up).astype(np.float64) / 2, 0.0)
    got = R.half_spacing16(torch.from_numpy(v)).numpy()
    assert np.array_equal(got, want)
    # ... and it bounds the rounding error of every value of at most that magnitude
    assert np.all(np.abs(v.astype(np.float16).astype(np.float64) - v) <= got)
    x = torch.from_numpy(np.concatenate([v, -v]))
    t = R.trunc16(x)
    assert torch.all(t.abs() <= x.abs()) and torch.all((t - x).abs() < 2 * R.half_spacing16(x.abs()) + 1e-300)


@pytest.mark.parametrize("wavelet", sorted({c.wavelet for c in CASES if c.family.startswith("mfma")}))
def test_tap_pair_accuracy_is_absolute(wavelet):
    """The derived accuracy of the f16 tap pairs holds for every tap of the bank, and is NOT a relative (f32) accuracy for the end
    taps: that is what DESIGN 4.9 says now."""
    worst_rel = 0.0
    for t in O.filter_bank(wavelet):
        th, tl = R.pair16(t)
        err = np.abs(t - (th + tl))
        assert np.all(err <= R.pair16_err(t))
        worst_rel = max(worst_rel, float(np.max(err / np.abs(t))))
    if wavelet in ("db12", "db14", "sym16"):
        assert worst_rel > 100 * R.U32  # far from f32-accurate on the smallest taps


def _judge(job, got_fn):
    worst, nbad, where = 0.0, 0, ""
    for sl in R.chunks(job.x.shape[0]):
        st = job.bound(job.x[sl])
        r, i, bad = R.worst(got_fn(job.x[sl]), st)
        nbad += bad
        if r > worst:
            worst, where = r, job.where(i, st.want.shape)
    return worst, nbad, where


def _unresolvable_ok(op, arith, mode):
    """Entries below their own rounding resolution (R.resolvable_entries): only in constant mode, only in high-pass rows, only in the
    two border columns, at most three per operator."""
    lost = (np.abs(op.M) > 0) & ~R.resolvable_entries(op, arith)
    if arith is R.VEC64:  # float64 resolves everything but the 1e-17 residue of the window that lies wholly on the border sample
        lost &= np.abs(op.M) > 2 * op.L * R.U64 * np.abs(op.M).max()
        return not lost.any()
    if not lost.any():
        return True
    rows, cols = np.nonzero(lost)
    return mode == "constant" and op.kind == "analysis" and np.all(rows >= op.M.shape[0] // 2) and set(cols) <= {0, op.M.shape[1] - 1} and len(rows) <= 3


def _unseen(job, st):
    """Per operator of the job, the entries that NO element of the batch sees (R.seen_mask)."""
    x = job.x
    if job.op_r is None:
        seen = [R.seen_mask(job.op_c, x.abs().unsqueeze(1), st.err.unsqueeze(1))]
    else:
        mr, mc = torch.from_numpy(job.op_r.M), torch.from_numpy(job.op_c.M)
        seen = [R.seen_mask(job.op_c, R._apply(mr, x, -2).abs(), st.err),
                R.seen_mask(job.op_r, (x @ mc.T).abs().transpose(-1, -2), st.err.transpose(-1, -2))]
    ops = [job.op_c] if job.op_r is None else [job.op_c, job.op_r]
    return [int((R.resolvable_entries(o, job.case.arith) & ~s.numpy()).sum()) for o, s in zip(ops, seen)]


def _mutants(job):
    """name -> emulation of the job's batch with one fault built in."""
    case, mode = job.case, job.mode
    muts = {"a: smallest tap of each filter dropped": lambda: job.emulate(job.x, drop=R.smallest_taps(job.op_c))}
    if case.direction == 0 and mode in R.OTHER_MIRROR:
        other = R.OTHER_MIRROR[mode]
        oc = R.analysis_axis(case.wavelet, job.op_c.M.shape[1], mode, last_tap_mode=other)
        orr = R.analysis_axis(case.wavelet, job.op_r.M.shape[1], mode, last_tap_mode=other) if job.op_r is not None else None
        muts["b: last tap reads the other mirror rule's sample"] = lambda: job.emulate(job.x, ops=(orr, oc))
    if case.arith.store == "f16":
        muts["c: f16 store truncates toward zero"] = lambda: job.emulate(job.x, trunc=True)
    if case.arith.taps == "pair16":
        muts["d: low halves of the tap pairs flushed"] = lambda: job.emulate(job.x, flush_lo=True)
    return muts


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_bound_holds_sees_every_entry_and_every_mutation(case):
    """Per case of the table and per mode, on every probe batch (the one-impulse-per-image batch thinned to the images that still put an
    impulse into every row and column, R.thin_single):
      1. the honest emulation of the kernel's arithmetic violates the bound at NO element (nothing is masked out);
      2. coverage: zeroing any single entry of either 1-D operator moves at least one element past its bound — 0 unseen;
      3. on the first batch (the one-impulse-per-image plane; 1-D: n = 2 L + 1) and on the last (a seam plane; the longer signal) each
         mutation that applies violates the bound."""
    for mode in case.modes:
        batch = R.jobs(case, mode, thin=True)
        for job in batch:
            st = job.bound(job.x)
            ratio, idx, nbad = R.worst(job.emulate(job.x), st)
            assert nbad == 0 and ratio <= 1.0, (job.where(idx, st.want.shape), ratio, nbad)
            ops = [o for o in (job.op_c, job.op_r) if o is not None]
            assert all(_unresolvable_ok(o, case.arith, mode) for o in ops), (case.id, mode, job.label)
            unseen = _unseen(job, st)
            assert unseen == [0] * len(ops), (case.id, mode, job.label, unseen)
            if job is batch[0] or job is batch[-1]:  # the one-impulse-per-image plane (1-D: 2 L + 1) and the last seam plane (the longer signal)
                for name, fn in _mutants(job).items():
                    ratio, _, nbad = R.worst(fn(), st)
                    assert nbad > 0 and ratio > 1.0, (case.id, mode, job.label, name, ratio)


@pytest.mark.parametrize("wavelet", ["db9", "db10", "db12", "db14", "sym16"])
def test_the_old_metric_does_not_see_a_dropped_end_tap_f16(wavelet):
    """The gap: on the randn input of test_mfma_dwt2_long_filters_half the matrix-core arithmetic with the smallest tap of each filter
    set to zero stays under the 5e-4 of the f16 tests in every sub-band."""
    case = next(c for c in CASES if c.family == "mfma_fwd" and c.wavelet == wavelet)
    rng = np.random.default_rng(len(wavelet) + 200)
    flen = case.flen
    x = torch.from_numpy(rng.standard_normal((2, 131, 3 * flen + 70))).to(torch.float16).to(torch.float64)
    for mode in ("reflect", "symmetric", "zero"):
        op_r, op_c = R.fwd_op(wavelet, 131, mode), R.fwd_op(wavelet, 3 * flen + 70, mode)
        got = R.emulate_2d(x, op_r, op_c, case.arith, drop=R.smallest_taps(op_c)).numpy()
        want = O.wavedec2(x.numpy(), wavelet, mode=mode, level=1)
        mh, mw = want[0].shape[-2:]
        bands = {"a": got[:, :mh, :mw], "v": got[:, :mh, mw:], "h": got[:, mh:, :mw], "d": got[:, mh:, mw:]}
        for name, ref in zip("ahvd", (want[0],) + tuple(want[1])):
            assert G.relerr(bands[name], ref) < 5e-4, (wavelet, mode, name)


def test_the_old_metric_does_not_see_a_dropped_end_tap_f32_db14():
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.standard_normal((3, 1027)))
    for mode in ("reflect", "zero"):
        op = R.fwd_op("db14", 1027, mode)
        got = R.emulate_pass(x.float().double(), op, R.VEC32, -1, None, drop=R.smallest_taps(op)).numpy()
        a, d = O.wavedec(x.float().double().numpy(), "db14", mode=mode, level=1)
        assert G.relerr(got[:, : a.shape[-1]], a) < 1e-6 and G.relerr(got[:, a.shape[-1]:], d) < 1e-6


# ---- several levels in one launch (kernel ids 14 / 15, 17 / 18, 20) ---------------------------------------------------------------
CHAINS = R.chain_cases()


def _chain_jobs_host(case, mode):
    """The multi-level jobs of a case; of the 4000-row batches of the long-row cases the CPU tests keep the 64 probes next to either end
    and every 16th in between (the GPU tests run the complete A . I)."""
    out = R.chain_jobs(case, mode)
    for job in out:
        n = job.x.shape[0]
        if n > 2000:
            keep = sorted(set(range(64)) | set(range(n - 64, n)) | set(range(0, n, 16)))
            job.x = job.x[keep]
    return out


@pytest.mark.parametrize("case", CHAINS, ids=R.case_ids(CHAINS))
def test_multi_level_bound_holds_and_sees_the_mutations(case):
    """The recurrence over levels (R.ChainJob): the honest emulation — every level in the kernel's own precision, nothing rounded in
    between — is inside the bound at every element of every returned band; a dropped end tap and (analysis, mirror modes) a last tap
    reading the other mirror rule's sample violate it."""
    for mode in case.modes:
        for job in _chain_jobs_host(case, mode):
            st = job.bound(job.x)
            ratio, idx, nbad = R.worst(job.emulate(job.x), st)
            assert nbad == 0 and ratio <= 1.0, (job.where(idx, st.want.shape), ratio, nbad)
            ratio, _, nbad = R.worst(job.emulate(job.x, drop=R.smallest_taps(job.op_c)), st)
            assert nbad > 0 and ratio > 1.0, (case.id, mode, job.label, "a", ratio)
            if case.direction == 0 and mode in R.OTHER_MIRROR:
                honest = job.ops
                try:
                    job.ops = [[R.analysis_axis(case.wavelet, o.M.shape[1], mode, last_tap_mode=R.OTHER_MIRROR[mode]) for o in lvl] for lvl in honest]
                    ratio, _, nbad = R.worst(job.emulate(job.x), st)
                finally:
                    job.ops = honest
                assert nbad > 0 and ratio > 1.0, (case.id, mode, job.label, "b", ratio)


_CHAINS_1D = [c for c in CHAINS if c.ndim == 1]


@pytest.mark.parametrize("case", _CHAINS_1D, ids=R.case_ids(_CHAINS_1D))
def test_multi_level_every_operator_entry_is_observable(case):
    """Coverage of the 1-D multi-level cases.  Their operator is the multi-level one (the oracle called with level = k on the identity), and
    with the batch A . I every returned element IS one entry of it: zeroing the entry alone zeroes that element, so the entry is seen
    when its magnitude exceeds the element's bound.  0 unseen.  (The entries of the single levels' operators at levels 2 and 3 are not
    individually observable with these probes — those levels are fed low-pass images of the impulses, not impulses, and sym16's 3e-6
    end taps hide behind the larger taps of the same window; the single-level cases cover those operators.)"""
    for mode in case.modes:
        for job in _chain_jobs_host(case, mode):
            st = job.bound(job.x)
            entries = st.want != 0
            assert int(entries.sum()) > 0 and int((entries & (st.want.abs() <= st.err)).sum()) == 0, (case.id, mode, job.label)


def test_small_plane_route_takes_the_planes_of_the_table():
    """The planes of the small-plane pyramid cases are the smallest and the largest the engine's own plan sends to kernel 20 at 20 taps,
    two levels, for the lattice batch of 64 images (host query, nothing is launched)."""
    from ptwt_amd import _engine

    def route(h, w, mode):
        x = torch.empty((64, h, w), dtype=torch.float32, device="meta")
        plan = _engine.ENGINE._pyramid_plan(x, 20, _engine.MODE_IDS[mode], 2)[1]
        return plan[1], plan[3]

    for mode in R.ALL_MODES:
        for h, w in R.SMALL_PLANES[mode == "periodic"]:
            assert route(h, w, mode) == (2, _engine.KID_SMALL), (mode, h, w)
        assert route(77, 78, mode) != (2, _engine.KID_SMALL) and route(88, 88, mode) != (2, _engine.KID_SMALL)


def test_small_plane_reconstruction_route_takes_the_planes_of_the_table():
    """Likewise for the small-plane reconstruction (kernel 21): the two-level coefficient sets of 21 x 22 and 85 x 86 go to it for the
    batch of 7 x 64 images, those of 86 x 87 do not."""
    from ptwt_amd import _engine

    def route(h, w, flen=20, batch=7 * 64):
        sh, sw = R.level_sizes(h, flen, 2), R.level_sizes(w, flen, 2)
        meta = lambda k: torch.empty((batch, sh[k], sw[k]), dtype=torch.float32, device="meta")
        plan = _engine.ENGINE.synthesis_pyramid_plan(meta(2), [[meta(2)] * 3, [meta(1)] * 3], flen, (2 * sh[1] - flen + 2, 2 * sw[1] - flen + 2))
        return plan[3], plan[0].kid

    for h, w in R.SMALL_INV_PLANES:
        assert route(h, w) == (1, _engine.KID_INV_SMALL), (h, w)
    assert route(86, 87)[0] != 1


_SMALL = [c for c in CHAINS if c.ndim == 2]


@pytest.mark.parametrize("case", _SMALL, ids=R.case_ids(_SMALL))
def test_small_plane_probes_see_every_entry_of_the_finest_level(case):
    """Coverage of the small-plane pyramid cases: 0 unseen entries of the row and the column operator of the FINEST level, the one whose
    input (analysis) or output (reconstruction) the probes and the returned elements touch directly.
    Analysis (id 20): the lattice images are that level's input; its approximation band is not returned, so only the three detail
    bands may see an entry (a low-pass row of one operator shows in the band that is high-pass along the other axis).
    Reconstruction (id 21): the lattices in the three finest detail bands are direct inputs of that level (the approximation block
    is fed by the coarser level), and the whole output is returned."""
    a = case.arith
    for mode in case.modes:
        for job in R.chain_jobs(case, mode):
            if case.direction == 0:
                op_r, op_c = job.ops[0]
                x = job.x
                st = R.level_2d(R.State(x), op_r, op_c, a)
                mh, mw = job.sizes[0][1], job.sizes[1][1]
                err = st.err.clone()
                err[:, :mh, :mw] = float("inf")  # the approximation stays on chip
            else:
                op_r, op_c = job.ops[-1]
                sh, sw = job.sizes
                n = sh[1] * sw[1]
                fine = job.x[:, -3 * n:]
                keep = fine.abs().sum(dim=1) > 0  # the images whose lattice lies in a band of the finest level
                ad, da, dd = (fine[keep][:, b * n:(b + 1) * n].reshape(-1, sh[1], sw[1]) for b in range(3))
                x = torch.cat([torch.cat([torch.zeros_like(ad), ad], -1), torch.cat([da, dd], -1)], -2)
                full = job.bound(job.x)
                err = full.err[keep].reshape(-1, op_r.M.shape[0], op_c.M.shape[0])
            mr, mc = torch.from_numpy(op_r.M), torch.from_numpy(op_c.M)
            seen_c = R.seen_mask(op_c, R._apply(mr, x, -2).abs(), err).numpy()
            seen_r = R.seen_mask(op_r, (x @ mc.T).abs().transpose(-1, -2), err.transpose(-1, -2)).numpy()
            unseen = [int((R.resolvable_entries(op_c, a) & ~seen_c).sum()), int((R.resolvable_entries(op_r, a) & ~seen_r).sum())]
            assert unseen == [0, 0], (case.id, mode, job.label, unseen)
            assert all(_unresolvable_ok(o, a, mode) for o in (op_r, op_c)), (case.id, mode, job.label)
