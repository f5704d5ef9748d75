"""GPU impulse probes and out-of-bounds canaries of the bfloat16 kernels (``-m gpu``).

Entry by entry, as tests/test_gpu_probes.py does for float16: isolated impulses of 1.0 (a power of two: exact in bf16) through kernel
ids 7, 8, 11, 23 and the 1-D inner-axis kernels 3 / 4, EVERY output element against the float64 operator with the element-wise bound of
tests/_bf16_ref.py (bf16 stores, bf16 tap pairs with residual 2^-16 |t|; derived, not fitted), on the seam planes of tests/_probe_ref.py.
Canaries: one call per kernel id in bf16 on guarded allocations (the helpers of tests/test_gpu_canaries.py).
"""
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine
from ptwt_amd._wavelets import host_taps
from tests import _bf16_ref as B
from tests import _probe_ref as R
from tests.test_gpu_canaries import _run, _x, guarded  # noqa: F401  (the fixture and the guarded-call helper)
from tests.test_gpu_probes import _check, _padded_pitch, _stack2

pytestmark = pytest.mark.gpu

CASES = B.cases()
BF16 = torch.bfloat16


def dev():
    return torch.device("cuda:0")


def _pick(family):
    cs = [c for c in CASES if c.family == family]
    return pytest.mark.parametrize("case", cs, ids=R.case_ids(cs))


class _Route:
    """Options 6 / 7 and 16-bit storage for the duration of a test; the kernel ids of the levels it ran."""

    def __init__(self, case, mfma_mode=0):
        self.case, self.mfma_mode = case, mfma_mode

    def __enter__(self):
        ptwt_amd.set_half_storage(True)
        _engine.set_option(7, self.mfma_mode)
        return self

    def __exit__(self, *exc):
        _engine.set_option(6, 0)
        _engine.set_option(7, 0)
        _engine.level_events = None
        ptwt_amd.set_half_storage(False)

    def run(self, fn, tile_rows=0):
        _engine.set_option(6, tile_rows)
        _engine.level_events = []
        try:
            out = fn()
            torch.cuda.synchronize()
            kids = [e[1] for e in _engine.level_events]
        finally:
            _engine.level_events = None
            _engine.set_option(6, 0)
        assert kids == [self.case.kids[0]], (self.case.id, kids)
        return out


def _analysis2d(case, mfma_mode, tile_rows_list):
    worst = []
    with _Route(case, mfma_mode) as route:
        for mode in case.modes:
            for job in R.jobs(case, mode, device=dev()):
                st = B.bound(job, job.x)
                xin = job.x.to(BF16)
                runs = [(tr, xin) for tr in tile_rows_list]
                if mode == "periodic" and job.label.endswith("lattice"):  # (even extents: the odd pitch comes from a view one column wider)
                    wide = torch.zeros(*xin.shape[:-1], xin.shape[-1] + 1, dtype=BF16, device=xin.device)
                    wide[..., :-1] = xin
                    runs.append((tile_rows_list[0], wide[..., :-1]))
                for tr, xrun in runs:
                    n_walk = _engine.launch_count(_engine.VARIANT_FWD_MFMA_WALK)
                    aa, (da, ad, dd) = route.run(lambda: ptwt_amd.wavedec2(xrun, case.wavelet, mode=mode, level=1), tr)
                    if case.family == "mfma_fwd":
                        assert _engine.launch_count(_engine.VARIANT_FWD_MFMA_WALK) - n_walk == 1
                    assert aa.dtype == BF16
                    _check(job, _stack2(aa, ad, da, dd), st, "%s %s %s rows=%d pitch=%d" % (case.id, mode, job.label, tr, xrun.stride(-2)), worst)
                del st
    print("PROBE %s worst error/bound %.4f" % (case.id, max(worst)))


def _synthesis2d(case, mfma_mode, variants):
    worst = []
    lo, hi = host_taps(case.wavelet)[2:]
    with _Route(case, mfma_mode) as route:
        for job in R.jobs(case, case.modes[0], device=dev()):
            mh, mw, h, w = job.extra
            st = B.bound(job, job.x)
            z = job.x.to(BF16)
            for opt6, padded in variants:
                pitch = _padded_pitch(mw, 2) if padded else mw
                buf = torch.zeros(job.x.shape[0], 4, mh, pitch, dtype=BF16, device=dev())
                for s in range(4):  # plane s: bit 1 = high-pass along axis -2, bit 0 along axis -1
                    buf[:, s, :, :mw] = z[:, (s >> 1) * mh:(s >> 1) * mh + mh, (s & 1) * mw:(s & 1) * mw + mw]
                bands = [buf[:, s, :, :mw] for s in range(4)]
                got = route.run(lambda: _engine.ENGINE.synthesis(bands[0], bands[1:], lo, hi, [h, w]), opt6)
                assert got.dtype == BF16
                _check(job, got.double(), st, "%s %s option6=%d pitch=%d" % (case.id, job.label, opt6, pitch), worst)
            del st
    print("PROBE %s worst error/bound %.4f" % (case.id, max(worst)))


@_pick("mfma_fwd")
def test_mfma_analysis_entry_by_entry(case):
    """Kernel id 11 in bf16: every position of the smallest plane, lattices on the seam planes (three to four stacked tiles, three
    column panels, ragged; even and odd pitch of the rows in memory), all five modes."""
    _analysis2d(case, 0, [0])


@_pick("mfma_inv")
def test_mfma_synthesis_entry_by_entry(case):
    """Kernel id 23 in bf16 (option 7 = 4): impulses in each band in turn, the odd-extent trims, dense and padded pitches, segments of
    any length, of two tiles and of one."""
    _synthesis2d(case, 4, [(0, False), (0, True), (3, False), (2, False), (1, True)])


@_pick("tile_fwd")
def test_tile_analysis_entry_by_entry(case):
    """Kernel id 7 in bf16 (option 7 = 2 for the long bank): tile heights automatic, 8 and 24."""
    _analysis2d(case, 2, [0, 8, 24])


@_pick("tile_inv")
def test_tile_synthesis_entry_by_entry(case):
    """Kernel id 8 in bf16 (option 7 = 2), tile heights automatic, 8 and 24, dense and padded pitch."""
    _synthesis2d(case, 2, [(0, False), (8, True), (24, False)])


@pytest.mark.parametrize("case", [c for c in CASES if c.ndim == 1], ids=R.case_ids([c for c in CASES if c.ndim == 1]))
def test_inner_axis_kernels_entry_by_entry(case):
    """The 1-D streaming passes (ids 3 / 4) in bf16 with the 32-tap bank: the complete operator (batch = I) at n = 2 L + 1 and n = 301."""
    worst = []
    with _Route(case) as route:
        for mode in case.modes:
            for job in R.jobs(case, mode, device=dev()):
                st = B.bound(job, job.x)
                xin = job.x.to(BF16)
                if case.direction == 0:
                    a, d = route.run(lambda: ptwt_amd.wavedec(xin, case.wavelet, mode=mode, level=1))
                    got = torch.cat([a, d], -1)
                else:
                    m, n = job.extra
                    lo, hi = host_taps(case.wavelet)[2:]
                    a, d = xin[:, :m].contiguous(), xin[:, m:].contiguous()
                    got = route.run(lambda: _engine.ENGINE.synthesis(a, [d], lo, hi, [n]))
                assert got.dtype == BF16
                _check(job, got.double(), st, "%s %s %s" % (case.id, mode, job.label), worst)
    print("PROBE %s worst error/bound %.4f" % (case.id, max(worst)))


def test_canaries_one_call_per_kernel_id(guarded):  # noqa: F811
    """Guard bytes around every allocation a bf16 kernel writes, inputs unmodified, results equal to those on ordinary allocations:
    ids 11 / 23 (sym16), 7 / 8 (db4), 3 / 4 (1-D db4), 0 (30 taps) and the 1-D stationary kernel, at odd extents."""
    seen = set()

    def recording(fn):
        def run(*ts):
            out = fn(*ts)
            if _engine.level_events is not None:
                seen.update(e[1] for e in _engine.level_events)
            return out
        return run

    keys = ("ad", "da", "dd")
    with ptwt_amd.half_storage():
        for shape, wavelet, level in (((2, 300, 420), "sym16", 2), ((3, 130, 171), "db4", 2)):
            x = _x(*shape, dtype=BF16)
            c = _run(guarded, f"fswavedec2 bf16 {shape} {wavelet}", recording(lambda t: ptwt_amd.fswavedec2(t, wavelet, level=level)), [x])
            _run(guarded, f"fswaverec2 bf16 {shape} {wavelet}",
                 recording(lambda *ts: ptwt_amd.fswaverec2((ts[0], *[dict(zip(keys, ts[1 + 3 * k: 4 + 3 * k])) for k in range(level)]), wavelet)),
                 [c[0]] + [d[k] for d in c[1:] for k in keys])
        for wavelet in ("db4", "coif5"):
            x = _x(3, 1001, dtype=BF16)
            c = _run(guarded, f"wavedec bf16 {wavelet}", recording(lambda t: ptwt_amd.wavedec(t, wavelet, level=2)), [x])
            _run(guarded, f"waverec bf16 {wavelet}", recording(lambda *ts: ptwt_amd.waverec(list(ts), wavelet)), list(c))

        def both(t):
            c = ptwt_amd.swt(t, "db2", level=3)
            return torch.stack(c + [ptwt_amd.iswt(c, "db2")])
        _run(guarded, "swt / iswt 3 x 1001 bf16", both, [_x(3, 1001, dtype=BF16)])
    assert seen >= {0, 3, 4, 7, 8, 11, 23}, sorted(seen)
