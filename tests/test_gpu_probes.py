"""GPU impulse-probe tests (``-m gpu``): the long-filter and f16 kernels, entry by entry.

Every parity test judges a sub-band by one norm-wise error; that metric cannot see the outer taps of the 18..32-tap banks, a wrong
border sample or a truncating f16 store (tests/test_probe_host.py states the gap).  Here a kernel is fed isolated impulses and EVERY
output element is compared with the float64 operator (oracle/fwt_oracle.py applied to the identity) against the element-wise
worst-case bound of tests/_probe_ref.py — derived from the kernel's arithmetic, no empirical factor, nothing masked out.  The bound,
the reference product and the comparison run on the device in float64 (plain matmul).  Each test pins its route: the kernel id of
every level (``_engine.level_events``), the variant counter of the matrix-core walk, options 6 and 7 restored in ``finally``.
Each test prints the largest error / bound ratio it met (DESIGN.md section 2 records them).
"""
import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine
from ptwt_amd._wavelets import host_taps
from tests import _probe_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()


def dev():
    return torch.device("cuda:0")


def _pick(family):
    cs = [c for c in CASES if c.family == family]
    return pytest.mark.parametrize("case", cs, ids=R.case_ids(cs))


class _Route:
    """Options 6 / 7 / 12 and half storage for the duration of a test; the kernel ids of the levels it ran."""

    def __init__(self, case, mfma_mode=0):
        self.case, self.mfma_mode = case, mfma_mode

    def __enter__(self):
        if self.case.dtype == "f16":
            ptwt_amd.set_half_storage(True)
        _engine.set_option(7, self.mfma_mode)
        if self.case.family == "tile_fwd":  # the one-launch pyramid kernels (ids 16 / 20) would serve the small f32 planes first
            _engine.set_option(_engine.OPT_PYRAMID_MODE, 2)
        return self

    def __exit__(self, *exc):
        _engine.set_option(6, 0)
        _engine.set_option(7, 0)
        _engine.set_option(_engine.OPT_PYRAMID_MODE, 0)
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
        assert kids and all(k in self.case.kids for k in kids), (self.case.id, kids)
        return out, kids


def _check(job, got, st, what, worst_seen):
    assert tuple(got.shape) == tuple(st.want.shape), (what, got.shape, st.want.shape)
    ratio, idx, nbad = R.worst(got, st)
    worst_seen.append(ratio)
    assert nbad == 0 and ratio <= 1.0, "%s: %d elements outside their bound, worst error / bound = %.3f at %s" % (
        what, nbad, ratio, job.where(idx, st.want.shape))


def _stack2(aa, ad, da, dd):
    return torch.cat([torch.cat([aa, ad], -1), torch.cat([da, dd], -1)], -2).double()


def _analysis2d(case, mfma_mode, tile_rows_list):
    worst = []
    with _Route(case, mfma_mode) as route:
        for mode in case.modes:
            for job in R.jobs(case, mode, device=dev()):
                st = job.bound(job.x)
                xin = job.x.to(case.torch_dtype)
                runs = [(tr, xin) for tr in tile_rows_list]
                if mode == "periodic" and job.label.endswith("lattice"):
                    # the periodic seam plane has even extents (multiples of the lattice pitch): its odd pitch of the rows in memory
                    # comes from a view of a buffer one column wider
                    wide = torch.zeros(*xin.shape[:-1], xin.shape[-1] + 1, dtype=xin.dtype, device=xin.device)
                    wide[..., :-1] = xin
                    assert wide[..., :-1].stride(-2) % 2 == 1
                    runs.append((tile_rows_list[0], wide[..., :-1]))
                for tr, xrun in runs:
                    n_walk = _engine.launch_count(_engine.VARIANT_FWD_MFMA_WALK)
                    (aa, (da, ad, dd)), kids = route.run(lambda: ptwt_amd.wavedec2(xrun, case.wavelet, mode=mode, level=1), tr)
                    assert kids == [case.kids[0]], kids
                    if case.family == "mfma_fwd":  # id 11 is two kernels: the one that walks down column panels served the level
                        assert _engine.launch_count(_engine.VARIANT_FWD_MFMA_WALK) - n_walk == 1
                    assert aa.dtype == case.torch_dtype
                    _check(job, _stack2(aa, ad, da, dd), st, "%s %s %s rows=%d pitch=%d" % (case.id, mode, job.label, tr, xrun.stride(-2)), worst)
                del st
    print("PROBE %s worst error/bound %.4f" % (case.id, max(worst)))


def _padded_pitch(mw, esz):
    """Rows padded to the next multiple of 128 bytes, and by a whole 128 bytes where they are one already."""
    per = 128 // esz
    pitch = -(-mw // per) * per
    return pitch + per if pitch == mw else pitch


def _synthesis2d(case, mfma_mode, variants):
    """variants: (option 6, padded pitch).  The coefficient planes are views of one [B, 4, mh, pitch] buffer, as the engine's own
    analysis returns them (rows padded to 128 bytes) or dense."""
    worst = []
    lo, hi = host_taps(case.wavelet)[2:]
    esz = 2 if case.dtype == "f16" else 4
    with _Route(case, mfma_mode) as route:
        for job in R.jobs(case, case.modes[0], device=dev()):
            mh, mw, h, w = job.extra
            st = job.bound(job.x)
            z = job.x.to(case.torch_dtype)
            for opt6, padded in variants:
                pitch = _padded_pitch(mw, esz) if padded else mw
                buf = torch.zeros(job.x.shape[0], 4, mh, pitch, dtype=case.torch_dtype, device=dev())
                for s in range(4):  # plane s: bit 1 = high-pass along the columns' axis (-2), bit 0 along the rows' axis (-1)
                    buf[:, s, :, :mw] = z[:, (s >> 1) * mh:(s >> 1) * mh + mh, (s & 1) * mw:(s & 1) * mw + mw]
                bands = [buf[:, s, :, :mw] for s in range(4)]
                assert padded == (bands[0].stride(-2) != mw)
                got, kids = route.run(lambda: _engine.ENGINE.synthesis(bands[0], bands[1:], lo, hi, [h, w]), opt6)
                assert kids == [case.kids[0]], kids
                _check(job, got.double(), st, "%s %s option6=%d pitch=%d" % (case.id, job.label, opt6, pitch), worst)
            del st
    print("PROBE %s worst error/bound %.4f" % (case.id, max(worst)))


@_pick("mfma_fwd")
def test_mfma_analysis_entry_by_entry(case):
    """Kernel id 11 (banded-Toeplitz MFMA analysis, f16): every position of the smallest plane, lattices on the seam planes (three to
    four stacked tiles, three column panels, ragged; even and odd pitch of the rows in memory), all five modes."""
    _analysis2d(case, 0, [0])


@_pick("mfma_inv")
def test_mfma_synthesis_entry_by_entry(case):
    """Kernel id 23 (MFMA synthesis, option 7 = 4): impulses in each band in turn at the coefficient extents of the analysis planes,
    the odd-extent trims included; segment option 0 and 3, each with dense coefficient planes and with views of a padded pitch, and
    segments of two tiles and of one (the seam planes stack three tiles of 32 output rows: a seam between segments is crossed)."""
    _synthesis2d(case, 4, [(0, False), (0, True), (3, False), (3, True), (2, False), (1, True)])


@_pick("tile_fwd")
def test_tile_analysis_entry_by_entry(case):
    """Kernel id 7 (LDS tiles; f16 with option 7 = 2 for the long banks, and f32): tile heights automatic, 8 and 24; the seam plane
    spans three tiles of 24 rows and three of 64 columns, ragged."""
    _analysis2d(case, 2, [0, 8, 24])


@_pick("tile_inv")
def test_tile_synthesis_entry_by_entry(case):
    """Kernel id 8 (LDS-tile synthesis; f16 with option 7 = 2, and f32), tile heights automatic, 8 and 24, dense and padded pitch."""
    _synthesis2d(case, 2, [(0, False), (8, True), (24, False)])


def _axis1d(case):
    worst, served = [], set()
    with _Route(case) as route:
        for mode in case.modes:
            for job in R.jobs(case, mode, device=dev()):
                st = job.bound(job.x)
                xin = job.x.to(case.torch_dtype)
                if case.direction == 0:
                    (a, d), kids = route.run(lambda: ptwt_amd.wavedec(xin, case.wavelet, mode=mode, level=1))
                    got = torch.cat([a, d], -1)
                else:
                    m, n = job.extra
                    lo, hi = host_taps(case.wavelet)[2:]
                    a, d = xin[:, :m].contiguous(), xin[:, m:].contiguous()
                    got, kids = route.run(lambda: _engine.ENGINE.synthesis(a, [d], lo, hi, [n]))
                served.update(kids)
                assert got.dtype == case.torch_dtype
                _check(job, got.double(), st, "%s %s %s" % (case.id, mode, job.label), worst)
    print("PROBE %s (kernel ids %s) worst error/bound %.4f" % (case.id, sorted(served), max(worst)))


@_pick("axis_fwd")
def test_axis_analysis_entry_by_entry(case):
    """The 1-D analysis pass, f16 / f32 / f64, the complete operator (batch = A . I) at n = 2 L + 1 and n = 301.  sym16 (32 taps) is
    served by the streaming kernel (id 3); db14 (28 taps) is not instantiated there and is served by the generic kernel (id 0)."""
    _axis1d(case)


@_pick("axis_inv")
def test_axis_synthesis_entry_by_entry(case):
    """The 1-D synthesis pass (id 4 for sym16, the generic kernel for db14), unit coefficient vectors, the odd-length trim."""
    _axis1d(case)


@_pick("generic_fwd")
def test_generic_analysis_entry_by_entry(case):
    """Kernel id 0 with coif17: 102 taps down to 1e-22, n = 205 (and 2 L + 1), f64 and f32."""
    _axis1d(case)


@_pick("generic_inv")
def test_generic_synthesis_entry_by_entry(case):
    _axis1d(case)


# ---- several levels in one launch: ids 14 / 15 (1-D tails), 17 / 18 (1-D long rows), 20 / 21 (small-plane pyramids) -----------------------
CHAINS = R.chain_cases()


def _pick_chain(family):
    cs = [c for c in CHAINS if c.family == family]
    return pytest.mark.parametrize("case", cs, ids=R.case_ids(cs))


def _chain(case):
    """The public multi-level call on the probe batch against the oracle called with level=k and the bound of the recurrence over levels
    (R.ChainJob); ONE launch of the named kernel must have served every level."""
    worst = []
    with _Route(case) as route:
        for mode in case.modes:
            for job in R.chain_jobs(case, mode, device=dev()):
                st = job.bound(job.x)
                xin = job.x.to(case.torch_dtype)
                if case.ndim == 2 and case.direction == 1:
                    (sh, sw), k = job.sizes, case.levels
                    parts, off = [xin[:, : sh[k] * sw[k]].reshape(-1, sh[k], sw[k]).contiguous()], sh[k] * sw[k]
                    for lv in range(k, 0, -1):
                        n = sh[lv] * sw[lv]
                        ad, da, dd = (xin[:, off + b * n: off + (b + 1) * n].reshape(-1, sh[lv], sw[lv]).contiguous() for b in range(3))
                        off += 3 * n
                        parts.append((da, ad, dd))
                    y, kids = route.run(lambda: ptwt_amd.waverec2(tuple(parts), case.wavelet))
                    got = y.flatten(1)
                elif case.ndim == 2:
                    c, kids = route.run(lambda: ptwt_amd.wavedec2(xin, case.wavelet, mode=mode, level=case.levels))
                    got = torch.cat([c[0].flatten(1)] + [b.flatten(1) for lvl in c[1:] for b in (lvl[1], lvl[0], lvl[2])], -1)
                elif case.direction == 0:
                    c, kids = route.run(lambda: ptwt_amd.wavedec(xin, case.wavelet, mode=mode, level=case.levels))
                    got = torch.cat(list(c), -1)
                else:
                    s, k = job.sizes[0], case.levels
                    coeffs = list(torch.split(xin, [s[k]] + [s[i] for i in range(k, 0, -1)], dim=-1))
                    got, kids = route.run(lambda: ptwt_amd.waverec([t.contiguous() for t in coeffs], case.wavelet))
                assert kids == [case.kids[0]], (case.id, mode, job.label, kids)
                assert got.dtype == case.torch_dtype
                _check(job, got.double(), st, "%s %s %s" % (case.id, mode, job.label), worst)
    print("PROBE %s worst error/bound %.4f" % (case.id, max(worst)))


@_pick_chain("tail_fwd")
def test_tail_analysis_three_levels_entry_by_entry(case):
    """Kernel id 14: three levels of n = 1001 in one launch, f32 and f64, the complete operator (A . I)."""
    _chain(case)


@_pick_chain("tail_inv")
def test_tail_synthesis_three_levels_entry_by_entry(case):
    """Kernel id 15: unit vectors in every coefficient of a three-level set of n = 1001 (odd extents: trims between the levels)."""
    _chain(case)


@_pick_chain("long_fwd")
def test_long_rows_analysis_entry_by_entry(case):
    """Kernel id 17: rows of 4101 samples (the chunked route starts at 4096; no multiple of a chunk), three levels in one launch."""
    _chain(case)


@_pick_chain("long_inv")
def test_long_rows_synthesis_entry_by_entry(case):
    """Kernel id 18: two levels back to rows of 4102 samples in one launch."""
    _chain(case)


@_pick_chain("small_fwd")
def test_small_plane_pyramid_entry_by_entry(case):
    """Kernel id 20: two levels of the smallest (21 x 22) and the largest (76 x 77) plane the route takes at 20 taps, lattice probes."""
    _chain(case)


@_pick_chain("small_inv")
def test_small_plane_reconstruction_entry_by_entry(case):
    """Kernel id 21: two levels back to 22 x 22 and 86 x 86 samples in one launch — the coefficient extents of the smallest plane and of
    the largest the route takes at 20 taps — with a lattice of impulses in each of the seven bands in turn."""
    _chain(case)
