"""GPU tests (``-m gpu``) of the boundary-mode wavelet packets: ``WaveletPacket`` / ``WaveletPacket2D`` with ``mode="boundary"`` and
the packet-subtree kernels behind the 1-D class (csrc/mifwt_bwt_tree.hip, ids 32 / 33).

References: the reference library's goldens (tests/golden/ptwt_ref_boundary_packets.npz) for the classes, and for the kernels the
float64 host chain of tests/_boundary_tree_ref.py (the host level operators applied node by node on the CPU; pinned to the same
goldens by tests/test_boundary_packets_host.py).  Every tree of TREES runs on the default route and with
``_bwt.FORCE_PER_LEVEL_TREE``; both meet the same bound against the same reference and are never compared with each other.

Bounds, norm-wise per level buffer (tests/_golden.relerr): float64 1e-12.  float32: ten times the largest deviation of the FLOAT32
host chain (operator entries rounded to float32, float32 tensors, the CPU's own summation order) from the float64 chain on the same
float32 inputs, over this module's own cases — ``python -m tests.test_gpu_boundary_packets`` prints them (CPU only):

  trees(), analysis levels                            2.52e-7 (cap-db1: 2 x 8192, depth 13)    bound 2.52e-6
  trees(), reconstruct() from random leaves           2.48e-7 (cap-db1)                        bound 2.48e-6
  32 x 4096 db4 depth 6: |E(leaves) - E(x)| / E(x)    1.27e-7                                  bound 1.27e-6
  32 x 4096 db4 depth 6: reconstruct() against x      2.27e-7                                  bound 2.27e-6
(every other tree of trees() is between 6.6e-8 and 2.5e-7 in both directions.)

The autouse fixture empties ``_bwt.PER_LEVEL_TREE_CELLS``: the module tests the subtree kernels whatever the measured routing table sends
to them by default.
"""
import zlib

import numpy as np
import pytest
import torch

import ptwt_amd
from ptwt_amd import _bwt, _engine
from ptwt_amd._wavelets import host_taps
from tests import _boundary_tree_ref as T
from tests import _golden as G

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
CAP = {F32: 8192, F64: 4096}
# worst errors of the float32 host chain against the float64 chain (measure_reference_f32 below, CPU)
F32_REF = {"fwd": 2.52e-7, "inv": 2.48e-7, "energy": 1.27e-7, "round trip": 2.27e-7}
F32_FACTOR = 10.0


@pytest.fixture(autouse=True)
def subtree_route(monkeypatch):
    """Every cell of the envelope on the subtree kernels, whatever ``_bwt.PER_LEVEL_TREE_CELLS`` routes by default today."""
    monkeypatch.setattr(_bwt, "PER_LEVEL_TREE_CELLS", set())


def dev():
    return torch.device("cuda:0")


def tag(dt):
    return "f32" if dt == F32 else "f64"


def tol(dtype, what):
    return 1e-12 if dtype == F64 else F32_FACTOR * F32_REF[what]


def _depth_at_cap(dtype, flen):
    return _bwt.tree_levels(dtype, flen, CAP[dtype], 16)


def trees(dtype):
    """(name, rows, n, wavelet, depth, launches of the analysis, launches of reconstruct()) on the default route."""
    out = []
    for w in ("db1", "db2", "db4", "db10"):
        flen = len(host_taps(w)[0])
        out.append(("touch-" + w, 3, 4 * 2 * (flen - 1), w, 3, [32], [33]))            # the ends of the deepest expanded node touch
        out.append(("cap-" + w, 2, CAP[dtype], w, _depth_at_cap(dtype, flen), [32], [33]))
    out.append(("13x16", 3, 13 * 16, "db2", 5, [32, 26], [27, 33]))                     # 208 .. 26 fused, the nodes of 13 per level
    for rows in (1, 3, 600):
        out.append(("rows%d" % rows, rows, 128, "db4", 4, [32], [33]))
    out.append(("twice-cap", 2, 2 * CAP[dtype], "db4", 6, [26, 32], [33, 27]))
    out.append(("odd67", 2, 67, "db2", 3, [26, 26, 26], [27, 27, 27]))                 # 67 -> 34 -> 17 -> 9: never two even levels
    return out


TREE_NAMES = [t[0] for t in trees(F32)]
_REF = {}


def reference(dtype, name):
    """Inputs (quantised to ``dtype``) and the float64 chain's results of a tree of TREES; computed once."""
    key = (dtype, name)
    if key not in _REF:
        _, rows, n, w, depth, _, _ = next(t for t in trees(dtype) if t[0] == name)
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
        taps = host_taps(w)
        x = torch.randn(rows, n, generator=g, dtype=F64).to(dtype)
        levels = T.packet_levels(x.double(), taps, depth)
        leaves = torch.randn(levels[-1].shape, generator=g, dtype=F64).to(dtype)
        lengths = [n] + [int(b.shape[-1]) for b in levels[:-1]]
        rec = T.packet_rec(leaves.double(), taps, lengths)
        _REF[key] = (x, levels, leaves, rec)
    return _REF[key]


def _run_tree(dtype, name, forced, monkeypatch):
    _, rows, n, w, depth, fwd_ids, inv_ids = next(t for t in trees(dtype) if t[0] == name)
    x, levels, leaves, rec = reference(dtype, name)
    monkeypatch.setattr(_bwt, "FORCE_PER_LEVEL_TREE", forced)
    _engine.level_events = []
    try:
        wp = ptwt_amd.WaveletPacket(x.to(dev()), w, mode="boundary", maxlevel=depth)
        keys = wp.get_level(depth, "natural")
        wp[keys[-1]]
        fwd_seen = [e[1] for e in _engine.level_events]
        got_levels = [wp._levels[i + 1] for i in range(depth)]
        for i, key in enumerate(keys):
            wp[key] = leaves[:, i].to(dev())
        del _engine.level_events[:]
        wp.reconstruct()
        inv_seen = [e[1] for e in _engine.level_events]
        got_rec = [wp._levels[i] for i in range(depth)]
        torch.cuda.synchronize()
    finally:
        _engine.level_events = None
    if forced:
        assert fwd_seen == [26] * depth and inv_seen == [27] * depth, (name, fwd_seen, inv_seen)
    else:
        assert fwd_seen == fwd_ids and inv_seen == inv_ids, (name, fwd_seen, inv_seen)
    for i in range(depth):
        a, b = got_levels[i].reshape(rows, 2 << i, -1), levels[i]
        assert a.dtype == dtype and tuple(a.shape) == tuple(b.shape), (name, i)
        e = G.relerr(a.cpu().numpy(), b.numpy())
        print("%s %s forced=%d analysis level %d: %.2e" % (name, tag(dtype), forced, i + 1, e))
        assert e < tol(dtype, "fwd"), (name, "analysis level", i + 1, e)
    for i in range(depth):
        a, b = got_rec[i].reshape(rows, 1 << i, -1), rec[i]
        assert tuple(a.shape) == tuple(b.shape), (name, i)
        e = G.relerr(a.cpu().numpy(), b.numpy())
        print("%s %s forced=%d reconstructed level %d: %.2e" % (name, tag(dtype), forced, i, e))
        assert e < tol(dtype, "inv"), (name, "reconstructed level", i, e)


@pytest.mark.parametrize("forced", [False, True], ids=["default-route", "per-level"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=tag)
@pytest.mark.parametrize("name", TREE_NAMES)
def test_trees_against_the_float64_host_chain(name, dtype, forced, monkeypatch):
    _run_tree(dtype, name, forced, monkeypatch)


def test_packets_vs_reference_goldens():
    z, idx = G.load("ptwt_ref_boundary_packets.npz")
    for case in idx:
        k = case["key"]
        kw = {a: (tuple(v) if isinstance(v, list) else v) for a, v in case["kw"].items()}
        x = torch.from_numpy(z[k + "_x"]).to(dev())
        cls = ptwt_amd.WaveletPacket if case["dim"] == 1 else ptwt_amd.WaveletPacket2D
        for orth in ("gramschmidt", "qr"):
            wp = cls(x, case["wavelet"], mode="boundary", maxlevel=case["maxlevel"], orthogonalization=orth, **kw)
            for key in case["keys"]:
                want = z["%s_n_%s" % (k, key)]
                got = wp[key]
                assert tuple(got.shape) == want.shape, (case, key)
                assert G.relerr(got.cpu().numpy(), want) < 1e-12, (case, key)
            for key in case["keys"]:
                wp[key] = 0.5 * wp[key]
            wp.reconstruct()
            want = z[k + "_rec"]
            assert tuple(wp[""].shape) == want.shape, case
            assert G.relerr(wp[""].cpu().numpy(), want) < 1e-12, (case, "reconstruct")


@pytest.mark.parametrize("dtype", [F64, F32], ids=tag)
def test_strided_and_misaligned_rows(dtype):
    """An input view whose row stride exceeds n (16-byte loads still legal) and one at an odd element offset (scalar staging)."""
    taps = host_taps("db4")
    bk = _bwt.bank(taps, "qr", "analysis")
    wide = torch.randn(5, 264, dtype=F64).to(dtype)
    on_dev = wide.to(dev())
    for rows, cols in ((slice(None), slice(0, 256)), (slice(None), slice(3, 259)), (slice(1, 2), slice(8, 264))):
        want = T.tree_fwd(wide[rows, cols].double(), taps, 4)
        got = _bwt.rows_tree(on_dev[rows, cols], bk, 4)
        for a, b in zip(got, want):
            assert G.relerr(a.cpu().numpy(), b.numpy()) < tol(dtype, "fwd")


@pytest.mark.parametrize("dtype", [F64, F32], ids=tag)
def test_tree_expanded_in_two_steps(dtype):
    """Depth 2 first, depth 5 afterwards: the second launch runs on B * 4 rows of n / 4 samples."""
    taps = host_taps("db3")
    x = torch.randn(3, 1280, dtype=F64, generator=torch.Generator().manual_seed(3)).to(dtype)
    want = T.packet_levels(x.double(), taps, 5)
    _engine.level_events = []
    try:
        wp = ptwt_amd.WaveletPacket(x.to(dev()), "db3", mode="boundary", maxlevel=5)
        wp["ad"]
        first = [(e[1], e[2]) for e in _engine.level_events]
        wp["daada"]
        both = [(e[1], e[2]) for e in _engine.level_events]
    finally:
        _engine.level_events = None
    assert first == [(32, (1280,))] and both == [(32, (1280,)), (32, (320,))]
    for depth, buf in ((2, want[1]), (5, want[4])):
        for i, key in enumerate(wp.get_level(depth, "natural")):
            assert G.relerr(wp[key].cpu().numpy(), buf[:, i].numpy()) < tol(dtype, "fwd"), key


@pytest.mark.parametrize("dtype", [F64, F32], ids=tag)
def test_round_trip_and_orthogonality(dtype):
    x = torch.randn(32, 4096, dtype=F32, generator=torch.Generator().manual_seed(1)).to(device=dev(), dtype=dtype)
    wp = ptwt_amd.WaveletPacket(x, "db4", mode="boundary", maxlevel=6)
    leaves = torch.stack([wp[k] for k in wp.get_level(6, "natural")], 1)
    e_x, e_c = float(x.double().pow(2).sum()), float(leaves.double().pow(2).sum())
    print("energy %s: %.2e" % (tag(dtype), abs(e_c - e_x) / e_x))
    assert abs(e_c - e_x) / e_x < tol(dtype, "energy")
    wp.reconstruct()
    e = G.relerr(wp[""].cpu().numpy(), x.cpu().numpy())
    print("round trip %s: %.2e" % (tag(dtype), e))
    assert wp[""] is not x and e < tol(dtype, "round trip")


def test_routing_is_one_launch_inside_the_envelope_and_per_level_outside():
    def ids(shape, wavelet, depth, dtype=F32):
        _engine.level_events = []
        try:
            wp = ptwt_amd.WaveletPacket(torch.randn(*shape, dtype=dtype, device=dev()), wavelet, mode="boundary", maxlevel=depth)
            wp["a" * depth]
            fwd = [e[1] for e in _engine.level_events]
            del _engine.level_events[:]
            wp.reconstruct()
            return fwd, [e[1] for e in _engine.level_events]
        finally:
            _engine.level_events = None

    assert ids((4, 1024), "db4", 6) == ([32], [33])
    assert ids((4, 4096), "db4", 6, F64) == ([32], [33])
    assert ids((2, 16384), "db4", 3) == ([26, 32], [33, 27])
    assert ids((2, 1024), "db11", 2) == ([28, 28], [29, 29])     # 22 taps: the generic passes
    assert ids((2, 67), "db2", 3) == ([26] * 3, [27] * 3)
    # an assigned node in the middle ends the run
    _engine.level_events = []
    try:
        wp = ptwt_amd.WaveletPacket(torch.randn(2, 1024, device=dev()), "db4", mode="boundary", maxlevel=4)
        wp["aa"]
        wp["ad"] = torch.zeros_like(wp["ad"])
        del _engine.level_events[:]
        wp["adda"]
        assert [e[1] for e in _engine.level_events] == [32]
        assert float(wp["adda"].abs().max()) == 0.0 and float(wp["aada"].abs().max()) > 0.0
    finally:
        _engine.level_events = None


class _GuardedTorch:
    """Stands in for ``torch`` inside ``_bwt``: ``empty`` on a device carves the tensor out of a block filled with a byte pattern
    (the pattern of tests/test_gpu_boundary.py)."""

    GUARD, PATTERN = 4096, 0xA5

    def __init__(self):
        self.blocks, self.shift = [], 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, shape, dtype=None, device=None):
        esize = torch.empty(0, dtype=dtype).element_size()
        n = int(np.prod(shape))
        self.shift = (self.shift + 1) % 4
        lead = self.GUARD + 256 * self.shift + esize * (self.shift % 2)  # (every other block starts off a 16-byte boundary)
        raw = torch.full((lead + n * esize + self.GUARD,), self.PATTERN, dtype=torch.uint8, device=device)
        self.blocks.append((raw, lead, n * esize))
        return raw[lead: lead + n * esize].view(dtype).view(tuple(shape))

    def check(self, what):
        torch.cuda.synchronize()
        assert self.blocks, what
        for raw, lead, nbytes in self.blocks:
            assert bool((raw[:lead] == self.PATTERN).all()), f"{what}: bytes BEFORE a {nbytes}-byte allocation were written"
            assert bool((raw[lead + nbytes:] == self.PATTERN).all()), f"{what}: bytes AFTER a {nbytes}-byte allocation were written"
        self.blocks.clear()


@pytest.mark.parametrize("dtype", [F32, F64], ids=tag)
def test_guard_bands_around_every_level_buffer(monkeypatch, dtype):
    guard = _GuardedTorch()
    for w, n, k in (("db1", 4, 2), ("db2", 24, 3), ("db4", 56, 3), ("db10", 152, 3), ("db4", CAP[dtype], _depth_at_cap(dtype, 8)),
                    ("db2", 13 * 16, 4)):
        taps = host_taps(w)
        fwd, inv = _bwt.bank(taps, "qr", "analysis"), _bwt.bank(taps, "qr", "synthesis")
        assert _bwt.tree_levels(dtype, len(taps[0]), n, k) == k
        x = guard.empty((3, n), dtype=dtype, device=dev())
        x.copy_(torch.randn(3, n, device=dev(), dtype=dtype))
        x_before = x.clone()
        want = _bwt.rows_tree(x, fwd, k)
        want_y = _bwt.transposed_tree(want[-1], inv, k)
        monkeypatch.setattr(_bwt, "torch", guard)
        try:
            got = _bwt.rows_tree(x, fwd, k)
            got_y = _bwt.transposed_tree(got[-1], inv, k)
        finally:
            monkeypatch.setattr(_bwt, "torch", torch)
        assert len(guard.blocks) == 1 + 2 * k
        guard.check((w, n, k, dtype))
        assert torch.equal(x, x_before)
        assert all(torch.equal(a, b) for a, b in zip(got + got_y, want + want_y))
        ref = T.tree_fwd(x.double().cpu(), taps, k)
        assert all(G.relerr(a.cpu().numpy(), b.numpy()) < tol(dtype, "fwd") for a, b in zip(got, ref))


def test_capture_replays_bit_identically_and_steady_state_has_no_sync():
    keys = ptwt_amd.WaveletPacket.get_level(4, "natural")

    def leaves(t):
        wp = ptwt_amd.WaveletPacket(t, "db3", mode="boundary", maxlevel=4)
        return [wp[k] for k in keys]

    def there_and_back(t):
        wp = ptwt_amd.WaveletPacket(t, "db3", mode="boundary", maxlevel=4)
        for k in keys:
            wp[k] = 0.5 * wp[k]
        return wp.reconstruct()[""]

    x0 = torch.randn(5, 1280, device=dev())
    x1 = torch.randn(5, 1280, device=dev())
    leaves(x0), there_and_back(x0)  # warm calls: the tables become resident
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = leaves(x1)
        back = there_and_back(x1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = ptwt_amd.capture(leaves, x0)(x1)
    assert len(got) == 16 and all(torch.equal(a, b) for a, b in zip(got, eager))
    assert torch.equal(ptwt_amd.capture(there_and_back, x0)(x1), back)


def test_gradients_run_level_by_level():
    x = torch.randn(2, 56, dtype=F64, device=dev(), requires_grad=True)

    def two_leaves(t):
        wp = ptwt_amd.WaveletPacket(t, "db4", mode="boundary", maxlevel=2)
        return wp["ad"], wp["da"]

    _engine.level_events = []
    try:
        two_leaves(x)
        assert [e[1] for e in _engine.level_events] == [26, 26]  # (without a gradient the same tree is one launch of id 32)
        del _engine.level_events[:]
        two_leaves(x.detach())
        assert [e[1] for e in _engine.level_events] == [32]
    finally:
        _engine.level_events = None
    assert torch.autograd.gradcheck(two_leaves, (x,), eps=1e-6, atol=1e-7)
    keys = ptwt_amd.WaveletPacket.get_level(2, "natural")
    leaf = [torch.randn(2, 14, dtype=F64, device=dev(), requires_grad=True) for _ in keys]

    def rebuilt(*ls):
        wp = ptwt_amd.WaveletPacket(x.detach(), "db4", mode="boundary", maxlevel=2)
        wp[keys[0]]
        for k, t in zip(keys, ls):
            wp[k] = t
        return wp.reconstruct()[""]

    _engine.level_events = []
    try:
        rebuilt(*leaf)
        assert [e[1] for e in _engine.level_events][-2:] == [27, 27]
    finally:
        _engine.level_events = None
    assert torch.autograd.gradcheck(rebuilt, tuple(leaf), eps=1e-6, atol=1e-7)


def measure_reference_f32():
    """The float32 host chain (operator entries rounded to float32, float32 tensors) against the float64 chain on the same float32
    inputs, over TREES and the round-trip case: the figures of F32_REF."""
    worst = {"fwd": 0.0, "inv": 0.0}
    for name, rows, n, w, depth, _, _ in trees(F32):
        x, levels, leaves, rec = reference(F32, name)
        taps = host_taps(w)
        lengths = [n] + [int(b.shape[-1]) for b in levels[:-1]]
        l32 = T.packet_levels(x, taps, depth, round32=True)
        r32 = T.packet_rec(leaves, taps, lengths, round32=True)
        assert l32[-1].dtype == F32 and r32[0].dtype == F32
        e_f = max(G.relerr(a.numpy(), b.numpy()) for a, b in zip(l32, levels))
        e_i = max(G.relerr(a.numpy(), b.numpy()) for a, b in zip(r32, rec))
        print("%-12s rows %4d n %6d %-5s depth %2d   analysis %.2e   reconstruct %.2e" % (name, rows, n, w, depth, e_f, e_i))
        worst["fwd"], worst["inv"] = max(worst["fwd"], e_f), max(worst["inv"], e_i)
    taps = host_taps("db4")
    x = torch.randn(32, 4096, dtype=F32, generator=torch.Generator().manual_seed(1))
    l32 = T.packet_levels(x, taps, 6, round32=True)
    e_x, e_c = float(x.double().pow(2).sum()), float(l32[-1].double().pow(2).sum())
    worst["energy"] = abs(e_c - e_x) / e_x
    back = T.packet_rec(l32[-1], taps, [4096 >> i for i in range(6)], round32=True)[0]
    worst["round trip"] = G.relerr(back.reshape(32, 4096).numpy(), x.numpy())
    print("F32_REF =", {k: float("%.2e" % v) for k, v in worst.items()})
    return worst


if __name__ == "__main__":
    measure_reference_f32()
