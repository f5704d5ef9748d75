"""``_engine.level_events``: one tuple ``(tag, kernel id, signal extent, start event, end event)`` per launch, none for a refused launch,
and results that do not depend on whether the launches are timed.

The expected tuples are computed here from the direction of each call and from the library's own host queries (``mifwt_kernel_id``,
``mifwt_kernel_id_dtaps``, ``mifwt_bwt_kernel_id``, the 1-D envelope queries) on the descriptors of the very geometries — nothing is
copied from a run.
"""
import ctypes

import pytest
import torch

import ptwt_amd
from ptwt_amd import _bwt, _engine, _wavelets

pytestmark = pytest.mark.gpu

REFLECT, ZERO = _engine.MODE_IDS["reflect"], _engine.MODE_IDS["zero"]
B, H, W = 2, 24, 70
DB2 = _wavelets.host_taps("db2")
MH, MW = (H + 3) // 2, (W + 3) // 2  # M = floor((N + L - 1) / 2), L = 4


def _dev():
    return torch.device("cuda:0")


def _x(*shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(sum(shape)), dtype=torch.float32).to(_dev())


def _level_desc(mode_id, flen=4):
    """The descriptor of the dense 2-D level [B, H, W] -> [B, 4, MH, MW] (the one the engine fills for these tensors)."""
    planes = (4 * MH * MW, MW, 1)
    return _engine._desc(2, torch.float32, mode_id, flen, B, (H, W), (H * W, W, 1), (MH, MW), planes, planes)


def _recorded(fn):
    """(result with ``level_events`` unset, result with it set, the tuples without their events) of ``fn()``."""
    plain = fn()
    _engine.level_events = []
    try:
        timed = fn()
        events = list(_engine.level_events)
    finally:
        _engine.level_events = None
    torch.cuda.synchronize()
    for e in events:
        assert len(e) == 5 and e[3].elapsed_time(e[4]) >= 0.0  # both events were recorded on the launch stream
    return plain, timed, [e[:3] for e in events]


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b)
    return len(a) == len(b) and all(_same(p, q) for p, q in zip(a, b))


def test_level_2d():
    x = _x(B, H, W)
    plain, timed, events = _recorded(lambda: _engine.ENGINE.analysis(x, DB2[0], DB2[1], REFLECT))
    kid = _engine.load_library().mifwt_kernel_id(ctypes.byref(_level_desc(REFLECT)), 0)
    assert kid == _engine.kernel_id(2, torch.float32, "reflect", 4, B, (H, W), 0)
    assert events == [("fwd", kid, (H, W))]
    assert _same(plain, timed)


def test_level_2d_adjoint():
    g = _x(B, 4, MH, MW)
    plain, timed, events = _recorded(lambda: _engine.ENGINE.analysis_adjoint(g, (H, W), DB2[0], DB2[1], REFLECT))
    kid = _engine.load_library().mifwt_kernel_id(ctypes.byref(_level_desc(REFLECT)), 2)
    assert events == [("fwd_adj", kid, (H, W))]
    assert _same(plain, timed)


def test_level_2d_device_taps():
    x = _x(B, H, W)
    lo, hi = (_engine.DevTaps(torch.tensor(t, dtype=torch.float64, device=_dev())) for t in DB2[:2])
    plain, timed, events = _recorded(lambda: _engine.ENGINE.analysis(x, lo, hi, REFLECT))
    kid = _engine.load_library().mifwt_kernel_id_dtaps(ctypes.byref(_level_desc(REFLECT)), 0)
    assert events == [("fwd", kid, (H, W))]
    assert _same(plain, timed)
    assert _same(plain, _engine.ENGINE.analysis(x, DB2[0], DB2[1], REFLECT))  # (device-resident taps: the same numbers)


def test_tail_1d():
    rows, n, flen, levels = 3, 1001, 10, 3
    x = _x(rows, n)
    lib = _engine.load_library()
    # the route the engine takes, from the library's own envelope queries: the chunked long-row kernel where it fuses two levels or more
    # (it then takes as many as it says, the rest follows), else every remaining level in the one-workgroup-per-row launch
    k = lib.mifwt_dwt1_fwd_long_levels(0, flen, REFLECT, rows, n, levels)
    assert k < 2 and n <= lib.mifwt_dwt1_fwd_tail_max_n(0)  # 3 x 1001: the tail kernel takes all three levels
    plain, timed, events = _recorded(lambda: ptwt_amd.wavedec(x, "db5", level=levels, mode="reflect"))
    assert events == [("fwd", _engine.KID_TAIL, (n,))]
    assert _same(plain, timed)


def test_boundary_level_2d():
    x = _x(B, H, W)
    bank = _bwt.bank(DB2, "qr", "analysis")
    plain, timed, events = _recorded(lambda: _bwt.rows_level(x, bank, ZERO))
    planes = (4 * (H // 2) * (W // 2), W // 2, 1)
    d = _engine._desc(2, torch.float32, ZERO, 4, B, (H, W), (H * W, W, 1), (H // 2, W // 2), planes, planes)
    kid = _engine.load_library().mifwt_bwt_kernel_id(ctypes.byref(d), 0)
    assert kid == _bwt.KID_FWD
    assert events == [("bwt_fwd", kid, (H, W))]
    assert _same(plain, timed)


def test_refused_tail_leaves_no_event():
    """A 3-tap bank: ``mifwt_dwt1_fwd_tail`` refuses odd lengths, the engine method answers None and the levels run one by one — the
    refused launch leaves no tuple."""
    s = 0.5 ** 0.5
    bank = (torch.tensor([s, s, 0.0]), torch.tensor([-s, s, 0.0]), torch.tensor([0.0, s, s]), torch.tensor([0.0, s, -s]))
    x = _x(3, 200)
    lo, hi = [s, s, 0.0], [-s, s, 0.0]
    assert _engine.ENGINE.analysis_tail(x, lo, hi, ZERO, 3) is None
    plain, timed, events = _recorded(lambda: ptwt_amd.wavedec(x, bank, level=3, mode="zero"))
    lib, want, n = _engine.load_library(), [], 200
    for _ in range(3):
        m = (n + 2 * ((2 * 3 - 3) // 2) + n % 2 - 3) // 2 + 1  # (padded length - L) / 2 + 1 with the reference's pads: 200 -> 100 -> 50 -> 25
        d = _engine._desc(1, torch.float32, ZERO, 3, 3, (n,), (n, 1), (m,), (2 * m, 1), (2 * m, 1))
        want.append(("fwd", lib.mifwt_kernel_id(ctypes.byref(d), 0), (n,)))
        n = m
    assert events == want
    assert _same(plain, timed)
