"""Guard bytes around what kernels 59 / 60 write: ``arr`` of coeffs_to_array / ravel_coeffs and the ONE backing allocation of the
copy=True calls, carved out of guarded blocks (the ``guarded`` fixture and helpers of tests/test_gpu_canaries.py), with the odd-extent
and narrow-band containers whose rows start and end anywhere inside a 16-byte vector."""
import importlib

import pytest
import torch

import ptwt_amd
from ptwt_amd import _engine
from ptwt_amd.constants import WaveletDetailTuple2d
from tests import _pack_ref as R
from tests.test_gpu_canaries import _x, guarded  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

C = importlib.import_module("ptwt_amd.coeff_array")
PAD = -7.5
ROUTED = set(C.COMPOSED_CELLS)


@pytest.fixture(autouse=True)
def kernels_everywhere(monkeypatch):
    """The tests are about kernels 59 / 60: the cells that the routing rule sends to the composition run on the kernels here."""
    monkeypatch.setattr(C, "COMPOSED_CELLS", set())


def _flat(c):
    return [c] if isinstance(c, torch.Tensor) else [c[0]] + [t for lv in R.levels(c)[1] for t in lv.values()]


def _tensors(out):
    """The tensors of a result: ``arr`` of ``(arr, slices[, shapes])``, else every tensor of the container."""
    if isinstance(out, tuple) and len(out) in (2, 3) and isinstance(out[1], list):
        return [out[0]]
    return _flat(out)


def _guarded_call(guarded, monkeypatch, what, fn, inputs, kid, blocks):
    """fn() with the module's allocations guarded: the guards, the inputs, the kernel that ran, and equality with the unguarded call."""
    keep = [t.clone() for t in inputs]
    ref = fn()
    guarded.check(what)  # (what the transforms that made the inputs allocated: checked and forgotten)
    monkeypatch.setattr(C, "torch", guarded)
    _engine.level_events = []
    try:
        got = fn()
        n = guarded.check(what)
        ids = [e[1] for e in _engine.level_events]
    finally:
        _engine.level_events = None
        monkeypatch.setattr(C, "torch", torch)
    assert n == blocks and ids == [kid], (what, n, ids)
    for a, b in zip(inputs, keep):
        assert torch.equal(a, b), f"{what}: an input was modified"
    for a, b in zip(_tensors(got), _tensors(ref)):
        assert R.same_bits(a, b), what
    return got


def _containers():
    out = {
        "wavedec 3 x 37 db4": (ptwt_amd.wavedec(_x(3, 37), "db4", mode="symmetric", level=3), "wavedec"),
        "wavedec 2 x 1001 db4": (ptwt_amd.wavedec(_x(2, 1001), "db4", mode="symmetric", level=3), "wavedec"),
        "wavedec2 3 x 23 x 37 db4": (ptwt_amd.wavedec2(_x(3, 23, 37), "db4", mode="symmetric", level=3), "wavedec2"),
        "wavedec2 2 x 64 x 65 db2 f64": (ptwt_amd.wavedec2(_x(2, 64, 65, dtype=torch.float64), "db2", mode="symmetric", level=3), "wavedec2"),
        "wavedec3 2 x 9 x 10 x 11 db2": (ptwt_amd.wavedec3(_x(2, 9, 10, 11), "db2", mode="symmetric", level=2), "wavedecn"),
    }
    for w in (1, 2, 3):  # bands narrower than one 16-byte vector, 16-bit elements included
        for dtype in (torch.float32, torch.bfloat16):
            bands = lambda h, ww: WaveletDetailTuple2d(*[_x(2, 4, h, ww, seed=k + w).to(dtype)[:, k + 1] for k in range(3)])
            out[f"narrow {w} {dtype}"] = ((_x(2, 2, w).to(dtype), bands(2, w), bands(3, w + 1), bands(5, 2 * w + 1)), "wavedec2")
    return out


def test_canaries_of_the_four_calls(guarded, monkeypatch):
    for what, (c, fmt) in _containers().items():
        inputs = _flat(c)
        arr, slices = _guarded_call(guarded, monkeypatch, f"coeffs_to_array {what}", lambda: ptwt_amd.coeffs_to_array(c, PAD), inputs, 59, 1)
        flat, rsl, shapes = _guarded_call(guarded, monkeypatch, f"ravel_coeffs {what}", lambda: ptwt_amd.ravel_coeffs(c), inputs, 59, 1)
        assert R.same_bits(arr, R.to_array(R.cpu(c), PAD)[0]) and R.same_bits(flat, R.ravel(R.cpu(c))[0])
        arr, flat = arr.clone(), flat.clone()  # (out of the guarded blocks, whose guards have been checked)
        back = _guarded_call(guarded, monkeypatch, f"array_to_coeffs copy {what}", lambda: ptwt_amd.array_to_coeffs(arr, slices, fmt, copy=True),
                             [arr], 60, 1)
        rback = _guarded_call(guarded, monkeypatch, f"unravel_coeffs copy {what}", lambda: ptwt_amd.unravel_coeffs(flat, rsl, shapes, fmt, copy=True),
                              [flat], 60, 1)
        assert R.same_container(back, R.cpu(c)) and R.same_container(rback, R.cpu(c), ordered=False)
