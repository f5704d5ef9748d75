"""Shared helpers of the data-gradient tests (tests/test_gpu_data_gradients.py, tests/test_gpu_independent_banks.py and their CPU
companions): one differentiable call with FIXED taps — a wavelet name, or a bank ``(dec_lo, dec_hi, rec_lo, rec_hi)`` given as four
tuples of Python floats (hashable: it serves as part of a case's key) — through the float64 differentiable CPU reference
(oracle/torch_autograd_ref.py), seeded Gaussian inputs and cotangents, the three error measures of a compared tensor, and the harness
(:class:`Harness`) that runs a case through the library and compares it tensor by tensor.

A case is ``(fn, shape, wavelet, mode, level, dtype)`` plus optional ``axes``; :func:`inputs` and :func:`chain` yield everything one
side of the comparison needs, computed by ``R`` in ``compute`` precision from inputs quantised to the case's dtype first:

* ``coeffs``   the flattened coefficients of ``R.<fn>(x)``;
* ``gx``       d/dx of ``sum_i <w_i, c_i>`` with Gaussian ``w_i``;
* ``rec``      ``R.<rec>(leaves)``, the leaves being the float64 coefficients quantised to the dtype;
* ``gleaves``  the gradients of ``<v, rec(leaves)>`` w.r.t. every leaf, Gaussian ``v``.

The cotangents are Gaussian on purpose: a smooth cotangent (the suite's ``cos(0.37 k + i)`` weights) is almost annihilated by the
high-pass adjoint, so the relative error of a float32 chain is cancellation noise (3.5e-6 .. 2.5e-5 norm-wise for the float32 reference
itself) and a bound derived from it would be 20 - 100 times too loose to see a wrong border sample.
"""
from __future__ import annotations

import contextlib
from collections import namedtuple
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

import ptwt_amd
from ptwt_amd import _engine
from oracle import fwt_oracle as O
from oracle import torch_autograd_ref as R
from tests import _golden as G

# analysis entry point -> (synthesis entry point, transformed axes)
FNS = {"wavedec": ("waverec", 1), "wavedec2": ("waverec2", 2), "fswavedec2": ("fswaverec2", 2), "wavedec3": ("waverec3", 3),
       "fswavedec3": ("fswaverec3", 3)}
MEASURES = ("norm", "maxabs", "border")
LEGS = ("fwd", "inv", "fwd_adj", "inv_adj")
# a wavelet name, or the four filters as tuples of floats
Bank = Union[str, Tuple[Tuple[float, ...], ...]]

Case = namedtuple("Case", "fn shape wavelet mode level dtype axes seed", defaults=(None, 0))


def gaussian(shape: Sequence[int], seed: int, dtype: torch.dtype) -> torch.Tensor:
    """A seeded standard-normal tensor, drawn in float64 and quantised to ``dtype`` (CPU)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64).to(dtype)


def flat(coeffs) -> List[torch.Tensor]:
    return [t for _, t in G.flatten_coeffs(coeffs)]


def rebuild(template, leaves: Sequence[torch.Tensor]):
    """The container of ``template`` (a list / tuple of tensors, 3-tuples or dicts) filled with ``leaves`` in :func:`flat` order."""
    it = iter(leaves)
    out = []
    for c in template:
        if isinstance(c, dict):
            out.append({k: next(it) for k in c})
        elif isinstance(c, (tuple, list)):
            out.append(tuple(next(it) for _ in c))
        else:
            out.append(next(it))
    return type(template)(out) if isinstance(template, (tuple, list)) else out


def filt_len(wavelet: Bank) -> int:
    return len(O.filter_bank(wavelet)[0])


def describe(wavelet: Bank) -> str:
    """A name as it is; a bank of floats by its length and first tap (what a failure message shows instead of 4 L numbers)."""
    return wavelet if isinstance(wavelet, str) else f"bank[{len(wavelet[0])} taps, dec_lo[0]={wavelet[0][0]:.6f}]"


def norm_axes(fn: str, ndim_tensor: int, axes) -> Tuple[int, ...]:
    n = FNS[fn][1]
    if axes is None:
        axes = tuple(range(-n, 0))
    if isinstance(axes, int):
        axes = (axes,)
    return tuple(a % ndim_tensor for a in axes)


def border_width(flen: int, n: int) -> int:
    """Samples of an axis of extent ``n`` within reach of a boundary extension of one level: ``L - 1 + n % 2`` per edge (the border
    kernels' own width)."""
    return flen - 1 + n % 2


def border_mask(shape: Sequence[int], axes: Sequence[int], flen: int) -> np.ndarray:
    """True for the samples within ``L - 1 + N % 2`` of any edge of any transformed axis."""
    mask = np.zeros(tuple(shape), dtype=bool)
    for a in axes:
        n = shape[a]
        b = min(border_width(flen, n), n)
        idx = [slice(None)] * len(shape)
        idx[a] = slice(0, b)
        mask[tuple(idx)] = True
        idx[a] = slice(n - b, n)
        mask[tuple(idx)] = True
    return mask


def measures(got, want, mask: Optional[np.ndarray] = None) -> Dict[str, float]:
    """Norm-wise error, max-abs error over the largest reference value and (with a mask) the norm-wise error of the masked samples."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    out = {"norm": float(G.relerr(got, want)), "maxabs": float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-300))}
    if mask is not None:
        out["border"] = float(G.relerr(got[mask], want[mask]))
    return out


def rowwise_measures(got, want_distinct, distinct: int, mask: Optional[np.ndarray] = None) -> Dict[str, float]:
    """:func:`measures` of ``got`` [rows, ...] against a reference known for ``distinct`` rows only, row ``r`` of ``got`` being a copy of
    source row ``r % distinct``: the same numbers as against the full, tiled reference, without ever building it.  ``mask``: the border
    strip of ONE row (shape ``got.shape[1:]``)."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want_distinct, dtype=np.float64)
    assert got.shape[1:] == want.shape[1:] and want.shape[0] == distinct, (got.shape, want.shape)
    num = den = bnum = bden = worst = 0.0
    for r0 in range(0, got.shape[0], distinct):
        blk = got[r0 : r0 + distinct]
        w = want[: blk.shape[0]]
        diff = blk - w
        num += float(np.sum(diff * diff))
        den += float(np.sum(w * w))
        worst = max(worst, float(np.abs(diff).max()))
        if mask is not None:
            bnum += float(np.sum(diff[:, mask] ** 2))
            bden += float(np.sum(w[:, mask] ** 2))
    out = {"norm": float(np.sqrt(num) / np.sqrt(den)) if den > 0 else float(np.sqrt(num)),
           "maxabs": worst / max(float(np.abs(want).max()), 1e-300)}
    if mask is not None:
        out["border"] = float(np.sqrt(bnum) / np.sqrt(bden)) if bden > 0 else float(np.sqrt(bnum))
    return out


def tile_rows(t: torch.Tensor, rows: int) -> torch.Tensor:
    """``rows`` rows, row ``r`` a copy of row ``r % len(t)`` of ``t``."""
    reps = -(-rows // t.shape[0])
    return t.repeat(reps, *([1] * (t.dim() - 1)))[:rows].contiguous()


def _bank(wavelet: Bank, compute: torch.dtype):
    """float64: the name or the bank of floats itself (``R`` turns either into float64 taps); float32: the same taps rounded to
    float32."""
    return wavelet if compute == torch.float64 else R.bank_of(wavelet, dtype=torch.float32)


def inputs(fn: str, shape, wavelet: Bank, mode: str, level: int, dtype: torch.dtype, axes=None, seed: int = 0):
    """The inputs of a case, quantised to its dtype: ``x``, the cotangents ``w`` of the coefficients, the ``leaves`` of the
    reconstruction (the float64 reference coefficients, quantised), the cotangent ``v`` of the reconstruction; and the container
    ``template`` of the coefficients."""
    rec = FNS[fn][0]
    kw = {"mode": mode, "level": level}
    akw = {} if axes is None else ({"axis": axes} if fn == "wavedec" else {"axes": axes})
    x = gaussian(shape, 1000 + seed, dtype)
    with torch.no_grad():
        template = getattr(R, fn)(x.double(), wavelet, **kw, **akw)
        leaves = [t.to(dtype) for t in flat(template)]
        y = getattr(R, rec)(rebuild(template, [t.double() for t in leaves]), wavelet, **akw)
    w = [gaussian(t.shape, 2000 + 17 * seed + i, dtype) for i, t in enumerate(leaves)]
    v = gaussian(y.shape, 3000 + seed, dtype)
    return {"x": x, "w": w, "leaves": leaves, "v": v, "template": template, "kw": kw, "akw": akw}


def chain(fn: str, wavelet: Bank, inp, compute: torch.dtype = torch.float64):
    """The four results of a case through ``R`` in ``compute`` precision (float32: float32 inputs and float32 taps)."""
    rec = FNS[fn][0]
    bank = _bank(wavelet, compute)
    x = inp["x"].to(compute).requires_grad_(True)
    coeffs = flat(getattr(R, fn)(x, bank, **inp["kw"], **inp["akw"]))
    (gx,) = torch.autograd.grad(sum((w.to(compute) * c).sum() for w, c in zip(inp["w"], coeffs)), x)
    leaves = [t.to(compute).requires_grad_(True) for t in inp["leaves"]]
    y = getattr(R, rec)(rebuild(inp["template"], leaves), bank, **inp["akw"])
    gl = torch.autograd.grad((inp["v"].to(compute) * y).sum(), leaves)
    return {"coeffs": [c.detach() for c in coeffs], "gx": gx.detach(), "rec": y.detach(), "gleaves": [g.detach() for g in gl]}


def compare(got, want, fn: str, wavelet: Bank, axes=None) -> Dict[str, float]:
    """Worst value of every measure over the tensors of two :func:`chain`-shaped results (the border strip for d/dx only)."""
    worst = {m: 0.0 for m in MEASURES}

    def take(m):
        for k, v in m.items():
            worst[k] = max(worst[k], v)

    for a, b in zip(got["coeffs"] + [got["rec"]] + got["gleaves"], want["coeffs"] + [want["rec"]] + want["gleaves"]):
        take(measures(a.double().numpy(), b.double().numpy()))
    shape = tuple(want["gx"].shape)
    take(measures(got["gx"].double().numpy(), want["gx"].double().numpy(), border_mask(shape, norm_axes(fn, len(shape), axes), filt_len(wavelet))))
    return worst


def reference_deviation(fn, shape, wavelet: Bank, mode, level, axes=None, seed: int = 0) -> Dict[str, float]:
    """What the float32 run of the reference itself (float32 inputs, float32 taps) deviates from its float64 run on the same quantised
    inputs, per measure: the yardstick of the float32 bounds."""
    inp = inputs(fn, shape, wavelet, mode, level, torch.float32, axes, seed)
    return compare(chain(fn, wavelet, inp, torch.float32), chain(fn, wavelet, inp, torch.float64), fn, wavelet, axes)


# ---- the harness: one case through the library, tensor by tensor against the reference ---------------------------------------------------
@contextlib.contextmanager
def options(opts):
    """Routing options of the library for the duration of a block: ``((key, value), ...)``, every key back to 0 afterwards."""
    try:
        for k, v in opts:
            _engine.set_option(k, v)
        yield
    finally:
        for k, _ in opts:
            _engine.set_option(k, 0)


def border_kernel(ndim, flen, mode, ext, debug):
    """Which border kernel an analysis adjoint of this geometry runs after its synthesis launch (adjoint_border_supported / border2_fits of
    csrc/mifwt_adjoint_border.hip), or None."""
    if mode == "zero" or (debug & 1024) or flen % 2 or flen > 32 or any(n < 2 * (flen + 1) for n in ext):
        return None
    if ndim == 2:
        return "line" if flen >= 8 and not (debug & 4096) else "sample"
    return "1d" if ndim == 1 else "3d"


def ids(ev, leg):
    return [(e, k) for e, k, _ in ev[leg]]


class Harness:
    """The state of one test module that runs cases through the library: its bounds (dtype -> measure -> bound), the (leg, kernel id)
    pairs and border kernels its cases reached, the worst error per dtype and measure, the float64 references of the last few cases
    (shared by the route variants of a case) and the float32 cases that ran with Gaussian cotangents (what the float32 yardstick of the
    module must list).  ``device``: where the library runs ("cpu": under a stand-in engine, no kernel events).  ``count_raises``: a
    case whose reference raises is run through the library, which must raise the same error type, and is counted in ``raised`` (the
    module's closing test decides how many it accepts); without it such a case fails where it stands."""

    def __init__(self, bounds, device="cuda:0", count_raises=False):
        self.count_raises = count_raises
        self.bounds = bounds
        self.device = torch.device(device)
        self.reached = set()  # (leg, kernel id) and ("border", "line" | "sample" | "1d" | "3d")
        self.worst = {dt: {} for dt in bounds}
        self.refs = {}  # case -> (inputs, float64 results)
        self.f32_cases = []
        self.ran = []  # every case that was compared, in order (variants of a case again)
        self.raised = []  # cases whose reference raised (and the library with it): nothing was compared
        self.last = None  # the library's tensors of the last run: coefficients, d/dx, reconstruction, leaf gradients

    def reference(self, case):
        if case not in self.refs:
            inp = inputs(case.fn, case.shape, case.wavelet, case.mode, case.level, case.dtype, case.axes, case.seed)
            self.refs[case] = (inp, chain(case.fn, case.wavelet, inp))
            if len(self.refs) > 6:
                self.refs.pop(next(iter(self.refs)))
        return self.refs[case]

    @contextlib.contextmanager
    def recording(self, into, leg):
        _engine.level_events = []
        try:
            yield
            if self.device.type == "cuda":
                torch.cuda.synchronize()
            into[leg] = [(e[0], e[1], e[2]) for e in _engine.level_events]
        finally:
            _engine.level_events = None

    def check(self, got, want, dtype, what, mask=None, rows=None):
        """Shape, dtype and the three measures of one tensor against the bounds; the figures go into ``worst`` before anything is
        asserted."""
        assert got.dtype == dtype, (what, got.dtype)
        got = got.detach().double().cpu().numpy()
        want = want.double().numpy()
        if rows is None:
            assert got.shape == want.shape, (what, got.shape, want.shape)
            m = measures(got, want, mask)
        else:
            assert got.shape == (rows,) + want.shape[1:], (what, got.shape, want.shape)
            m = rowwise_measures(got, want, want.shape[0], mask)
        for k, v in m.items():
            self.worst[dtype][k] = max(self.worst[dtype].get(k, 0.0), v)
        for k, v in m.items():
            assert v < self.bounds[dtype][k], (what, k, v, self.bounds[dtype][k])
        return m

    def run(self, case, opts=(), create_graph=False, expect=None, generic=(), layout=None, loss="gauss", rows=None, grads=True, bank=None):
        """One case on the device against its reference.  ``expect``: leg -> kernel ids that must all appear on it; ``generic``: legs that
        may reach the generic passes; ``layout``: "transposed" hands x over as a transposed view; ``loss``: "gauss", "sum" (sum of
        c.sum(): the backward gets expanded stride-0 cotangents) or an index (that band alone: the other cotangents arrive as zeros);
        ``rows``: the batch of the device run, built from the case's (fewer) distinct rows; ``grads`` false: values only — the
        coefficients and the reconstruction of calls that build no graph (their own routes), nothing recorded on the backward legs;
        ``bank``: what the library is handed as the wavelet in place of ``case.wavelet`` (another form of the same taps)."""
        self.last = None
        try:
            inp, want = self.reference(case)
        except (RuntimeError, ValueError) as err:  # (a pad the reference refuses: the library must refuse it too)
            if not self.count_raises:
                raise
            x = gaussian(case.shape, 1000 + case.seed, case.dtype).to(self.device)
            akw = {} if case.axes is None else ({"axis": case.axes} if case.fn == "wavedec" else {"axes": case.axes})
            try:
                getattr(ptwt_amd, case.fn)(x, case.wavelet if bank is None else bank, mode=case.mode, level=case.level, **akw)
            except type(err):
                self.raised.append(case)
                return None, None
            raise AssertionError(("the reference raises, the library does not", case[:2], describe(case.wavelet), case[3:], err))
        if loss != "gauss":  # (another cotangent of the analysis: its own reference chain, the inputs stay)
            inp = dict(inp)
            inp["w"] = [torch.ones_like(w) if loss == "sum" else (w if i == loss else torch.zeros_like(w)) for i, w in enumerate(inp["w"])]
            want = chain(case.fn, case.wavelet, inp)
        elif case.dtype == torch.float32:
            if case not in self.f32_cases:
                self.f32_cases.append(case)
        fn, rec = getattr(ptwt_amd, case.fn), getattr(ptwt_amd, FNS[case.fn][0])
        dev = self.device
        up = (lambda t: t.to(dev)) if rows is None else (lambda t: tile_rows(t, rows).to(dev))
        what = (case.fn, case.shape, describe(case.wavelet)) + tuple(case[3:]) + (tuple(opts), create_graph, layout, loss, rows, grads)
        wavelet = case.wavelet if bank is None else bank
        debug = dict(opts).get(_engine.OPT_DEBUG, 0)
        ev = {leg: [] for leg in LEGS}
        gx, gl = None, ()
        with options(opts):
            x = up(inp["x"])
            if layout == "transposed":
                x = x.transpose(-1, -2).contiguous().transpose(-1, -2)
                assert not x.is_contiguous()
            x.requires_grad_(grads)
            with self.recording(ev, "fwd"):
                coeffs = fn(x, wavelet, **inp["kw"], **inp["akw"])
            fl = flat(coeffs)
            assert len(fl) == len(want["coeffs"]), what
            if grads:
                if loss == "sum":
                    total = sum(c.sum() for c in fl)
                elif loss == "gauss":
                    total = sum((up(w) * c).sum() for w, c in zip(inp["w"], fl))
                else:
                    total = (up(inp["w"][loss]) * fl[loss]).sum()
                with self.recording(ev, "fwd_adj"):
                    (gx,) = torch.autograd.grad(total, x, create_graph=create_graph)
            leaves = [up(t).requires_grad_(grads) for t in inp["leaves"]]
            with self.recording(ev, "inv"):
                y = rec(rebuild(inp["template"], leaves), wavelet, **inp["akw"])
            if grads:
                with self.recording(ev, "inv_adj"):
                    gl = torch.autograd.grad((up(inp["v"]) * y).sum(), leaves, create_graph=create_graph)
        self.last = {"coeffs": [c.detach() for c in fl], "gx": None if gx is None else gx.detach(), "rec": y.detach(),
                     "gleaves": [g.detach() for g in gl]}
        self.ran.append(case)
        for i, (a, b) in enumerate(zip(fl, want["coeffs"])):
            self.check(a, b, case.dtype, what + ("coefficient", i), rows=rows)
        if grads:
            axes = norm_axes(case.fn, len(case.shape), case.axes)
            mask = border_mask(case.shape[1:] if rows else case.shape, [a - 1 for a in axes] if rows else axes, filt_len(case.wavelet))
            self.check(gx, want["gx"], case.dtype, what + ("d/dx",), mask=mask, rows=rows)
        self.check(y, want["rec"], case.dtype, what + ("reconstruction",), rows=rows)
        for i, (a, b) in enumerate(zip(gl, want["gleaves"])):
            self.check(a, b, case.dtype, what + ("d/dleaf", i), rows=rows)
        # routes: after the numbers, so that a moved route does not hide a wrong gradient
        kids = {leg: {k for _, k, _ in ev[leg]} for leg in LEGS}
        for leg in LEGS:
            self.reached.update((leg, k) for k in kids[leg])
            assert 0 not in kids[leg] or leg in generic, (what, leg, "generic passes", ev[leg])
            assert set((expect or {}).get(leg, ())) <= kids[leg], (what, leg, "expected", expect[leg], "ran", ev[leg])
        nd, flen = FNS[case.fn][1], filt_len(case.wavelet)
        for eng_leg, _, ext in ev["fwd_adj"]:
            b = border_kernel(nd, flen, case.mode, ext, debug) if eng_leg == "fwd_adj" else None
            if b:
                self.reached.add(("border", b))
        return ev, kids
