"""Transforms of complex data (complex64 / complex128, index-map modes) on four legs per cell and direction:

  fused      the interleaved kernels: one fused launch per level (kernel ids 46 / 47; 3-D: the fused launch plus the pass along depth),
             whatever ``_cplx.COMPOSED_CELLS`` says (it is emptied for this leg)
  composed   the library's fallback, ``torch.complex(f(x.real), f(x.imag))`` per level (``_cplx.FORCE_COMPOSED``)
  emulation  the best a user wrote before complex data was accepted: ``view_as_real``, a ``movedim`` and a ``.contiguous()`` copy, ONE
             real call on the doubled batch, one ``torch.complex`` per sub-band
  real       the real call on a float tensor of the same number of bytes (the batch doubled), as context

Protocol of tools/ext_bench.py: device events; every leg warmed; a timed window of at least 0.2 s per leg; the legs alternate inside
each repeat; min / median / max over the repeats.  Before timing, the fused and the composed outputs are compared at the timed size
(norm-wise per tensor; complex64 1e-5, complex128 1e-12: random data, the reference-derived bounds are the tests').  One JSON line per
cell and direction goes to stdout and to ``--out`` (default profiles/cplx_bench.jsonl): microseconds per call, the ratios of the medians
and the share of the 8 TB/s HBM peak on the compulsory bytes (a level reads its input once and writes about as many samples once, 8 / 16
bytes each).  ``fused_behind_composed``: the fused median loses to the composed one by more than the spread of the windows — such a cell
belongs in ``_cplx.COMPOSED_CELLS``; a cell measured otherwise in ``_cplx.FUSED_AHEAD``.

    python tools/cplx_bench.py [--repeats 5] [--cells 2d,2d16,2d128,1d,3d] [--small] [--out FILE]
    python tools/cplx_bench.py --sweep [--out FILE]     every (direction, dtype, L, ndim) cell of the fused envelope, ONE level, the fused and
                                                        the composed leg only: the routing table
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, ".")
import ptwt_amd  # noqa: E402
from ptwt_amd import _cplx  # noqa: E402
from ptwt_amd._wavelets import filter_length  # noqa: E402

HBM_PEAK = 8e12
DEC = {1: ptwt_amd.wavedec, 2: ptwt_amd.wavedec2, 3: ptwt_amd.wavedec3}
REC = {1: ptwt_amd.waverec, 2: ptwt_amd.waverec2, 3: ptwt_amd.waverec3}
MODE = "symmetric"


def window(fn, min_seconds=0.2):
    """us per call over a window of at least ``min_seconds`` of device time."""
    n = 2
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= min_seconds * 1e3:
            return ms / n * 1e3
        n = max(n * 2, int(n * min_seconds * 1e3 / max(ms, 1e-3) * 1.2))


def tree_map(fn, c):
    if isinstance(c, torch.Tensor):
        return fn(c)
    if isinstance(c, dict):
        return {k: tree_map(fn, v) for k, v in c.items()}
    parts = [tree_map(fn, v) for v in c]
    return type(c)(*parts) if hasattr(c, "_fields") else type(c)(parts)


def flat(c):
    if isinstance(c, torch.Tensor):
        return [c]
    return [t for v in (c.values() if isinstance(c, dict) else c) for t in flat(v)]


def to_doubled_batch(t):
    """[B, ..] complex -> [2 B, ..] float: the components as two halves of the batch (a copy)."""
    r = torch.view_as_real(t).movedim(-1, 0).contiguous()
    return r.reshape(2 * t.shape[0], *t.shape[1:])


def from_doubled_batch(t):
    h = t.shape[0] // 2
    return torch.complex(t[:h], t[h:])


def with_route(fn, composed):
    """``fn`` with every cell of the envelope fused (``composed`` false) or every level composed."""
    def run():
        cells, _cplx.COMPOSED_CELLS, _cplx.FORCE_COMPOSED = _cplx.COMPOSED_CELLS, set(), composed
        try:
            return fn()
        finally:
            _cplx.COMPOSED_CELLS, _cplx.FORCE_COMPOSED = cells, False
    return run


def measure(legs, repeats):
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(window(fn))
    stat = {k: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v)) for k, v in times.items()}
    spread = {k: (v["max"] - v["min"]) / v["median"] for k, v in stat.items()}
    behind = stat["fused"]["median"] - stat["composed"]["median"] > max(stat["fused"]["max"] - stat["fused"]["min"],
                                                                         stat["composed"]["max"] - stat["composed"]["min"])
    return stat, spread, behind


def bench(name, shape, wavelet, level, dtype, repeats, sweep, emit):
    ndim = len(shape) - 1
    comp = torch.float32 if dtype == torch.complex64 else torch.float64
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.complex(torch.randn(*shape, device="cuda", dtype=comp, generator=g), torch.randn(*shape, device="cuda", dtype=comp, generator=g))
    xr = torch.randn(2 * shape[0], *shape[1:], device="cuda", dtype=comp, generator=g)
    coeffs = with_route(lambda: DEC[ndim](x, wavelet, mode=MODE, level=level), False)()
    coeffs_r = DEC[ndim](xr, wavelet, mode=MODE, level=level)
    tol = 1e-5 if dtype == torch.complex64 else 1e-12
    byts = 2 * x.element_size() * sum(x.numel() / (1 << (ndim * lv)) for lv in range(level))
    for direction, what in ((0, "wavedec"), (1, "waverec")):
        if direction == 0:
            call = lambda: DEC[ndim](x, wavelet, mode=MODE, level=level)  # noqa: E731
            legs = {"fused": with_route(call, False), "composed": with_route(call, True)}
            if not sweep:
                legs["emulation"] = lambda: tree_map(from_doubled_batch, DEC[ndim](to_doubled_batch(x), wavelet, mode=MODE, level=level))
                legs["real"] = lambda: DEC[ndim](xr, wavelet, mode=MODE, level=level)
        else:
            call = lambda: REC[ndim](coeffs, wavelet)  # noqa: E731
            legs = {"fused": with_route(call, False), "composed": with_route(call, True)}
            if not sweep:
                legs["emulation"] = lambda: from_doubled_batch(REC[ndim](tree_map(to_doubled_batch, coeffs), wavelet))
                legs["real"] = lambda: REC[ndim](coeffs_r, wavelet)
        ref = flat(legs["fused"]())
        err = {k: max(float((a - b).norm() / b.norm()) for a, b in zip(flat(legs[k]()), ref)) for k in legs if k in ("composed", "emulation")}
        assert all(e < tol for e in err.values()), (name, what, err)
        stat, spread, behind = measure(legs, repeats)
        emit(dict(cell=name, call="%s%s" % (what, "" if ndim == 1 else ndim), direction=direction, shape=list(shape), wavelet=wavelet,
                  filt_len=filter_length(wavelet), level=level, dtype=str(dtype).split(".")[-1], mode=MODE, repeats=repeats, us=stat, spread=spread,
                  over_fused={k: stat[k]["median"] / stat["fused"]["median"] for k in legs if k != "fused"}, fused_behind_composed=behind,
                  compulsory_bytes=byts, hbm_share={k: byts / (v["median"] * 1e-6) / HBM_PEAK for k, v in stat.items()}, max_rel_diff=err))


C64, C128 = torch.complex64, torch.complex128
CELLS = {
    "2d": [((32, 1024, 1024), "db4", 3, C64)],
    "2d16": [((32, 1024, 1024), "db8", 3, C64)],
    "2d128": [((16, 1024, 1024), "db4", 3, C128)],
    "1d": [((16, 1000000), "db5", 10, C64)],
    "3d": [((4, 256, 256, 256), "db2", 3, C64)],
}
SMALL = {
    "2d": [((4, 256, 256), "db4", 3, C64)],
    "2d16": [((4, 256, 256), "db8", 3, C64)],
    "2d128": [((4, 256, 256), "db4", 3, C128)],
    "1d": [((4, 16384), "db5", 4, C64)],
    "3d": [((2, 32, 32, 32), "db2", 2, C64)],
}
SWEEP_SHAPES = {1: (16, 1000000), 2: (16, 1024, 1024), 3: (2, 192, 192, 192)}
SWEEP_SMALL = {1: (4, 16384), 2: (4, 256, 256), 3: (2, 32, 32, 32)}
SWEEP_WAVELETS = ("haar", "db2", "db3", "db4", "db5", "db6", "db7", "db8", "db9", "db10")  # 2 .. 20 taps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cells", default="2d,2d16,2d128,1d,3d")
    ap.add_argument("--small", action="store_true", help="small shapes: a check that every leg runs and agrees, not a measurement")
    ap.add_argument("--sweep", action="store_true", help="one level of every cell of the fused envelope, fused against composed")
    ap.add_argument("--ndims", default="1,2,3", help="--sweep: the numbers of transformed axes")
    ap.add_argument("--out", default=os.path.join("profiles", "cplx_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        def emit(res):
            line = json.dumps(res)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        if args.sweep:
            for ndim in [int(v) for v in args.ndims.split(",")]:
                for dtype in (C64, C128):
                    for wavelet in SWEEP_WAVELETS:
                        bench("sweep%dd" % ndim, (SWEEP_SMALL if args.small else SWEEP_SHAPES)[ndim], wavelet, 1, dtype, args.repeats, True, emit)
            return
        for name in args.cells.split(","):
            for shape, wavelet, level, dtype in (SMALL if args.small else CELLS)[name]:
                bench(name, shape, wavelet, level, dtype, args.repeats, False, emit)


if __name__ == "__main__":
    main()
