"""Periodized transforms (mode="periodization") on three legs per cell:

  fused      the default route: one fused launch per level (kernel ids 38 / 39; 3-D: the fused launch plus the axis pass along depth)
  axis       the axis passes of the same library (ids 40 / 41, ``_per.FORCE_AXIS``), alternating with the fused leg in one process
  emulation  what a user had to write before the mode existed, on the padded kernels: per level torch.roll by -(L/2 - 1), one
             mode="periodic" level, a slice to N/2 coefficients per axis (an odd extent first repeats its last sample); synthesis:
             every band periodically extended to the padded coefficient count with torch.cat, one padded synthesis level, a roll back

Protocol of tools/boundary_bench.py: device events; every leg warmed; a timed window of at least 0.2 s per leg; the legs alternate
inside each repeat; min / median / max over the repeats.  One JSON line per cell: microseconds per call, the ratios of the medians,
and the share of the 8 TB/s HBM peak on the compulsory bytes (a level reads its input once and writes as many samples once).
A fused cell whose median loses to the axis median by more than the spread of the windows belongs in ``_per.AXIS_PASS_CELLS``.

    python tools/per_bench.py [--repeats 5] [--cells 2d,2d64,1d,3d] [--small]
"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import ptwt_amd  # noqa: E402
from ptwt_amd import _per  # noqa: E402
from ptwt_amd._wavelets import filter_length  # noqa: E402

HBM_PEAK = 8e12
DEC = {1: ptwt_amd.wavedec, 2: ptwt_amd.wavedec2, 3: ptwt_amd.wavedec3}
REC = {1: ptwt_amd.waverec, 2: ptwt_amd.waverec2, 3: ptwt_amd.waverec3}


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


def _details(c):
    return list(c.values()) if isinstance(c, dict) else (list(c) if isinstance(c, (tuple, list)) else [c])


def _like(c, tensors):
    if isinstance(c, dict):
        return dict(zip(c.keys(), tensors))
    return type(c)(*tensors) if hasattr(c, "_fields") else (tuple(tensors) if isinstance(c, tuple) else tensors[0])


def emulated_dec(x, wavelet, level, ndim):
    """The periodized decomposition of even extents on the padded "periodic" kernels."""
    flen = filter_length(wavelet)
    dims = tuple(range(-ndim, 0))
    out, cur = [], x
    for _ in range(level):
        for d in dims:  # (an odd extent repeats its last sample)
            if cur.shape[d] % 2:
                cur = torch.cat([cur, cur.narrow(d, cur.shape[d] - 1, 1)], d)
        half = [n // 2 for n in cur.shape[-ndim:]]
        c = DEC[ndim](torch.roll(cur, [-(flen // 2 - 1)] * ndim, dims), wavelet, mode="periodic", level=1)
        crop = (Ellipsis, *[slice(0, h) for h in half])
        out.insert(0, _like(c[1], [t[crop] for t in _details(c[1])]))
        cur = c[0][crop]
    return [cur] + out


def emulated_rec(coeffs, wavelet, ndim):
    """Its inverse: every band extended periodically to the padded count, one padded synthesis level, the roll undone."""
    flen = filter_length(wavelet)
    dims = tuple(range(-ndim, 0))
    cur = coeffs[0]
    for pos, c in enumerate(coeffs[1:]):
        def ext(t):
            for d in dims:
                m, reps = t.shape[d], -(-(flen // 2 - 1) // t.shape[d]) + 1
                t = torch.cat([t] * reps, d).narrow(d, 0, m + flen // 2 - 1)
            return t

        y = REC[ndim]([ext(cur), _like(c, [ext(t) for t in _details(c)])], wavelet)
        # the padded synthesis returns 2 (M + L/2 - 1) - L + 2 = 2 M samples per axis: its sample n is sample n + L/2 - 1 of the
        # periodized output
        cur = torch.roll(y, [flen // 2 - 1] * ndim, dims)
        if pos + 2 < len(coeffs):  # (an odd level comes out one sample long)
            cur = cur[(Ellipsis, *[slice(0, n) for n in _details(coeffs[pos + 2])[0].shape[-ndim:]])]
    return cur


def bench(name, shape, wavelet, level, dtype, repeats):
    ndim = {"1d": 1, "2d": 2, "2d64": 2, "3d": 3}[name]
    x = torch.randn(*shape, device="cuda", dtype=dtype)

    def forced(fn):
        def run():
            _per.FORCE_AXIS = True
            try:
                return fn()
            finally:
                _per.FORCE_AXIS = False
        return run

    coeffs = DEC[ndim](x, wavelet, mode="periodization", level=level)
    legs = {
        "dec fused": lambda: DEC[ndim](x, wavelet, mode="periodization", level=level),
        "dec emulation": lambda: emulated_dec(x, wavelet, level, ndim),
        "rec fused": lambda: REC[ndim](coeffs, wavelet, mode="periodization"),
        "rec emulation": lambda: emulated_rec(coeffs, wavelet, ndim),
    }
    legs["dec axis"], legs["rec axis"] = forced(legs["dec fused"]), forced(legs["rec fused"])
    # the emulation computes what the fused leg computes
    flat = lambda c: [c[0]] + [t for e in c[1:] for t in _details(e)]  # noqa: E731
    err_dec = max(float((a - b).abs().max()) for a, b in zip(flat(legs["dec fused"]()), flat(legs["dec emulation"]())))
    err_rec = float((legs["rec fused"]() - legs["rec emulation"]()).abs().max())
    err_rt = float((legs["rec fused"]()[tuple(slice(0, n) for n in x.shape)] - x).abs().max())
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
    # level l reads N / 2^(n l) samples and writes as many
    byts = 2 * x.element_size() * sum(x.numel() / (1 << (ndim * lv)) for lv in range(level))
    res = dict(cell=name, shape=list(shape), wavelet=wavelet, level=level, dtype=str(dtype).split(".")[-1], repeats=repeats, us=stat,
               spread=spread,
               emulation_over_fused={d: stat[d + " emulation"]["median"] / stat[d + " fused"]["median"] for d in ("dec", "rec")},
               axis_over_fused={d: stat[d + " axis"]["median"] / stat[d + " fused"]["median"] for d in ("dec", "rec")},
               compulsory_bytes=byts, hbm_share={k: byts / (v["median"] * 1e-6) / HBM_PEAK for k, v in stat.items()},
               max_abs_diff=dict(dec_vs_emulation=err_dec, rec_vs_emulation=err_rec, round_trip=err_rt))
    print(json.dumps(res), flush=True)


CELLS = {
    "2d": [((64, 1024, 1024), "db4", 3, torch.float32), ((64, 1024, 1024), "db8", 3, torch.float32)],
    "2d64": [((64, 1024, 1024), "db4", 3, torch.float64)],
    "1d": [((32, 1000000), "db5", 10, torch.float32)],
    "3d": [((8, 256, 256, 256), "db2", 3, torch.float32)],
}
SMALL = {
    "2d": [((4, 256, 256), "db4", 3, torch.float32), ((4, 256, 256), "db8", 3, torch.float32)],
    "2d64": [((4, 256, 256), "db4", 3, torch.float64)],
    "1d": [((4, 16384), "db5", 4, torch.float32)],
    "3d": [((2, 32, 32, 32), "db2", 2, torch.float32)],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cells", default="2d,2d64,1d,3d")
    ap.add_argument("--small", action="store_true", help="small shapes: a check that every leg runs and agrees, not a measurement")
    args = ap.parse_args()
    for name in args.cells.split(","):
        for shape, wavelet, level, dtype in (SMALL if args.small else CELLS)[name]:
            bench(name, shape, wavelet, level, dtype, args.repeats)


if __name__ == "__main__":
    main()
