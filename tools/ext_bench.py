"""Analysis in the value-map extension modes ("smooth", "antisymmetric", "antireflect") on four legs per cell and mode:

  fused      the default route: one fused launch per level (kernel id 42; 3-D: the fused launch plus the axis pass along depth, id 44)
  axis       the axis passes of the same library (id 44, ``_ext.FORCE_AXIS``), alternating with the fused leg in one process
  emulation  what a user had to write before the modes existed: per level the extended tensor built with torch ops (slices, flips,
             an arange ramp, torch.cat per axis), ONE mode="zero" level of it, a crop to floor((n + L - 1) / 2) coefficients per axis
  symmetric  the padded route of the same call in mode="symmetric" (whatever launches it takes: multi-level where the library fuses
             levels), as context: what a boundary mode costs that an index map serves

Protocol of tools/per_bench.py: device events; every leg warmed; a timed window of at least 0.2 s per leg; the legs alternate inside
each repeat; min / median / max over the repeats.  One JSON line per cell and mode: microseconds per call, the ratios of the medians and
the share of the 8 TB/s HBM peak on the compulsory bytes (a level reads its input once and writes about as many samples once).
A fused cell whose median loses to the axis median by more than the spread of the windows belongs in ``_ext.AXIS_PASS_CELLS``.

    python tools/ext_bench.py [--repeats 5] [--cells 2d,2d64,1d,3d] [--modes smooth,antisymmetric,antireflect] [--small]
"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import ptwt_amd  # noqa: E402
from ptwt_amd import _ext  # noqa: E402
from ptwt_amd._wavelets import filter_length  # noqa: E402

HBM_PEAK = 8e12
DEC = {1: ptwt_amd.wavedec, 2: ptwt_amd.wavedec2, 3: ptwt_amd.wavedec3}


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


def extend(x, mode, pl, pr, d):
    """The extended tensor along ``d`` with torch ops (pads below the extent: one wrap)."""
    n = x.shape[d]
    assert 0 <= pl < n and 0 <= pr < n
    first, last = x.narrow(d, 0, 1), x.narrow(d, n - 1, 1)
    if mode == "antisymmetric":
        parts = [-x.narrow(d, 0, pl).flip(d), x, -x.narrow(d, n - pr, pr).flip(d)]
    elif mode == "antireflect":
        parts = [2 * first - x.narrow(d, 1, pl).flip(d), x, 2 * last - x.narrow(d, n - 1 - pr, pr).flip(d)]
    else:
        shape = [1] * x.dim()
        shape[d] = -1
        il = torch.arange(-pl, 0, device=x.device, dtype=x.dtype).view(shape)
        ir = torch.arange(1, pr + 1, device=x.device, dtype=x.dtype).view(shape)
        parts = [first + il * (x.narrow(d, 1, 1) - first), x, last + ir * (last - x.narrow(d, n - 2, 1))]
    return torch.cat(parts, d)


def emulated_dec(x, wavelet, mode, level, ndim):
    """The decomposition on the padded kernels: extend, one mode="zero" level, crop (coefficient k of the level is coefficient
    k + (L - 2) / 2 of the zero-padded level of the extended tensor)."""
    flen = filter_length(wavelet)
    out, cur = [], x
    for _ in range(level):
        ext = cur
        for d in range(-ndim, 0):
            n = cur.shape[d]
            ext = extend(ext, mode, flen - 2, flen - 2 + n % 2, d)
        c = DEC[ndim](ext, wavelet, mode="zero", level=1)
        crop = (Ellipsis, *[slice(flen // 2 - 1, flen // 2 - 1 + (n + flen - 1) // 2) for n in cur.shape[-ndim:]])
        out.insert(0, _like(c[1], [t[crop] for t in _details(c[1])]))
        cur = c[0][crop]
    return [cur] + out


def bench(name, shape, wavelet, level, dtype, mode, repeats):
    ndim = {"1d": 1, "2d": 2, "2d64": 2, "3d": 3}[name]
    x = torch.randn(*shape, device="cuda", dtype=dtype)

    def forced(fn):
        def run():
            _ext.FORCE_AXIS = True
            try:
                return fn()
            finally:
                _ext.FORCE_AXIS = False
        return run

    legs = {
        "fused": lambda: DEC[ndim](x, wavelet, mode=mode, level=level),
        "emulation": lambda: emulated_dec(x, wavelet, mode, level, ndim),
        "symmetric": lambda: DEC[ndim](x, wavelet, mode="symmetric", level=level),
    }
    legs["axis"] = forced(legs["fused"])
    flat = lambda c: [c[0]] + [t for e in c[1:] for t in _details(e)]  # noqa: E731
    ref = flat(legs["fused"]())
    # (norm-wise per tensor: the extrapolating modes grow the coefficients of random data from level to level)
    err = {k: max(float((a - b).norm() / b.norm()) for a, b in zip(ref, flat(legs[k]()))) for k in ("emulation", "axis")}
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
    # level l reads N / 2^(n l) samples and writes about as many
    byts = 2 * x.element_size() * sum(x.numel() / (1 << (ndim * lv)) for lv in range(level))
    res = dict(cell=name, mode=mode, shape=list(shape), wavelet=wavelet, level=level, dtype=str(dtype).split(".")[-1], repeats=repeats,
               us=stat, spread=spread, over_fused={k: stat[k]["median"] / stat["fused"]["median"] for k in ("axis", "emulation", "symmetric")},
               fused_behind_axis=stat["fused"]["median"] - stat["axis"]["median"] > max(stat["fused"]["max"] - stat["fused"]["min"],
                                                                                         stat["axis"]["max"] - stat["axis"]["min"]),
               compulsory_bytes=byts, hbm_share={k: byts / (v["median"] * 1e-6) / HBM_PEAK for k, v in stat.items()}, max_rel_diff=err)
    print(json.dumps(res), flush=True)


CELLS = {
    "2d": [((64, 1024, 1024), "db4", 3, torch.float32), ((64, 1024, 1024), "db8", 3, torch.float32)],
    "2d64": [((64, 1024, 1024), "db4", 3, torch.float64), ((64, 1024, 1024), "db8", 3, torch.float64)],
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
    ap.add_argument("--modes", default="smooth,antisymmetric,antireflect")
    ap.add_argument("--small", action="store_true", help="small shapes: a check that every leg runs and agrees, not a measurement")
    args = ap.parse_args()
    for name in args.cells.split(","):
        for shape, wavelet, level, dtype in (SMALL if args.small else CELLS)[name]:
            for mode in args.modes.split(","):
                bench(name, shape, wavelet, level, dtype, mode, args.repeats)


if __name__ == "__main__":
    main()
