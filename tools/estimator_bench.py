"""estimate_sigma / shrink on whole coefficient containers against the emulation a user writes with torch operations (``abs`` /
``flatten`` / ``sort`` for the median, ``pow(2).mean`` for the moments, ``thresholding._composed`` to apply) at the same commit.

  sigma      ``estimate_sigma(coeffs)`` on the containers of ``wavedec2`` db4 level 3 of 64 x 1024 x 1024 (float32 and float64),
             ``wavedec`` db5 level 10 of 32 x 1 000 000 and ``wavedec3`` db2 level 3 of 8 x 256^3: the streaming selection (the default
             at these sizes) against the sort
  routes     the two selections against each other and the sort where both run: 4096 images of 33 x 33 and 64 images of 12 288
  shrink     ``shrink(coeffs, "bayes", "soft")`` on the same containers against the emulation
  pipeline   ``waverec2(shrink(wavedec2(x)))`` next to the fixed-threshold pipeline ``waverec2(threshold(wavedec2(x), 0.5))``

Protocol of tools/thresh_bench.py: device events; every leg warmed; a timed window of at least 0.2 s per leg; the legs alternate inside
each repeat; min / median / max over the repeats (five by default).  Before timing, the legs are compared at the timed size.  One JSON
line per cell goes to stdout and to ``--out`` (default profiles/estimator_bench.jsonl): microseconds per call, the share of the 8 TB/s
HBM peak on the counted bytes (one read of the finest band per selection pass, plus one read and one write of the container for
``shrink``) and, per other leg, ``not_ahead``: the first leg's median does not lead that leg's by more than the spread of the windows.

    python tools/estimator_bench.py [--repeats 5] [--cells sigma,routes,shrink,pipeline] [--small] [--out FILE]
"""
import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, ".")
import ptwt_amd  # noqa: E402
from ptwt_amd import estimators as E, thresholding as T  # noqa: E402

HBM_PEAK = 8e12


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


def flat(c):
    if isinstance(c, torch.Tensor):
        return [c]
    return [t for v in (c.values() if isinstance(c, dict) else c) for t in flat(v)]


def tree_map(fn, c):
    if isinstance(c, torch.Tensor):
        return fn(c)
    if isinstance(c, dict):
        return {k: tree_map(fn, v) for k, v in c.items()}
    parts = [tree_map(fn, v) for v in c]
    return type(c)(*parts) if hasattr(c, "_fields") else type(c)(parts)


def emulate_sigma(coeffs):
    d, lead = E._finest(coeffs, None)
    return E._composed_sigma(d, lead)[1].reshape(d.shape[:lead])


def emulate_shrink(coeffs):
    d, lead = E._finest(coeffs, None)
    sigma = emulate_sigma(coeffs).double()
    eps = float(torch.finfo(d.dtype).eps)

    def one(t):
        m2 = t.double().pow(2).flatten(lead).mean(-1)
        v = (sigma * sigma / torch.sqrt(torch.clamp(m2 - sigma * sigma, min=eps))).to(t.dtype)
        return T._composed(t, v, None, T.MODES["soft"], 0.0)

    return type(coeffs)([coeffs[0]] + [tree_map(one, e) for e in coeffs[1:]])


def forced(fn):
    def run():
        E.FORCE_STREAM = True
        try:
            return fn()
        finally:
            E.FORCE_STREAM = False

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
    spread = max(v["max"] - v["min"] for v in stat.values())
    first = next(iter(legs))
    return stat, {k: stat[k]["median"] - stat[first]["median"] <= spread for k in legs if k != first}


def emit_cell(emit, name, what, shape, dtype, legs, byts, repeats, tol):
    outs = {k: flat(fn()) for k, fn in legs.items() if k != "fixed"}
    first = next(iter(outs))
    err = max(float((u.double() - v.double()).norm() / v.double().norm().clamp(min=1e-300))
              for k, o in outs.items() if k != first for u, v in zip(outs[first], o))
    assert err < tol, (name, what, err)
    del outs
    stat, not_ahead = measure(legs, repeats)
    emit(dict(cell=name, call=what, shape=list(shape), dtype=str(dtype).split(".")[-1], repeats=repeats, us=stat, not_ahead=not_ahead,
              counted_bytes=byts, hbm_share={k: byts / (v["median"] * 1e-6) / HBM_PEAK for k, v in stat.items()}, max_rel_diff=err))


def passes(dtype, count):
    return 1 if count <= E.lds_capacity(dtype) else len(E.stream_plan(dtype))


def container(dec, shape, wavelet, level, dtype):
    x = torch.randn(*shape, device="cuda", dtype=dtype, generator=torch.Generator(device="cuda").manual_seed(1))
    return dec(x, wavelet, level=level)


def bench_container(name, dec, shape, wavelet, level, dtype, repeats, emit, cells):
    coeffs = container(dec, shape, wavelet, level, dtype)
    d, lead = E._finest(coeffs, None)
    count = d.numel() // math.prod(d.shape[:lead])
    band = passes(dtype, count) * d.numel() * d.element_size()
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    if "sigma" in cells:
        emit_cell(emit, name, f"estimate_sigma ({count} per image)", shape, dtype,
                  {"kernel": lambda: ptwt_amd.estimate_sigma(coeffs), "emulation": lambda: emulate_sigma(coeffs)}, band, repeats, tol)
    if "shrink" in cells:
        byts = band + 2 * sum(t.numel() * t.element_size() for t in flat(coeffs))
        emit_cell(emit, name, "shrink bayes soft", shape, dtype,
                  {"kernel": lambda: ptwt_amd.shrink(coeffs), "emulation": lambda: emulate_shrink(coeffs)}, byts, repeats, tol)


def bench_routes(shape, dtype, repeats, emit):
    x = torch.randn(*shape, device="cuda", dtype=dtype, generator=torch.Generator(device="cuda").manual_seed(1))
    count = x.numel() // shape[0]
    emit_cell(emit, "routes", f"estimate_sigma ({count} per image)", shape, dtype, {
        "lds": lambda: ptwt_amd.estimate_sigma(x, lead=1),
        "stream": forced(lambda: ptwt_amd.estimate_sigma(x, lead=1)),
        "emulation": lambda: E._composed_sigma(x, 1)[1],
    }, x.numel() * x.element_size(), repeats, 1e-6)


def bench_pipeline(shape, repeats, emit):
    x = torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    byts = 2 * x.numel() * x.element_size()
    emit_cell(emit, "pipeline", "waverec2(shrink(wavedec2))", shape, x.dtype, {
        "kernel": lambda: ptwt_amd.waverec2(ptwt_amd.shrink(ptwt_amd.wavedec2(x, "db4", level=3)), "db4"),
        "emulation": lambda: ptwt_amd.waverec2(emulate_shrink(ptwt_amd.wavedec2(x, "db4", level=3)), "db4"),
        "fixed": lambda: ptwt_amd.waverec2(ptwt_amd.threshold(ptwt_amd.wavedec2(x, "db4", level=3), 0.5, "soft"), "db4"),
    }, byts, repeats, 1e-5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cells", default="sigma,routes,shrink,pipeline")
    ap.add_argument("--small", action="store_true", help="small shapes: a check that every leg runs and agrees, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "estimator_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    big = not args.small
    with open(args.out, "w") as f:
        def emit(res):
            line = json.dumps(res)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        cells = args.cells.split(",")
        if "sigma" in cells or "shrink" in cells:
            r = args.repeats
            bench_container("2d", ptwt_amd.wavedec2, (64, 1024, 1024) if big else (4, 128, 128), "db4", 3, torch.float32, r, emit, cells)
            bench_container("2d64", ptwt_amd.wavedec2, (64, 1024, 1024) if big else (4, 128, 128), "db4", 3, torch.float64, r, emit, cells)
            bench_container("1d", ptwt_amd.wavedec, (32, 1000000) if big else (4, 16384), "db5", 10 if big else 4, torch.float32, r, emit, cells)
            bench_container("3d", ptwt_amd.wavedec3, (8, 256, 256, 256) if big else (2, 32, 32, 32), "db2", 3 if big else 2, torch.float32, r, emit, cells)
        if "routes" in cells:
            bench_routes((4096, 33, 33) if big else (64, 33, 33), torch.float32, args.repeats, emit)
            bench_routes((64, 12288) if big else (4, 12288), torch.float32, args.repeats, emit)
            bench_routes((64, 6144) if big else (4, 6144), torch.float64, args.repeats, emit)
        if "pipeline" in cells:
            bench_pipeline((64, 1024, 1024) if big else (4, 128, 128), args.repeats, emit)


if __name__ == "__main__":
    main()
