"""threshold / threshold_firm on whole coefficient containers, the fused launch against the emulation with torch operations
(``thresholding._composed``, the same closed forms: real soft thresholding is the usual ``sign(x) * relu(|x| - v)``) at the same commit.

  fwd        ``threshold(coeffs, v, "soft")`` and ``threshold_firm(coeffs, v_lo, v_hi)`` on the containers of ``wavedec2`` db4 level 3 of
             64 x 1024 x 1024 (float32 and float64), ``wavedec`` db5 level 10 of 32 x 1 000 000 and ``wavedec3`` db2 level 3 of 8 x 256^3
  pipeline   ``waverec2(threshold(wavedec2(x)))``, whole
  fwdbwd     forward plus backward of the 2-D float32 container with a learnable one-element threshold and with a per-image one

Protocol of tools/ext_bench.py: device events; every leg warmed; a timed window of at least 0.2 s per leg; the legs alternate inside each
repeat; min / median / max over the repeats (five by default).  Before timing, both legs are compared at the timed size.  One JSON line
per cell goes to stdout and to ``--out`` (default profiles/thresh_bench.jsonl): microseconds per call, the ratio of the medians, the
share of the 8 TB/s HBM peak on the compulsory bytes (one read plus one write of the container; the backward two reads plus one write)
and ``fused_not_ahead``: the fused median does not lead the emulation's by more than the spread of the windows.

    python tools/thresh_bench.py [--repeats 5] [--cells fwd,pipeline,fwdbwd] [--small] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, ".")
import ptwt_amd  # noqa: E402
from ptwt_amd import thresholding as T  # noqa: E402

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


def emulate(coeffs, lo, hi=None):
    mode = T.FIRM if hi is not None else T.MODES["soft"]
    return tree_map(lambda t: T._composed(t, lo, hi, mode, 0.0), coeffs)


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
    return stat, stat["emulation"]["median"] - stat["fused"]["median"] <= spread


def emit_cell(emit, name, what, shape, dtype, legs, byts, repeats, tol):
    a, b = flat(legs["fused"]()), flat(legs["emulation"]())
    err = max(float((u.double() - v.double()).norm() / v.double().norm().clamp(min=1e-300)) for u, v in zip(a, b))
    assert err < tol, (name, what, err)
    del a, b
    stat, not_ahead = measure(legs, repeats)
    emit(dict(cell=name, call=what, shape=list(shape), dtype=str(dtype).split(".")[-1], repeats=repeats, us=stat,
              emulation_over_fused=stat["emulation"]["median"] / stat["fused"]["median"], fused_not_ahead=not_ahead, compulsory_bytes=byts,
              hbm_share={k: byts / (v["median"] * 1e-6) / HBM_PEAK for k, v in stat.items()}, max_rel_diff=err))


def bench_fwd(name, dec, shape, wavelet, level, dtype, repeats, emit):
    x = torch.randn(*shape, device="cuda", dtype=dtype, generator=torch.Generator(device="cuda").manual_seed(1))
    coeffs = dec(x, wavelet, level=level)
    del x
    byts = 2 * sum(t.numel() * t.element_size() for t in flat(coeffs))
    tol = 1e-5 if dtype == torch.float32 else 1e-12
    emit_cell(emit, name, "threshold soft", shape, dtype,
              {"fused": lambda: ptwt_amd.threshold(coeffs, 0.5, "soft"), "emulation": lambda: emulate(coeffs, 0.5)}, byts, repeats, tol)
    emit_cell(emit, name, "threshold_firm", shape, dtype,
              {"fused": lambda: ptwt_amd.threshold_firm(coeffs, 0.5, 1.5), "emulation": lambda: emulate(coeffs, 0.5, 1.5)}, byts, repeats, tol)


def bench_pipeline(shape, repeats, emit):
    x = torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    byts = 2 * x.numel() * x.element_size()  # (the thresholding step's share: about one read and one write of the data set)
    emit_cell(emit, "pipeline", "waverec2(threshold(wavedec2))", shape, x.dtype, {
        "fused": lambda: ptwt_amd.waverec2(ptwt_amd.threshold(ptwt_amd.wavedec2(x, "db4", level=3), 0.5, "soft"), "db4"),
        "emulation": lambda: ptwt_amd.waverec2(emulate(ptwt_amd.wavedec2(x, "db4", level=3), 0.5), "db4"),
        "transforms": lambda: ptwt_amd.waverec2(ptwt_amd.wavedec2(x, "db4", level=3), "db4"),
    }, byts, repeats, 1e-5)


def bench_fwdbwd(shape, repeats, emit):
    x = torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    coeffs = ptwt_amd.wavedec2(x, "db4", level=3)
    del x
    leaves = flat(coeffs)
    gouts = [torch.randn_like(t) for t in leaves]
    byts = 3 * sum(t.numel() * t.element_size() for t in leaves) + 2 * sum(t.numel() * t.element_size() for t in leaves)
    for what, v0 in (("one-element threshold", torch.full((1,), 0.5, device="cuda")), ("per-image threshold", torch.full((shape[0],), 0.5, device="cuda"))):
        def step(fn, v0=v0):
            v = v0.clone().requires_grad_(True)
            xs = [t.detach().requires_grad_(True) for t in leaves]
            out = flat(fn(tree_map(lambda t, it=iter(xs): next(it), coeffs), v))
            return list(torch.autograd.grad(out, xs + [v], gouts))

        emit_cell(emit, "fwdbwd", what, shape, torch.float32, {
            "fused": lambda: step(lambda c, v: ptwt_amd.threshold(c, v, "soft")),
            "emulation": lambda: step(lambda c, v: emulate(c, v)),
        }, byts, repeats, 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cells", default="fwd,pipeline,fwdbwd")
    ap.add_argument("--small", action="store_true", help="small shapes: a check that every leg runs and agrees, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "thresh_bench.jsonl"))
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
        if "fwd" in cells:
            bench_fwd("2d", ptwt_amd.wavedec2, (64, 1024, 1024) if big else (4, 128, 128), "db4", 3, torch.float32, args.repeats, emit)
            bench_fwd("2d64", ptwt_amd.wavedec2, (64, 1024, 1024) if big else (4, 128, 128), "db4", 3, torch.float64, args.repeats, emit)
            bench_fwd("1d", ptwt_amd.wavedec, (32, 1000000) if big else (4, 16384), "db5", 10 if big else 4, torch.float32, args.repeats, emit)
            bench_fwd("3d", ptwt_amd.wavedec3, (8, 256, 256, 256) if big else (2, 32, 32, 32), "db2", 3 if big else 2, torch.float32, args.repeats, emit)
        if "pipeline" in cells:
            bench_pipeline((64, 1024, 1024) if big else (4, 128, 128), args.repeats, emit)
        if "fwdbwd" in cells:
            bench_fwdbwd((64, 1024, 1024) if big else (4, 128, 128), args.repeats, emit)


if __name__ == "__main__":
    main()
