"""mra: all components in one launch (kernels 63 / 64) against ``mra._composed``, the definition a user would write with this package's
own calls — ``level + 1`` zero-filled containers through ``iswt`` / ``waverec`` — at the same commit.

  swt / swt64          ``swt`` db5 level 6 on 32 x 1 000 000, float32 / float64
  dwt-per / dwt-reflect  ``wavedec`` db5 level 6 on 32 x 1 000 000 float32, periodization / reflect;  dwt-per64: float64
  short-swt / short-dwt  db4 level 5 on 4096 x 1024 float32 (rows of at most a tile), ``swt`` / ``wavedec`` periodization;  *64: float64

Per cell three legs: ``fused``, the default route with an empty routing table (analysis + the projection launch); ``composed``; and
``projection``, the launch alone on prepared coefficients.  ``analysis`` is timed next to them.  ``hbm_share`` of the projection counts
``2 (n + 1) N`` elements per row for ``swt`` (every band read once, every component written once) and one read of the container plus
``(n + 1) N`` written for ``dwt``, against the 8 TB/s peak.

Protocol of tools/best_basis_bench.py: device events; every leg warmed; a timed window of at least 0.2 s per leg; the legs alternate inside
each repeat; min / median / max over the repeats (five by default).  Before timing, the two routes are compared at the timed size within
the bound of tests/test_gpu_mra.py (1e-6 / 1e-12 of each component's norm).  One JSON line per cell goes to stdout and to ``--out``
(default profiles/mra_bench.jsonl); ``not_ahead``: the fused median does not lead the composition's by more than the widest spread of
the windows — such a cell belongs in ``mra.COMPOSED_CELLS``.  No speed-up is promised: cells that trail are recorded as they are.

    python tools/mra_bench.py [--repeats 5] [--cells swt,swt64,...] [--small] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, ".")
import ptwt_amd  # noqa: E402

M = importlib.import_module("ptwt_amd.mra")
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
    return stat, spread


def bench(name, shape, wavelet, level, transform, mode, dtype, repeats, emit):
    x = torch.randn(*shape, device="cuda", dtype=dtype, generator=torch.Generator(device="cuda").manual_seed(1))
    rows, n = shape
    kw = dict(transform=transform, mode=mode)
    saved = M.COMPOSED_CELLS
    M.COMPOSED_CELLS = set()
    try:
        # the legs agree within the tests' bound
        tol = 1e-6 if dtype == torch.float32 else 1e-12
        got, want = ptwt_amd.mra(x, wavelet, level, **kw), M._composed(x, wavelet, level, -1, transform, mode)
        worst = max(float((g.double() - w.double()).norm() / w.double().norm()) for g, w in zip(got, want))
        assert worst < tol, (name, worst)
        del got, want

        coeffs = M._analysis(x, wavelet, level, -1, transform, mode)
        nb = len(coeffs)
        depths = [nb - 1] + [nb - i for i in range(1, nb)]
        level_len = None if transform == "swt" else [n] + [int(c.shape[-1]) for c in coeffs[:0:-1]]
        _, _, rec_lo, rec_hi = ptwt_amd._wavelets.host_taps(wavelet)
        out = torch.empty((nb, rows, n), dtype=dtype, device="cuda")
        size = x.element_size()
        read = sum(c.numel() for c in coeffs)
        counted = (read + nb * rows * n) * size

        stat, spread = measure({
            "fused": lambda: ptwt_amd.mra(x, wavelet, level, **kw),
            "composed": lambda: M._composed(x, wavelet, level, -1, transform, mode),
            "projection": lambda: M._project(coeffs, depths, level_len, n, rec_lo, rec_hi, circular=mode == "periodization", out=out),
            "analysis": lambda: M._analysis(x, wavelet, level, -1, transform, mode),
        }, repeats)
    finally:
        M.COMPOSED_CELLS = saved
    emit(dict(cell=name, call=f"mra {transform} {wavelet} level {level}" + ("" if transform == "swt" else " " + mode), shape=list(shape),
              dtype=str(dtype).split(".")[-1], routing_cell=[transform, str(dtype).split(".")[-1], M._regime(n)], repeats=repeats, us=stat,
              widest_spread_us=spread, speedup=stat["composed"]["median"] / stat["fused"]["median"],
              not_ahead=stat["composed"]["median"] - stat["fused"]["median"] <= spread, counted_bytes=counted,
              hbm_share_projection=counted / (stat["projection"]["median"] * 1e-6) / HBM_PEAK, worst_diff=worst))


def main():
    ap = argparse.ArgumentParser()
    cells = "swt,swt64,dwt-per,dwt-reflect,dwt-per64,short-swt,short-dwt,short-swt64,short-dwt64"
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cells", default=cells)
    ap.add_argument("--small", action="store_true", help="small shapes: a check that every leg runs and agrees, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "mra_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    big = not args.small
    long, short = ((32, 1000000), (4096, 1024)) if big else ((4, 20000), (64, 1024))
    deep = 6 if big else 4
    f32, f64, per = torch.float32, torch.float64, "periodization"
    table = {
        "swt": (long, "db5", deep, "swt", per, f32),
        "swt64": (long, "db5", deep, "swt", per, f64),
        "dwt-per": (long, "db5", deep, "dwt", per, f32),
        "dwt-reflect": (long, "db5", deep, "dwt", "reflect", f32),
        "dwt-per64": (long, "db5", deep, "dwt", per, f64),
        "short-swt": (short, "db4", 5, "swt", per, f32),
        "short-dwt": (short, "db4", 5, "dwt", per, f32),
        "short-swt64": (short, "db4", 5, "swt", per, f64),
        "short-dwt64": (short, "db4", 5, "dwt", per, f64),
    }
    with open(args.out, "w") as f:
        def emit(res):
            line = json.dumps(res)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for name in args.cells.split(","):
            bench(name, *table[name], args.repeats, emit)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
