"""bfloat16 against float16 storage on the same calls, and against what a bf16 user writes without it: cast to float32, transform,
cast back.

Protocol of tools/boundary_bench.py / tools/swt2_bench.py: device events, every leg warmed, timed windows of at least 0.2 s, the legs
alternate inside each repeat, min / median / max over the repeats (default 5).  One JSON line per cell and direction: microseconds
per call for each leg, the spread of the windows, bf16 over f16 and f32-with-casts over bf16.

Cells: ``wavedec2`` / ``waverec2`` db4 level 3 on 64 x 1024 x 1024 (LDS-tile kernels, ids 7 / 8); ``fswavedec2`` / ``fswaverec2`` sym16
level 5 on 32 x 8192 x 8192 (a slice of BASELINE config 5) on the matrix-core kernels (ids 11 / 23) and forced to the vector tile kernels
(option 7 = 2); ``wavedec`` / ``waverec`` db5 level 10 on 32 x 1 000 000 (streaming axis kernels, ids 3 / 4).

    python tools/bf16_bench.py [--repeats 5] [--cells 0,1,2,3] [--dtypes f16,bf16,f32cast]

``--dtypes f16`` runs on a library without bf16 as well (MIFWT_LIB=libmifwt_<tag>.so: the float16 figures of another build of the
library on the same box, for the "float16 must not get slower" comparison).  ``routing`` says, per matrix-core cell, whether the bf16
matrix-core median is behind the bf16 tile-kernel median by more than the spread (the project's routing rule: such a cell would go to
the tile kernel).
"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import ptwt_amd  # noqa: E402
from ptwt_amd import _engine  # noqa: E402

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
# (name, analysis, synthesis, wavelet, level, shape, option 7)
CELLS = [
    ("tile", "wavedec2", "waverec2", "db4", 3, (64, 1024, 1024), 0),
    ("mfma", "fswavedec2", "fswaverec2", "sym16", 5, (32, 8192, 8192), 0),
    ("mfma->tile", "fswavedec2", "fswaverec2", "sym16", 5, (32, 8192, 8192), 2),
    ("stream1d", "wavedec", "waverec", "db5", 10, (32, 1000000), 0),
]


def window(fn, min_seconds=0.2):
    """us per call over a window of at least ``min_seconds`` of device time."""
    n = 1
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


def map_tree(c, f):
    if isinstance(c, torch.Tensor):
        return f(c)
    if isinstance(c, dict):
        return {k: f(v) for k, v in c.items()}
    return type(c)(map_tree(e, f) for e in c) if not hasattr(c, "_fields") else type(c)(*(map_tree(e, f) for e in c))


def bench(cell, repeats, dtypes):
    name, fwd, inv, wavelet, level, shape, opt7 = cell
    f, r = getattr(ptwt_amd, fwd), getattr(ptwt_amd, inv)
    g = torch.Generator(device="cuda").manual_seed(1)
    x32 = torch.randn(*shape, device="cuda", generator=g)
    legs = {0: {}, 1: {}}
    keep = []
    for d in dtypes:
        if d == "f32cast":
            xb = x32.to(torch.bfloat16)
            cb = map_tree(f(xb.float(), wavelet, level=level), lambda t: t.to(torch.bfloat16))
            legs[0][d] = lambda xb=xb: map_tree(f(xb.float(), wavelet, level=level), lambda t: t.to(torch.bfloat16))
            legs[1][d] = lambda cb=cb: r(map_tree(cb, lambda t: t.float()), wavelet).to(torch.bfloat16)
        else:
            xd = x32.to(DT[d])
            cd = map_tree(f(xd, wavelet, level=level), lambda t: t.clone())  # dense operands, not views of level buffers
            legs[0][d] = lambda xd=xd: f(xd, wavelet, level=level)
            legs[1][d] = lambda cd=cd: r(cd, wavelet)
        keep.append(d)
    del x32
    for direction in (0, 1):
        for fn in legs[direction].values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs[direction]}
        for _ in range(repeats):
            for k, fn in legs[direction].items():
                times[k].append(window(fn))
        stat = {k: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v)) for k, v in times.items()}
        spread = max((s["max"] - s["min"]) / s["median"] for s in stat.values())
        res = dict(cell=name, call=(fwd, inv)[direction], wavelet=wavelet, level=level, shape=list(shape), option7=opt7, repeats=repeats,
                   us=stat, spread=spread)
        if "f16" in stat and "bf16" in stat:
            res["bf16_over_f16"] = stat["bf16"]["median"] / stat["f16"]["median"]
        if "f32cast" in stat and "bf16" in stat:
            res["f32cast_over_bf16"] = stat["f32cast"]["median"] / stat["bf16"]["median"]
        print(json.dumps(res), flush=True)
        yield res
    legs.clear()
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cells", default="")
    ap.add_argument("--dtypes", default="f16,bf16,f32cast")
    args = ap.parse_args()
    dtypes = [d for d in args.dtypes.split(",") if d]
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, library=_engine.LIB_PATH.split("/")[-1])), flush=True)
    picked = [CELLS[int(i)] for i in args.cells.split(",")] if args.cells else CELLS
    results = {}
    ptwt_amd.set_half_storage(True)
    try:
        for cell in picked:
            _engine.set_option(7, cell[6])
            try:
                results[cell[0]] = list(bench(cell, args.repeats, dtypes))
            finally:
                _engine.set_option(7, 0)
    finally:
        ptwt_amd.set_half_storage(False)
    if "bf16" in dtypes and "mfma" in results and "mfma->tile" in results:
        for a, b in zip(results["mfma"], results["mfma->tile"]):
            m, t = a["us"]["bf16"]["median"], b["us"]["bf16"]["median"]
            spread = max(a["spread"], b["spread"])
            print(json.dumps(dict(routing=a["call"], bf16_mfma_us=m, bf16_tile_us=t, spread=spread,
                                  verdict="tile" if m > t * (1 + spread) else "matrix cores")), flush=True)
