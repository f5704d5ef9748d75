"""node_costs / best_basis of whole packet trees: the cost kernel (ids 61 / 62) against ``best_basis._composed_costs``, the float64 torch
composition a user would write per level buffer, at the same commit.

  2d-per / 2d-reflect   ``WaveletPacket2D`` db4 depth 3 on 64 x 1024 x 1024, float32 and float64 (85 nodes per image)
  1d                    ``WaveletPacket`` db5 depth 8 on 32 x 1 000 000 float32 (511 nodes per row)
  short                 4096 images of 33 x 33, db2 depth 2: 65 536 leaves of about 100 elements (the short-node regime)

Per cell: ``node_costs("shannon")`` alone, kernel against composition; the cost entry alone on prepared level buffers (``launch``: without
the tree's host work) for ``"shannon"``, for ``"norm", p=2`` and for ``"threshold"`` — the same bytes without the float64 ``log``, which
says whether the logarithm or the memory holds the launch back —; ``best_basis("shannon", joint=False)`` whole, kernel against
composition; and the time of expanding the tree, next to them.  ``hbm_share`` counts one read of every level buffer
against the 8 TB/s peak.

Protocol of tools/estimator_bench.py: device events; every leg warmed; a timed window of at least 0.2 s per leg; the legs alternate inside
each repeat; min / median / max over the repeats (five by default).  Before timing, the two legs are compared at the timed size to twice
the bound of tests/test_gpu_best_basis.py, ``(n + 64) 2^-53 sum |term|`` per node.  One JSON line per cell goes to stdout and to ``--out``
(default profiles/best_basis_bench.jsonl); ``not_ahead``: the kernel's median does not lead that leg's by more than the spread of the
windows.  No speed-up is promised: cells that trail are recorded as they are.

    python tools/best_basis_bench.py [--repeats 5] [--cells 2d-per,2d-reflect,2d-per64,2d-reflect64,1d,short] [--small] [--out FILE]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, ".")
import ptwt_amd  # noqa: E402
from ptwt_amd import best_basis as BB  # noqa: E402

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
    first = next(iter(legs))
    return stat, {k: stat[k]["median"] - stat[first]["median"] <= spread for k in legs if k != first}


class composed:
    """Inside: every cell takes the torch composition."""

    def __enter__(self):
        self.saved = BB.COMPOSED_CELLS
        BB.COMPOSED_CELLS = {(dt, nd, r) for dt in (torch.float32, torch.float64) for nd in (0, 1, 2) for r in ("short", "long")}

    def __exit__(self, *exc):
        BB.COMPOSED_CELLS = self.saved


def emulated(fn):
    def run():
        with composed():
            return fn()
    return run


def bench_tree(name, cls, shape, wavelet, mode, depth, dtype, repeats, emit):
    x = torch.randn(*shape, device="cuda", dtype=dtype, generator=torch.Generator(device="cuda").manual_seed(1))
    wp = cls(x, wavelet, mode=mode, maxlevel=depth)
    leaf = wp._keys_of_level(depth)[0]
    wp[leaf]
    bufs = [wp._level_buffer(s) for s in range(depth + 1)]
    byts = sum(b.numel() * b.element_size() for b in bufs)
    nodes = [b.shape[0] * len(wp._bands) ** s for s, b in enumerate(bufs)]
    regimes = sorted({BB._regime(dtype, b.numel() // n) for b, n in zip(bufs, nodes)})

    def emulate_costs():
        return [BB._composed_costs(b, n, "shannon") for b, n in zip(bufs, nodes)]

    # the legs agree: both lie within the bound of the exact value
    got = wp.node_costs("shannon")
    want = emulate_costs()
    worst = 0.0
    for s, (b, n, w) in enumerate(zip(bufs, nodes, want)):
        t2 = b.double().reshape(n, -1).square()
        mag = torch.where(t2 > 0, t2 * torch.log(torch.where(t2 > 0, t2, torch.ones_like(t2))), torch.zeros_like(t2)).abs().sum(-1)
        bound = 2 * (t2.shape[1] + 64) * 2.0 ** -53 * mag
        g = torch.stack([got[k].reshape(-1) for k in wp._keys_of_level(s)], -1).reshape(-1)
        assert bool(((g - w).abs() <= bound).all()), (name, s)
        worst = max(worst, float(((g - w).abs() / bound.clamp(min=1e-300)).max()))
        del t2, mag
    masks = wp.best_basis("shannon", joint=False)
    with composed():
        masks_e = wp.best_basis("shannon", joint=False)
    same = all(torch.equal(a, b) for a, b in zip(masks, masks_e))  # (a cost within rounding of a tie may fall either way)
    del got, want, masks, masks_e

    def expand():
        t = cls(x, wavelet, mode=mode, maxlevel=depth)
        return t[leaf]

    flat = [b.reshape(b.shape[0], -1, *b.shape[b.dim() - wp._ndim:]) for b in bufs]
    leads = [2] * len(flat)

    def launch(cost, p, param):
        return lambda: BB._costs_of(flat, leads, wp._ndim, cost, p, None, param)

    stat, not_ahead = measure({
        "kernel": lambda: wp.node_costs("shannon"),
        "emulation": emulate_costs,
        "launch": launch("shannon", None, 0.0),
        "launch_norm2": launch("norm", 2, 2.0),
        "launch_threshold": launch("threshold", None, 0.5),
        "best_basis_kernel": lambda: wp.best_basis("shannon", joint=False),
        "best_basis_emulation": emulated(lambda: wp.best_basis("shannon", joint=False)),
        "expand_tree": expand,
    }, repeats)
    emit(dict(cell=name, tree=f"{cls.__name__} {wavelet} depth {depth} {mode}", shape=list(shape), dtype=str(dtype).split(".")[-1],
              nodes=sum(nodes) // bufs[0].shape[0], regimes=regimes, repeats=repeats, us=stat, not_ahead=not_ahead, counted_bytes=byts,
              hbm_share={k: byts / (stat[k]["median"] * 1e-6) / HBM_PEAK for k in ("kernel", "emulation", "launch", "launch_norm2", "launch_threshold")},
              worst_diff_over_bound=worst, same_masks=same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cells", default="2d-per,2d-reflect,2d-per64,2d-reflect64,1d,short")
    ap.add_argument("--small", action="store_true", help="small shapes: a check that every leg runs and agrees, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "best_basis_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    big = not args.small
    WP, WP2 = ptwt_amd.WaveletPacket, ptwt_amd.WaveletPacket2D
    plane = (64, 1024, 1024) if big else (4, 128, 128)
    table = {
        "2d-per": (WP2, plane, "db4", "periodization", 3, torch.float32),
        "2d-reflect": (WP2, plane, "db4", "reflect", 3, torch.float32),
        "2d-per64": (WP2, plane, "db4", "periodization", 3, torch.float64),
        "2d-reflect64": (WP2, plane, "db4", "reflect", 3, torch.float64),
        "1d": (WP, (32, 1000000) if big else (4, 16384), "db5", "reflect", 8 if big else 4, torch.float32),
        "short": (WP2, (4096, 33, 33) if big else (64, 33, 33), "db2", "reflect", 2, torch.float32),
    }
    with open(args.out, "w") as f:
        def emit(res):
            line = json.dumps(res)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for name in args.cells.split(","):
            cls, shape, wavelet, mode, depth, dtype = table[name]
            bench_tree(name, cls, shape, wavelet, mode, depth, dtype, args.repeats, emit)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
