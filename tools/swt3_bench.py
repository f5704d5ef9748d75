"""swt3 / iswt3: the fused 3-D stationary levels (kernel ids 36 / 37, one launch per level) against the COMPOSED route of the same
library (``stationary_transform.FORCE_COMPOSED``: the 2-D level composed from the 1-D kernels on every depth slice, then the 1-D level
along depth on permuted copies — only kernels that the fused route does not touch).

Protocol of tools/swt2_bench.py: device events, every leg warmed, timed windows of at least 0.2 s, the legs alternate inside each
repeat, min / median / max over the repeats.  One JSON line per cell: microseconds per call and per level, the ratio of the medians,
and the share of the 8 TB/s HBM peak on the compulsory bytes of a level (9 volumes: 1 in + 8 out, resp. 8 in + 1 out).  ``verdict``
is "fused" only where the fused median beats the composed median by more than the spread of the windows — the cells that say
"composed" belong in ``stationary_transform.COMPOSED3_CELLS``.

    python tools/swt3_bench.py [--repeats 5] [--slices 0,16,64] [--cells 0,2] [--once CELL]

--slices: lattice slices per workgroup of the fused kernels to try (MIFWT_OPT_ROWS_PER_CHUNK; 0 = the library's own choice) on the
first cell of each direction; every other cell runs on the library's choice.  --once CELL: one fused call of that cell and nothing
else (the workload of a counter run: fetched bytes against the compulsory ones).
"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import ptwt_amd  # noqa: E402
from ptwt_amd import _engine  # noqa: E402
from ptwt_amd import stationary_transform as st  # noqa: E402
from ptwt_amd._wavelets import host_taps  # noqa: E402

HBM_PEAK = 8e12
# (transform, levels, wavelet, shape, dtype)
CELLS = [
    ("swt3", 3, "db2", (8, 256, 256, 256), torch.float32),
    ("swt3", 3, "db4", (8, 256, 256, 256), torch.float32),
    ("iswt3", 3, "db2", (8, 256, 256, 256), torch.float32),
    ("iswt3", 3, "db4", (8, 256, 256, 256), torch.float32),
    ("swt3", 3, "db4", (4, 256, 256, 256), torch.float64),
    ("iswt3", 3, "db4", (4, 256, 256, 256), torch.float64),
    ("swt3", 3, "haar", (8, 256, 256, 256), torch.float32),
    ("swt3", 3, "db3", (8, 256, 256, 256), torch.float32),
    ("swt3", 3, "db5", (8, 256, 256, 256), torch.float32),
    ("iswt3", 3, "haar", (8, 256, 256, 256), torch.float32),
    ("iswt3", 3, "db3", (8, 256, 256, 256), torch.float32),
    ("iswt3", 3, "db5", (8, 256, 256, 256), torch.float32),
]


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


def routed(fn, composed):
    def run():
        st.FORCE_COMPOSED = composed
        try:
            return fn()
        finally:
            st.FORCE_COMPOSED = False
    return run


def flat(c):
    return [c] if isinstance(c, torch.Tensor) else [t for e in c for t in (e.values() if isinstance(e, dict) else [e])]


def make_call(cell):
    transform, level, wavelet, shape, dtype = cell
    x = torch.randn(*shape, device="cuda", dtype=dtype)
    if transform == "swt3":
        return x, lambda: ptwt_amd.swt3(x, wavelet, level)
    coeffs = ptwt_amd.swt3(x, wavelet, level)
    coeffs = [coeffs[0].clone()] + [{k: t.clone() for k, t in c.items()} for c in coeffs[1:]]  # dense operands, not views of level buffers
    return x, lambda: ptwt_amd.iswt3(coeffs, wavelet)


def bench(cell, repeats, slices=0):
    transform, level, wavelet, shape, dtype = cell
    x, call = make_call(cell)
    legs = {"fused": routed(call, False), "composed": routed(call, True)}
    kid = st.KID_SWT3 if transform == "swt3" else st.KID_ISWT3
    _engine.set_option(_engine.OPT_ROWS_PER_CHUNK, slices)
    try:
        n0 = _engine.launch_count(kid)
        a = legs["fused"]()
        assert _engine.launch_count(kid) - n0 == level, "the fused leg did not run the fused kernel"
        b = legs["composed"]()
        assert _engine.launch_count(kid) - n0 == level, "the composed leg ran the fused kernel"
        diff = max(float((p - q).abs().max()) for p, q in zip(flat(a), flat(b)))
        del a, b
        for fn in legs.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in legs}
        for _ in range(repeats):
            for k, fn in legs.items():
                times[k].append(window(fn))
    finally:
        _engine.set_option(_engine.OPT_ROWS_PER_CHUNK, 0)
    stat = {k: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v)) for k, v in times.items()}
    spread = max((s["max"] - s["min"]) / s["median"] for s in stat.values())
    level_bytes = 9 * x.numel() * x.element_size()
    ratio = stat["composed"]["median"] / stat["fused"]["median"]
    flen = len(host_taps(wavelet)[0])
    plan = st.swt3_plan(dtype, flen, transform == "iswt3", shape[0], shape[1], shape[2], shape[3], 1)
    res = dict(transform=transform, shape=list(shape), wavelet=wavelet, filt_len=flen, level=level,
               dtype=str(dtype).split(".")[-1], slices_per_group=slices or "auto", repeats=repeats, us=stat,
               us_per_level={k: s["median"] / level for k, s in stat.items()},
               hbm_share={k: level_bytes / (s["median"] / level * 1e-6) / HBM_PEAK for k, s in stat.items()},
               composed_over_fused=ratio, spread=spread, verdict="fused" if ratio > 1 + spread else "composed",
               fused_vs_composed_max_abs_diff=diff, plan_level0=plan)
    print(json.dumps(res), flush=True)
    del x
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--slices", default="0")
    ap.add_argument("--cells", default="")
    ap.add_argument("--once", type=int, default=-1)
    args = ap.parse_args()
    if args.once >= 0:
        x, call = make_call(CELLS[args.once])
        torch.cuda.synchronize()
        call()
        torch.cuda.synchronize()
        print(json.dumps(dict(once=args.once, compulsory_bytes_per_level=9 * x.numel() * x.element_size(), levels=CELLS[args.once][1])))
        sys.exit(0)
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    slices = [int(r) for r in args.slices.split(",")]
    picked = [CELLS[int(i)] for i in args.cells.split(",")] if args.cells else CELLS
    seen = set()
    for cell in picked:
        first = cell[0] not in seen
        seen.add(cell[0])
        for r in (slices if first else [0]):
            bench(cell, args.repeats, r)
