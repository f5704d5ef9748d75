"""swt2 / iswt2: the fused 2-D stationary levels (kernel ids 34 / 35, one launch per level) against the COMPOSED route of the same
library (``stationary_transform.FORCE_COMPOSED``: the 1-D level kernels along the last axis, then along the other one on permuted
copies — only kernels that the fused route does not touch).

Protocol of tools/boundary_bench.py: device events, every leg warmed, timed windows of at least 0.2 s, the legs alternate inside each
repeat, min / median / max over the repeats.  One JSON line per cell: microseconds per call and per level, the ratio of the medians,
and the share of the 8 TB/s HBM peak on the compulsory bytes of a level (5 planes: 1 in + 4 out, resp. 4 in + 1 out).  ``verdict``
is "fused" only where the fused median beats the composed median by more than the spread of the windows — the cells that say
"composed" belong in ``stationary_transform.COMPOSED2_CELLS``.

    python tools/swt2_bench.py [--repeats 5] [--rows 0,32,64,128]

--rows: lattice rows per wave of the fused kernels to try (MIFWT_OPT_ROWS_PER_CHUNK; 0 = the library's own choice) on the first cell
of each direction; every other cell runs on the library's choice.
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
    ("swt2", 3, "db4", (64, 1024, 1024), torch.float32),
    ("swt2", 3, "db8", (64, 1024, 1024), torch.float32),
    ("swt2", 3, "db4", (8, 4096, 4096), torch.float32),
    ("swt2", 3, "db8", (8, 4096, 4096), torch.float32),
    ("iswt2", 3, "db4", (64, 1024, 1024), torch.float32),
    ("iswt2", 3, "db8", (64, 1024, 1024), torch.float32),
    ("swt2", 3, "db4", (64, 1024, 1024), torch.float64),
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


def bench(cell, repeats, rows=0):
    transform, level, wavelet, shape, dtype = cell
    x = torch.randn(*shape, device="cuda", dtype=dtype)
    if transform == "swt2":
        call = lambda: ptwt_amd.swt2(x, wavelet, level)  # noqa: E731
    else:
        coeffs = ptwt_amd.swt2(x, wavelet, level)
        coeffs = [coeffs[0].clone()] + [tuple(t.clone() for t in c) for c in coeffs[1:]]  # dense operands, not views of level buffers
        call = lambda: ptwt_amd.iswt2(coeffs, wavelet)  # noqa: E731
    legs = {"fused": routed(call, False), "composed": routed(call, True)}
    kid = st.KID_SWT2 if transform == "swt2" else st.KID_ISWT2
    _engine.set_option(_engine.OPT_ROWS_PER_CHUNK, rows)
    try:
        n0 = _engine.launch_count(kid)
        a = legs["fused"]()
        assert _engine.launch_count(kid) - n0 == level, "the fused leg did not run the fused kernel"
        b = legs["composed"]()
        assert _engine.launch_count(kid) - n0 == level, "the composed leg ran the fused kernel"
        flat = lambda c: [c] if isinstance(c, torch.Tensor) else [t for e in c for t in (e if isinstance(e, tuple) else [e])]  # noqa: E731
        diff = max(float((p - q).abs().max()) for p, q in zip(flat(a), flat(b)))
        del a, b
        for fn in legs.values():
            for _ in range(3):
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
    level_bytes = 5 * x.numel() * x.element_size()
    ratio = stat["composed"]["median"] / stat["fused"]["median"]
    res = dict(transform=transform, shape=list(shape), wavelet=wavelet, filt_len=len(host_taps(wavelet)[0]), level=level,
               dtype=str(dtype).split(".")[-1], rows_per_wave=rows or "auto", repeats=repeats, us=stat,
               us_per_level={k: s["median"] / level for k, s in stat.items()},
               hbm_share={k: level_bytes / (s["median"] / level * 1e-6) / HBM_PEAK for k, s in stat.items()},
               composed_over_fused=ratio, spread=spread, verdict="fused" if ratio > 1 + spread else "composed",
               fused_vs_composed_max_abs_diff=diff)
    print(json.dumps(res), flush=True)
    del x
    torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", default="0")
    ap.add_argument("--cells", default="")
    args = ap.parse_args()
    print(json.dumps(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__)), flush=True)
    rows = [int(r) for r in args.rows.split(",")]
    picked = [CELLS[int(i)] for i in args.cells.split(",")] if args.cells else CELLS
    seen = set()
    for cell in picked:
        first = cell[0] not in seen
        seen.add(cell[0])
        for r in (rows if first else [0]):
            bench(cell, args.repeats, r)
