"""Boundary-wavelet transforms (MatrixWavedec2 / MatrixWavedec) against two yardsticks that are not the code under test:

  sparse   what a ptwt user has on this GPU: the same level operators applied with torch.sparse.mm, as the reference does
           (2-D: A_cols over the flattened batch, then A_rows; the operators are assembled from this package's tables)
  padded   this project's padded transform of the same input (wavedec2 / wavedec, mode="zero") on the per-level route
           (OPT_PYRAMID_MODE 2, OPT_PAIR_MODE 2: one launch per level against one launch per level)

Device events; every leg warmed; a timed window of at least 0.2 s per leg; the legs alternate inside each repeat; min / median /
max over the repeats.  One JSON line per shape: microseconds per call, the two ratios, and the share of the 8 TB/s HBM peak on the
compulsory bytes (input + coefficients, from the shapes).

    python tools/boundary_bench.py [--repeats 5] [--shape 2d|1d]
"""
import argparse
import json
import sys

import torch

sys.path.insert(0, ".")
import ptwt_amd  # noqa: E402
from ptwt_amd import _bwt, _engine  # noqa: E402
from ptwt_amd._wavelets import host_taps  # noqa: E402

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


def sparse_legs(x, wavelet, level):
    """The reference's level loop on torch.sparse.mm (src/ptwt/matmul_transform.py:409-430, matmul_transform_2.py:514-529)."""
    bank = _bwt.bank(host_taps(wavelet), "qr", "analysis")
    ops = {}

    def op(n):
        if n not in ops:
            ops[n] = _bwt.sparse_level(bank, n, x.device, x.dtype)
        return ops[n]

    def pad_even(t, dims):
        pad = []
        for d in reversed(dims):
            pad += [0, t.shape[d] % 2]
        return torch.nn.functional.pad(t, pad) if any(pad) else t

    if x.dim() == 2:
        def run():
            lo, out = x.T, []
            for _ in range(level):
                if lo.shape[0] % 2:
                    lo = torch.nn.functional.pad(lo, (0, 0, 0, 1))
                c = torch.sparse.mm(op(lo.shape[0]), lo)
                lo, hi = torch.split(c, c.shape[0] // 2, dim=0)
                out.append(hi)
            return [s.T for s in [lo] + out[::-1]]
    else:
        def run():
            ll, out = x, []
            for _ in range(level):
                ll = pad_even(ll, (-2, -1))
                b, h, w = ll.shape
                ll = torch.sparse.mm(op(w), ll.reshape(b * h, w).T).T.reshape(b, h, w)
                ll = torch.sparse.mm(op(h), ll.permute(1, 0, 2).reshape(h, b * w)).reshape(h, b, w).permute(1, 0, 2)
                a, d = torch.split(ll, h // 2, dim=-2)
                ll, lh = torch.split(a, w // 2, dim=-1)
                hl, hh = torch.split(d, w // 2, dim=-1)
                out.append((lh, hl, hh))
            return [ll] + out[::-1]
    return run


def bench(shape, wavelet, level, repeats):
    x = torch.randn(*shape, device="cuda", dtype=torch.float32)
    ndim = len(shape) - 1
    dec = (ptwt_amd.MatrixWavedec if ndim == 1 else ptwt_amd.MatrixWavedec2)(wavelet, level=level)
    padded_fn = ptwt_amd.wavedec if ndim == 1 else ptwt_amd.wavedec2
    legs = {"boundary": lambda: dec(x), "padded": lambda: padded_fn(x, wavelet, level=level, mode="zero"),
            "sparse": sparse_legs(x, wavelet, level)}
    # the sparse leg computes what the boundary leg computes
    got, want = dec(x), legs["sparse"]()
    flat = lambda c: [t for e in c for t in (e if isinstance(e, tuple) else [e])]  # noqa: E731
    err = max(float((a - b).abs().max()) for a, b in zip(flat(got), flat(want)))
    coef_padded = sum(t.numel() for t in flat(legs["padded"]()))
    del got, want
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(window(fn))
    stat = {k: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v)) for k, v in times.items()}
    esz = x.element_size()
    byts = {"boundary": 2 * x.numel() * esz, "padded": (x.numel() + coef_padded) * esz}
    res = dict(shape=list(shape), wavelet=wavelet, level=level, dtype="float32", repeats=repeats, us=stat,
               sparse_over_boundary=stat["sparse"]["median"] / stat["boundary"]["median"],
               boundary_over_padded=stat["boundary"]["median"] / stat["padded"]["median"],
               padded_spread=(stat["padded"]["max"] - stat["padded"]["min"]) / stat["padded"]["median"],
               boundary_spread=(stat["boundary"]["max"] - stat["boundary"]["min"]) / stat["boundary"]["median"],
               compulsory_bytes=byts,
               hbm_share={k: byts[k] / (stat[k]["median"] * 1e-6) / HBM_PEAK for k in byts},
               sparse_vs_boundary_max_abs_diff=err)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", choices=["2d", "1d", "both"], default="both")
    args = ap.parse_args()
    _engine.set_option(_engine.OPT_PYRAMID_MODE, 2)
    _engine.set_option(_engine.OPT_PAIR_MODE, 2)
    if args.shape in ("2d", "both"):
        bench((64, 1024, 1024), "db4", 3, args.repeats)
    if args.shape in ("1d", "both"):
        bench((32, 1000000), "db5", 10, args.repeats)


if __name__ == "__main__":
    main()
