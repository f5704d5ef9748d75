"""Boundary-wavelet transforms (MatrixWavedec2 / MatrixWavedec) against two yardsticks that are not the code under test:

  sparse   what a ptwt user has on this GPU: the same level operators applied with torch.sparse.mm, as the reference does
           (2-D: A_cols over the flattened batch, then A_rows; the operators are assembled from this package's tables)
  padded   this project's padded transform of the same input (wavedec2 / wavedec, mode="zero") on the per-level route
           (OPT_PYRAMID_MODE 2, OPT_PAIR_MODE 2: one launch per level against one launch per level)

Device events; every leg warmed; a timed window of at least 0.2 s per leg; the legs alternate inside each repeat; min / median /
max over the repeats.  One JSON line per shape: microseconds per call, the two ratios, and the share of the 8 TB/s HBM peak on the
compulsory bytes (input + coefficients, from the shapes).

The 3-D section (MatrixWavedec3 / MatrixWaverec3, --shape 3d) has the same protocol and four legs per direction: the fused route
(kernel ids 30 / 31), the composed route of the same library (the axis passes 28 / 29, forced by ``_bwt.FORCE_COMPOSED3``, alternating
with the fused leg in the same process), wavedec3 / waverec3 with mode="zero", and the level operators through torch.sparse.mm.
--shape cells times ONE level per (direction, dtype, L) cell of the fused envelope, fused against composed: the routing table
``_bwt.COMPOSED3_CELLS`` is filled from its verdicts (fused only where its median beats the composed median by more than the spread of
the windows).

--shape packets: WaveletPacket(mode="boundary") — the whole tree of a depth (analysis) and reconstruct() from its leaves (synthesis) on
the default subtree route (kernel ids 32 / 33 where ``_bwt.tree_route`` takes them), on per-level launches of the same library
(``_bwt.FORCE_PER_LEVEL_TREE``, alternating in the same process) and WaveletPacket(mode="zero") of the same depth; the verdict per
(direction, dtype) cell fills ``_bwt.PER_LEVEL_TREE_CELLS`` by the rule of the 3-D cells.

    python tools/boundary_bench.py [--repeats 5] [--shape 2d|1d|3d|cells|packets]
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


def sparse_legs3(x, wavelet, level):
    """MatrixWavedec3 / MatrixWaverec3 as the reference runs them: one torch.sparse.mm per axis and level."""
    taps = host_taps(wavelet)
    banks = {"analysis": _bwt.bank(taps, "qr", "analysis"), "synthesis": _bwt.bank(taps, "qr", "synthesis")}
    ops = {}

    def op(which, n):
        if (which, n) not in ops:
            ops[which, n] = _bwt.sparse_level(banks[which], n, x.device, x.dtype)
        return ops[which, n]

    def along(which, t, dim):
        t = t.transpose(dim, -1)
        shape = t.shape
        out = torch.sparse.mm(op(which, shape[-1]), t.reshape(-1, shape[-1]).T).T
        return out.reshape(shape).transpose(dim, -1)

    def dec():
        lll, out = x, []
        for _ in range(level):
            pad = [v for n in reversed(lll.shape[1:]) for v in (0, n % 2)]
            lll = torch.nn.functional.pad(lll, pad) if any(pad) else lll
            for dim in (3, 2, 1):
                lll = along("analysis", lll, dim)
            b, d, h, w = lll.shape
            planes = lll.reshape(b, 2, d // 2, 2, h // 2, 2, w // 2).permute(0, 1, 3, 5, 2, 4, 6).reshape(b, 8, d // 2, h // 2, w // 2)
            lll = planes[:, 0]
            out.append([planes[:, s] for s in range(1, 8)])
        return [lll] + out[::-1]

    def rec(coeffs):
        lll = coeffs[0]
        for bands in coeffs[1:]:
            lll = lll[:, : bands[0].shape[1], : bands[0].shape[2], : bands[0].shape[3]]
            p = [lll] + list(bands)
            halves = [torch.cat([torch.cat([p[q], p[q + 1]], -1), torch.cat([p[q + 2], p[q + 3]], -1)], -2) for q in (0, 4)]
            lll = torch.cat(halves, -3)
            for dim in (1, 2, 3):
                lll = along("synthesis", lll, dim)
        return lll

    return dec, rec


def _stats(times):
    return {k: dict(min=min(v), median=sorted(v)[len(v) // 2], max=max(v)) for k, v in times.items()}


def _timed(legs, repeats):
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            times[k].append(window(fn))
    return _stats(times)


def _forced(fn):
    def run():
        _bwt.FORCE_COMPOSED3 = True
        try:
            return fn()
        finally:
            _bwt.FORCE_COMPOSED3 = False
    return run


def _bricks(fn):
    """The leg on the brick kernels for every cell of the envelope, whatever ``_bwt.COMPOSED3_CELLS`` routes today."""
    def run():
        keep = set(_bwt.COMPOSED3_CELLS)
        _bwt.COMPOSED3_CELLS.clear()
        try:
            return fn()
        finally:
            _bwt.COMPOSED3_CELLS.update(keep)
    return run


def _flat3(coeffs):
    """The tensors of a 3-D coefficient container (dicts or lists of details), in order."""
    out = []
    for entry in coeffs:
        if isinstance(entry, dict):
            out.extend(entry.values())
        elif isinstance(entry, (list, tuple)):
            out.extend(entry)
        else:
            out.append(entry)
    return out


def bench3(shape, wavelet, level, repeats):
    x = torch.randn(*shape, device="cuda", dtype=torch.float32)
    dec, rec = ptwt_amd.MatrixWavedec3(wavelet, level=level), ptwt_amd.MatrixWaverec3(wavelet)
    sdec, srec = sparse_legs3(x, wavelet, level)
    flat = _flat3
    coeffs = dec(x)
    flat_c = [coeffs[0]] + [[d[k] for k in ("aad", "ada", "add", "daa", "dad", "dda", "ddd")] for d in coeffs[1:]]
    err = max(float((a - b).abs().max()) for a, b in zip(flat(coeffs), flat(sdec())))
    err_rec = float((rec(coeffs) - srec(flat_c)).abs().max())
    padded_c = ptwt_amd.wavedec3(x, wavelet, level=level, mode="zero")
    coef_padded = sum(t.numel() for t in flat(padded_c))
    esz, res = x.element_size(), {}
    for direction, legs in (("analysis", {"fused": _bricks(lambda: dec(x)), "composed": _forced(lambda: dec(x)),
                                          "padded": lambda: ptwt_amd.wavedec3(x, wavelet, level=level, mode="zero"), "sparse": sdec}),
                            ("synthesis", {"fused": _bricks(lambda: rec(coeffs)), "composed": _forced(lambda: rec(coeffs)),
                                           "padded": lambda: ptwt_amd.waverec3(padded_c, wavelet), "sparse": lambda: srec(flat_c)})):
        stat = _timed(legs, repeats)
        byts = {"fused": 2 * x.numel() * esz, "composed": 2 * x.numel() * esz, "padded": (x.numel() + coef_padded) * esz,
                "sparse": 2 * x.numel() * esz}
        med = {k: v["median"] for k, v in stat.items()}
        res[direction] = dict(us=stat, fused_over_composed=med["fused"] / med["composed"], fused_over_padded=med["fused"] / med["padded"],
                              fused_over_sparse=med["fused"] / med["sparse"],
                              spread={k: (v["max"] - v["min"]) / v["median"] for k, v in stat.items()},
                              hbm_share={k: byts[k] / (med[k] * 1e-6) / HBM_PEAK for k in byts})
    print(json.dumps(dict(shape=list(shape), wavelet=wavelet, level=level, dtype="float32", repeats=repeats,
                          compulsory_bytes=2 * x.numel() * esz, sparse_vs_fused_max_abs_diff=[err, err_rec], **res)), flush=True)


def cells3(repeats):
    """One level per (direction, dtype, L) cell of the fused 3-D envelope on a 4 x 128^3 volume: fused against composed."""
    for dtype in (torch.float32, torch.float64):
        for flen, wavelet in ((2, "haar"), (4, "db2"), (6, "db3"), (8, "db4")):
            taps = host_taps(wavelet)
            x = torch.randn(4, 128, 128, 128, device="cuda", dtype=dtype)
            bands = [torch.randn(4, 64, 64, 64, device="cuda", dtype=dtype) for _ in range(8)]
            bk_a, bk_s = _bwt.bank(taps, "qr", "analysis"), _bwt.bank(taps, "qr", "synthesis")
            for direction, fn in ((0, lambda: _bwt.rows_level(x, bk_a, 0)), (1, lambda: _bwt.transposed_level(bands, bk_s, (128, 128, 128)))):
                stat = _timed({"fused": _bricks(fn), "composed": _forced(fn)}, repeats)  # (the kernel itself, whatever the table says)
                f, c = stat["fused"], stat["composed"]
                spread = max(f["max"] - f["min"], c["max"] - c["min"])
                print(json.dumps(dict(cell=[direction, str(dtype).split(".")[-1], flen], us=stat, fused_over_composed=f["median"] / c["median"],
                                      spread_us=spread, route="fused" if c["median"] - f["median"] > spread else "composed",
                                      hbm_share_fused=2 * x.numel() * x.element_size() / (f["median"] * 1e-6) / HBM_PEAK)), flush=True)


def _per_level(fn):
    def run():
        _bwt.FORCE_PER_LEVEL_TREE = True
        try:
            return fn()
        finally:
            _bwt.FORCE_PER_LEVEL_TREE = False
    return run


def _subtree(fn):
    """The leg on the subtree kernels wherever the envelope allows, whatever ``_bwt.PER_LEVEL_TREE_CELLS`` routes today."""
    def run():
        keep = set(_bwt.PER_LEVEL_TREE_CELLS)
        _bwt.PER_LEVEL_TREE_CELLS.clear()
        try:
            return fn()
        finally:
            _bwt.PER_LEVEL_TREE_CELLS.update(keep)
    return run


def bench_packets(shape, wavelet, depth, dtype, repeats):
    x = torch.randn(*shape, device="cuda", dtype=dtype)
    leaf = "a" * depth

    def tree(mode):
        wp = ptwt_amd.WaveletPacket(x, wavelet, mode=mode, maxlevel=depth)
        wp[leaf]
        return wp

    grown = {"fused": _subtree(lambda: tree("boundary"))(), "per_level": _per_level(lambda: tree("boundary"))(), "padded": tree("zero")}
    keys = ptwt_amd.WaveletPacket.get_level(depth, "natural")
    err = max(float((grown["fused"][k] - grown["per_level"][k]).abs().max()) for k in keys)
    res = {}
    for direction, legs in (("analysis", {"fused": _subtree(lambda: tree("boundary")), "per_level": _per_level(lambda: tree("boundary")),
                                          "padded": lambda: tree("zero")}),
                            ("synthesis", {"fused": _subtree(grown["fused"].reconstruct), "per_level": _per_level(grown["per_level"].reconstruct),
                                           "padded": grown["padded"].reconstruct})):
        stat = _timed(legs, repeats)
        f, c = stat["fused"], stat["per_level"]
        spread = max(f["max"] - f["min"], c["max"] - c["min"])
        byts = (1 + depth) * x.numel() * x.element_size()  # the input (the leaves) once, every level written once
        res[direction] = dict(us=stat, fused_over_per_level=f["median"] / c["median"], fused_over_padded=f["median"] / stat["padded"]["median"],
                              spread_us=spread, route="subtree" if c["median"] - f["median"] > spread else "per_level",
                              hbm_share_fused=byts / (f["median"] * 1e-6) / HBM_PEAK)
    print(json.dumps(dict(shape=list(shape), wavelet=wavelet, depth=depth, dtype=str(dtype).split(".")[-1], repeats=repeats,
                          fused_vs_per_level_max_abs_diff=err, **res)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", choices=["2d", "1d", "both", "3d", "cells", "packets"], default="both")
    args = ap.parse_args()
    _engine.set_option(_engine.OPT_PYRAMID_MODE, 2)
    _engine.set_option(_engine.OPT_PAIR_MODE, 2)
    if args.shape in ("2d", "both"):
        bench((64, 1024, 1024), "db4", 3, args.repeats)
    if args.shape in ("1d", "both"):
        bench((32, 1000000), "db5", 10, args.repeats)
    if args.shape == "3d":
        bench3((8, 256, 256, 256), "db2", 3, args.repeats)
        bench3((32, 100, 100, 100), "db4", 2, args.repeats)
    if args.shape == "cells":
        cells3(args.repeats)
    if args.shape == "packets":
        bench_packets((4096, 4096), "db4", 6, torch.float32, args.repeats)
        bench_packets((32, 1024), "db4", 6, torch.float32, args.repeats)
        bench_packets((4096, 4096), "db4", 6, torch.float64, args.repeats)


if __name__ == "__main__":
    main()
