"""keep_threshold / sparsify on whole coefficient containers against the emulation a user writes with torch operations (``abs`` /
``flatten`` / ``cat`` / ``sort`` for the value — ``sparsify._composed_kth`` —, ``thresholding._composed`` to apply) at the same commit.

  value      ``keep_threshold(coeffs, 0.05)`` on the containers of ``wavedec2`` db4 level 3 of 64 x 1024 x 1024 (float32 and float64),
             ``wavedec`` db5 level 10 of 32 x 1 000 000 and ``wavedec3`` db2 level 3 of 8 x 256^3 (22 tensors): the streaming selection
             (the default at these sizes) against the sort
  sparsify   ``sparsify(coeffs, 0.05, "hard")`` on the same containers against the emulation
  routes     the two selections against each other and the sort where both run: 4096 images of 33 x 33 and 64 images at the LDS capacity
  pipeline   ``waverec2(sparsify(wavedec2(x), 0.05))`` against the same pipeline with the emulation in the middle

Protocol of tools/estimator_bench.py: device events; every leg warmed; a timed window of at least 0.2 s per leg; the legs alternate
inside each repeat; min / median / max over the repeats (five by default).  Before timing, the legs are compared at the timed size:
bit for bit, the selection computes nothing.  One JSON line per cell goes to stdout and to ``--out`` (default
profiles/sparsify_bench.jsonl): microseconds per call, the share of the 8 TB/s HBM peak on the counted bytes (one read of the pooled
bands per digit pass, plus one read and one write of the container for ``sparsify``), ``spread`` — the widest max - min over the windows
of a leg — and, per other leg, ``not_ahead``: the first leg's median does not lead that leg's by more than that spread.

    python tools/sparsify_bench.py [--repeats 5] [--cells value,sparsify,routes,pipeline] [--small] [--out FILE]
"""
import argparse
import importlib
import json
import math
import os
import sys

import torch

sys.path.insert(0, ".")
import ptwt_amd  # noqa: E402
from ptwt_amd import estimators as E, thresholding as T  # noqa: E402
from tools.estimator_bench import HBM_PEAK, flat, measure, tree_map  # noqa: E402

S = importlib.import_module("ptwt_amd.sparsify")  # (the package attribute of that name is the function)
KEEP = 0.05


def pool_of(coeffs):
    """(the pooled tensors, leading axes, leading shape, pooled elements per image) of ``sparsify(coeffs, ...)``."""
    leaves, pooled, lead, shape, n = S._pool(coeffs, False, None)
    return [leaves[i] for i in pooled], lead, shape, n


def emulate_value(coeffs):
    ts, lead, shape, n = pool_of(coeffs)
    return S._composed_kth(ts, lead, S._k_of(KEEP, n)).reshape(shape)


def emulate_sparsify(coeffs):
    v = emulate_value(coeffs)
    if isinstance(coeffs, torch.Tensor):
        return T._composed(coeffs, v, None, S.MODES["hard"], 0.0)
    return type(coeffs)([coeffs[0]] + [tree_map(lambda t: T._composed(t, v, None, S.MODES["hard"], 0.0), e) for e in coeffs[1:]])


def forced(fn):
    def run():
        S.FORCE_STREAM = True
        try:
            return fn()
        finally:
            S.FORCE_STREAM = False

    return run


def emit_cell(emit, name, what, shape, dtype, legs, byts, repeats):
    outs = {k: flat(fn()) for k, fn in legs.items()}
    first = next(iter(outs))
    same = all(torch.equal(u, v) for k, o in outs.items() if k != first for u, v in zip(outs[first], o))
    # (the pipeline's synthesis reads dense tensors on one leg and views of level buffers on the other: the same kernels, but only the
    # values and the sparsified containers are held to the bit)
    assert same or (name == "pipeline" and all(torch.allclose(u, v, rtol=1e-5, atol=1e-5) for k, o in outs.items() if k != first
                                               for u, v in zip(outs[first], o))), (name, what, "the legs differ")
    del outs
    stat, not_ahead = measure(legs, repeats)
    emit(dict(cell=name, call=what, shape=list(shape), dtype=str(dtype).split(".")[-1], repeats=repeats, us=stat, not_ahead=not_ahead,
              spread=max(v["max"] - v["min"] for v in stat.values()), counted_bytes=byts,
              hbm_share={k: byts / (v["median"] * 1e-6) / HBM_PEAK for k, v in stat.items()}, legs_bit_equal=same))


def passes(dtype, n, tensors):
    return 1 if n <= E.lds_capacity(dtype) and tensors <= S.max_segments() else len(E.stream_plan(dtype))


def bench_container(name, dec, shape, wavelet, level, dtype, repeats, emit, cells):
    x = torch.randn(*shape, device="cuda", dtype=dtype, generator=torch.Generator(device="cuda").manual_seed(1))
    coeffs = dec(x, wavelet, level=level)
    del x
    ts, _, lshape, n = pool_of(coeffs)
    images = math.prod(lshape)
    esz = ts[0].element_size()
    select = passes(dtype, n, len(ts)) * n * images * esz
    if "value" in cells:
        emit_cell(emit, name, f"keep_threshold {KEEP} ({n} per image in {len(ts)} tensors)", shape, dtype,
                  {"kernel": lambda: ptwt_amd.keep_threshold(coeffs, KEEP), "emulation": lambda: emulate_value(coeffs)}, select, repeats)
    if "sparsify" in cells:
        byts = select + 2 * sum(t.numel() * esz for t in flat(coeffs))
        emit_cell(emit, name, f"sparsify {KEEP} hard", shape, dtype,
                  {"kernel": lambda: ptwt_amd.sparsify(coeffs, KEEP), "emulation": lambda: emulate_sparsify(coeffs)}, byts, repeats)


def bench_routes(shape, dtype, repeats, emit):
    x = torch.randn(*shape, device="cuda", dtype=dtype, generator=torch.Generator(device="cuda").manual_seed(1))
    n = x.numel() // shape[0]
    k = S._k_of(KEEP, n)
    emit_cell(emit, "routes", f"keep_threshold {KEEP} ({n} per image)", shape, dtype, {
        "lds": lambda: ptwt_amd.keep_threshold(x, k, lead=1),
        "stream": forced(lambda: ptwt_amd.keep_threshold(x, k, lead=1)),
        "emulation": lambda: S._composed_kth([x], 1, k),
    }, x.numel() * x.element_size(), repeats)


def bench_pipeline(shape, repeats, emit):
    x = torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    emit_cell(emit, "pipeline", "waverec2(sparsify(wavedec2))", shape, x.dtype, {
        "kernel": lambda: ptwt_amd.waverec2(ptwt_amd.sparsify(ptwt_amd.wavedec2(x, "db4", level=3), KEEP), "db4"),
        "emulation": lambda: ptwt_amd.waverec2(emulate_sparsify(ptwt_amd.wavedec2(x, "db4", level=3)), "db4"),
    }, 2 * x.numel() * x.element_size(), repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cells", default="value,sparsify,routes,pipeline")
    ap.add_argument("--small", action="store_true", help="small shapes: a check that every leg runs and agrees, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "sparsify_bench.jsonl"))
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
        if "value" in cells or "sparsify" in cells:
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
