"""sparse_encode / sparse_decode on whole coefficient containers against the emulation a user writes with torch operations (``cat`` /
stable ``sort`` / ``sort`` / ``gather`` — ``sparse._composed_encode`` —, ``zeros`` / ``scatter`` — ``sparse._composed_decode``) at the same
commit.

  encode     ``sparse_encode(coeffs, 0.05)`` on the containers of ``wavedec2`` db4 level 3 of 64 x 1024 x 1024 (float32 and float64),
             ``wavedec`` db5 level 10 of 32 x 1 000 000 and ``wavedec3`` db2 level 3 of 8 x 256^3: selection + streaming compaction
             (the default at these sizes) against the emulation
  decode     ``sparse_decode`` of each against the emulation
  routes     the LDS route against forced streaming and the emulation where both run: 4096 images of 33 x 33 and 64 images at the LDS
             capacity
  pipeline   ``waverec2(sparse_decode(sparse_encode(wavedec2(x), 0.05)))`` against the same pipeline with the emulation in the middle

Protocol of tools/sparsify_bench.py: device events; every leg warmed; a timed window of at least 0.2 s per leg; the legs alternate inside
each repeat; min / median / max over the repeats (five by default).  Before timing, the legs are compared at the timed size, bit for bit.
One JSON line per cell goes to stdout and to ``--out`` (default profiles/sparse_bench.jsonl): microseconds per call, the share of the
8 TB/s HBM peak on the compulsory bytes (encode: the selection's reads — one read of the pool per digit pass —, two more reads of the pool
and ``k (sizeof + 4)`` bytes written per image; decode: the container written once and ``k (sizeof + 4)`` read), ``spread`` and, per
other leg, ``not_ahead`` as there.

    python tools/sparse_bench.py [--repeats 5] [--cells encode,decode,routes,pipeline] [--small] [--out FILE]
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
from tools.estimator_bench import flat  # noqa: E402
from tools.sparsify_bench import KEEP, emit_cell, passes, pool_of  # noqa: E402

S = importlib.import_module("ptwt_amd.sparse")
SP = importlib.import_module("ptwt_amd.sparsify")


def emulate_encode(coeffs):
    ts, lead, shape, n = pool_of(coeffs)
    k = SP._k_of(KEEP, n)
    return S._composed_encode(ts, lead, k, None, k)


def emulate_decode(s):
    lay = s.layout
    outs = S._composed_decode(s.values, s.indices, s.counts, [shape for shape, _ in lay.entries], lay.n)
    return S._filled(lay.skeleton, outs, s.approx)


def parts(s):
    return [s.values.reshape(-1, s.layout.capacity), s.indices.reshape(-1, s.layout.capacity), s.counts.reshape(-1)]


def forced(fn):
    def run():
        S.FORCE_STREAM = True
        try:
            return fn()
        finally:
            S.FORCE_STREAM = False

    return run


def bench_container(name, dec, shape, wavelet, level, dtype, repeats, emit, cells):
    x = torch.randn(*shape, device="cuda", dtype=dtype, generator=torch.Generator(device="cuda").manual_seed(1))
    coeffs = dec(x, wavelet, level=level)
    del x
    ts, _, lshape, n = pool_of(coeffs)
    images, esz, k = math.prod(lshape), ts[0].element_size(), SP._k_of(KEEP, n)
    packed = images * k * (esz + 4)
    if "encode" in cells:
        byts = (passes(dtype, n, len(ts)) + 2) * n * images * esz + packed
        emit_cell(emit, name, f"sparse_encode {KEEP} ({n} per image in {len(ts)} tensors, k = {k})", shape, dtype,
                  {"kernel": lambda: parts(ptwt_amd.sparse_encode(coeffs, KEEP)), "emulation": lambda: list(emulate_encode(coeffs))}, byts, repeats)
    if "decode" in cells:
        s = ptwt_amd.sparse_encode(coeffs, KEEP)
        byts = n * images * esz + packed
        emit_cell(emit, name, f"sparse_decode (k = {k})", shape, dtype,
                  {"kernel": lambda: flat(ptwt_amd.sparse_decode(s))[1:], "emulation": lambda: flat(emulate_decode(s))[1:]}, byts, repeats)


def bench_routes(shape, dtype, repeats, emit):
    x = torch.randn(*shape, device="cuda", dtype=dtype, generator=torch.Generator(device="cuda").manual_seed(1))
    a = torch.zeros(shape[0], 1, device="cuda", dtype=dtype)  # (an approximation that stays out of the pool: one pool per image)
    coeffs = [a, x.reshape(shape[0], -1)]
    n = x.numel() // shape[0]
    k = SP._k_of(KEEP, n)
    byts = 3 * x.numel() * x.element_size() + shape[0] * k * (x.element_size() + 4)
    emit_cell(emit, "routes", f"sparse_encode {KEEP} ({n} per image, k = {k})", shape, dtype, {
        "lds": lambda: parts(ptwt_amd.sparse_encode(coeffs, k)),
        "stream": forced(lambda: parts(ptwt_amd.sparse_encode(coeffs, k))),
        "emulation": lambda: list(S._composed_encode(coeffs[1:], 1, k, None, k)),
    }, byts, repeats)


def bench_pipeline(shape, repeats, emit):
    x = torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))

    def emulated():
        c = ptwt_amd.wavedec2(x, "db4", level=3)
        ts, lead, lshape, n = pool_of(c)
        k = SP._k_of(KEEP, n)
        values, indices, counts = S._composed_encode(ts, lead, k, None, k)
        outs = iter(S._composed_decode(values, indices, counts, [tuple(t.shape) for t in ts], n))
        return ptwt_amd.waverec2([c[0]] + [type(e)(*[next(outs) for _ in e]) for e in c[1:]], "db4")

    emit_cell(emit, "pipeline", "waverec2(sparse_decode(sparse_encode(wavedec2)))", shape, x.dtype, {
        "kernel": lambda: ptwt_amd.waverec2(ptwt_amd.sparse_decode(ptwt_amd.sparse_encode(ptwt_amd.wavedec2(x, "db4", level=3), KEEP)), "db4"),
        "emulation": emulated,
    }, 2 * x.numel() * x.element_size(), repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cells", default="encode,decode,routes,pipeline")
    ap.add_argument("--small", action="store_true", help="small shapes: a check that every leg runs and agrees, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "sparse_bench.jsonl"))
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
        if "encode" in cells or "decode" in cells:
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
