"""coeffs_to_array / ravel_coeffs / array_to_coeffs(copy=True) / unravel_coeffs(copy=True) on whole coefficient containers (kernels 59 / 60)
against the emulation a user writes with torch operations at the same commit: ``torch.full`` (``torch.empty`` where the blocks tile the
array) and one slice assignment per tensor — ``coeff_array._composed_to_array`` —, a ``reshape`` per tensor and one ``cat`` —
``_composed_ravel`` —, one ``clone`` per block — ``_composed_to_bands``.

  2d / 2d64   the ``wavedec2`` db4 level 3 container of 64 x 1024 x 1024 float32 / float64, ``mode="symmetric"`` (gaps, padding 0.0)
  2dper / 2dper64   the same in ``mode="periodization"`` (tight, ``padding=None``)
  1d          the ``wavedec`` db5 level 10 container of 32 x 1 000 000
  3d          the ``wavedec3`` db2 level 3 container of 8 x 256^3 (22 tensors)
  small       4096 images of 33 x 33, ``wavedec2`` db4 level 3
  pipeline    ``waverec2(array_to_coeffs(coeffs_to_array(wavedec2(x))))`` with ``copy=False`` and with ``copy=True`` against the same
              pipeline with the emulation in the middle

Protocol of tools/sparsify_bench.py: device events; every leg warmed; a timed window of at least 0.2 s per leg; the legs alternate inside
each repeat; min / median / max over the repeats (five by default).  Before timing, the legs are compared at the timed size, bit for bit.
One JSON line per cell goes to stdout and to ``--out`` (default profiles/pack_bench.jsonl): microseconds per call, the share of the
8 TB/s HBM peak on one read of the tensors plus one write of the array (the other direction: one read of the blocks, one write of the
tensors), ``spread`` and, per other leg, ``not_ahead`` as there.  The "kernel" legs run with ``coeff_array.COMPOSED_CELLS`` emptied
(:func:`on_kernels`), so every cell is measured on kernels 59 / 60 whatever the routing table holds at this commit: the table is what
this tool decides, not an input to it.

    python tools/pack_bench.py [--repeats 5] [--cells 2d,2d64,2dper,2dper64,1d,3d,small,pipeline] [--small] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys

import torch

sys.path.insert(0, ".")
import ptwt_amd  # noqa: E402
from tools.estimator_bench import flat  # noqa: E402
from tools.sparsify_bench import emit_cell  # noqa: E402

C = importlib.import_module("ptwt_amd.coeff_array")


def on_kernels(fn):
    """``fn`` with every cell on kernels 59 / 60: the routing table emptied around the call and put back."""
    def run():
        cells, C.COMPOSED_CELLS = C.COMPOSED_CELLS, set()
        try:
            return fn()
        finally:
            C.COMPOSED_CELLS = cells

    return run


def plans(coeffs, tight):
    """What the emulation needs, computed once: the layouts are host work both legs share."""
    p = C._parse("pack_bench", coeffs, None)
    shape, slices, _, _ = C._array_layout("pack_bench", p, tight)
    lead, n, rsl, shapes = C._ravel_layout(p)
    keys = [list(s) for s in rsl[1:]]
    return dict(tensors=C._flat(p), flat_slices=[slices[0]] + [s[k] for s in slices[1:] for k in s], shape=shape, slices=slices,
                sorted_tensors=C._flat(p, keys), axes=p.axes, rsl=rsl, shapes=shapes,
                flat_rsl=[rsl[0]] + [s[k] for s in rsl[1:] for k in s], flat_shapes=[shapes[0]] + [sh[k] for sh in shapes[1:] for k in sh])


def bench_container(name, dec, shape, wavelet, level, mode, dtype, fmt, repeats, emit):
    x = torch.randn(*shape, device="cuda", dtype=dtype, generator=torch.Generator(device="cuda").manual_seed(1))
    coeffs = dec(x, wavelet, level=level, mode=mode)
    del x
    tight = mode == "periodization" or fmt == "wavedec"
    padding = None if tight else 0.0
    q = plans(coeffs, tight)
    esz = q["tensors"][0].element_size()
    read = sum(t.numel() for t in q["tensors"]) * esz
    arr, slices = on_kernels(lambda: ptwt_amd.coeffs_to_array(coeffs, padding))()
    flat_arr, rsl, shapes = on_kernels(lambda: ptwt_amd.ravel_coeffs(coeffs))()
    what = f"{len(q['tensors'])} tensors, {'tight' if tight else 'gaps'}"
    emit_cell(emit, name, f"coeffs_to_array ({what})", shape, dtype, {
        "kernel": on_kernels(lambda: [ptwt_amd.coeffs_to_array(coeffs, padding)[0]]),
        "emulation": lambda: [C._composed_to_array(q["tensors"], q["flat_slices"], q["shape"], padding)]}, read + arr.numel() * esz, repeats)
    emit_cell(emit, name, f"ravel_coeffs ({what})", shape, dtype, {
        "kernel": on_kernels(lambda: [ptwt_amd.ravel_coeffs(coeffs)[0]]),
        "emulation": lambda: [C._composed_ravel(q["sorted_tensors"], q["axes"])]}, 2 * read, repeats)
    emit_cell(emit, name, f"array_to_coeffs copy=True ({what})", shape, dtype, {
        "kernel": on_kernels(lambda: flat(ptwt_amd.array_to_coeffs(arr, slices, fmt, copy=True))),
        "emulation": lambda: C._composed_to_bands([arr[s] for s in q["flat_slices"]])}, 2 * read, repeats)
    emit_cell(emit, name, f"unravel_coeffs copy=True ({what})", shape, dtype, {
        "kernel": on_kernels(lambda: sorted_flat(ptwt_amd.unravel_coeffs(flat_arr, rsl, shapes, fmt, copy=True))),
        "emulation": lambda: C._composed_to_bands([flat_arr[..., s].unflatten(-1, sh) for s, sh in zip(q["flat_rsl"], q["flat_shapes"])])},
        2 * read, repeats)


def sorted_flat(c):
    """The tensors of a container, every level in sorted key order (the order of the flat layout)."""
    out = [c[0]]
    for e in c[1:]:
        if isinstance(e, torch.Tensor):
            out.append(e)
        elif isinstance(e, dict):
            out += [e[k] for k in sorted(e)]
        else:
            out += [e[1], e[0], e[2]]  # ad, da, dd
    return out


def bench_pipeline(shape, repeats, emit):
    x = torch.randn(*shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    q = plans(ptwt_amd.wavedec2(x, "db4", level=3, mode="symmetric"), False)
    WD = ptwt_amd.WaveletDetailTuple2d

    def emulated(copy):
        def run():
            c = ptwt_amd.wavedec2(x, "db4", level=3, mode="symmetric")
            arr = C._composed_to_array([c[0]] + [t for e in c[1:] for t in e], q["flat_slices"], q["shape"], 0.0)
            views = [arr[s] for s in q["flat_slices"]]
            it = iter(C._composed_to_bands(views) if copy else views)
            return ptwt_amd.waverec2((next(it), *[WD(next(it), next(it), next(it)) for _ in c[1:]]), "db4")

        return run

    def fused(copy):
        def run():
            arr, slices = ptwt_amd.coeffs_to_array(ptwt_amd.wavedec2(x, "db4", level=3, mode="symmetric"), 0.0)
            return ptwt_amd.waverec2(ptwt_amd.array_to_coeffs(arr, slices, "wavedec2", copy=copy), "db4")

        return run

    for copy in (False, True):
        emit_cell(emit, "pipeline", f"waverec2(array_to_coeffs(coeffs_to_array(wavedec2)), copy={copy})", shape, x.dtype,
                  {"kernel": on_kernels(fused(copy)), "emulation": emulated(copy)}, 2 * x.numel() * x.element_size(), repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cells", default="2d,2d64,2dper,2dper64,1d,3d,small,pipeline")
    ap.add_argument("--small", action="store_true", help="small shapes: a check that every leg runs and agrees, not a measurement")
    ap.add_argument("--out", default=os.path.join("profiles", "pack_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    big = not args.small
    plane = (64, 1024, 1024) if big else (4, 128, 128)
    table = {
        "2d": (ptwt_amd.wavedec2, plane, "db4", 3, "symmetric", torch.float32, "wavedec2"),
        "2d64": (ptwt_amd.wavedec2, plane, "db4", 3, "symmetric", torch.float64, "wavedec2"),
        "2dper": (ptwt_amd.wavedec2, plane, "db4", 3, "periodization", torch.float32, "wavedec2"),
        "2dper64": (ptwt_amd.wavedec2, plane, "db4", 3, "periodization", torch.float64, "wavedec2"),
        "1d": (ptwt_amd.wavedec, (32, 1000000) if big else (4, 16384), "db5", 10 if big else 4, "symmetric", torch.float32, "wavedec"),
        "3d": (ptwt_amd.wavedec3, (8, 256, 256, 256) if big else (2, 32, 32, 32), "db2", 3 if big else 2, "symmetric", torch.float32, "wavedecn"),
        "small": (ptwt_amd.wavedec2, (4096, 33, 33) if big else (64, 33, 33), "db4", 3, "symmetric", torch.float32, "wavedec2"),
    }
    with open(args.out, "w") as f:
        def emit(res):
            line = json.dumps(res)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()

        for cell in args.cells.split(","):
            if cell == "pipeline":
                bench_pipeline(plane, args.repeats, emit)
            else:
                dec, shape, wavelet, level, mode, dtype, fmt = table[cell]
                bench_container(cell, dec, shape, wavelet, level, mode, dtype, fmt, args.repeats, emit)


if __name__ == "__main__":
    main()
