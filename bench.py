#!/usr/bin/env python
"""bench.py — headline benchmark of the MI355X FWT engine (contract: see the task statement / DESIGN.md §5).

One "step" = one full ``wavedec2(x, "db4", level=3)`` over a 64 x 1024 x 1024 fp32 batch that is already
resident in HBM (BASELINE.json configs[1], the configuration the metric is quoted on).  With N GPUs every
rank transforms its own 64-image batch shard (weak scaling, no data-path collective: batch elements are
independent); the only collectives are the barrier and the max-over-ranks of the wall time.

Output: ONE JSON line on rank 0 with the whole-job throughput in Msamples/s and ms_per_step.  A plain run does only that: set up,
warm up, time the --steps steps, write the last step's outputs (--dump-outputs DIR), print the line.  With --full the line also holds
  "roofline"     achieved algorithmic GB/s of the dominant kernel (the level-1 analysis kernel), measured
                 live with HIP events on the launch stream inside the timed region, against 8 TB/s HBM peak;
  "whole_call"   (always there: compulsory bytes and fraction of the peak) + per-level kernel times, the rotating-outputs and
                 collector-on figures (loops of their own);
  "secondary"    the other BASELINE configurations (headline workload, N = 1);
  "cpu_baseline" the reference's CPU op sequence (oracle/torch_cpu_port.py) timed on this host's cores
                 (N = 1 only);
  "config4_shard" N > 1: config 4's per-GPU shard on every rank and the gather of its coefficients.

    python bench.py --gpus 1 --steps 50 --warmup 5 [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nproc-per-node 8 ... bench.py --gpus 8 --steps 50 --warmup 5
"""
from __future__ import annotations

import argparse
import json
import gc
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

# MIFWT_BENCH_DEVICE=cpu: control-flow dry run without a GPU (tests/test_bench_dryrun.py swaps the level engine for the
# tests' CPU stand-in and launches this file under torch.distributed.run with the gloo backend): tensors on the host, the
# synchronisation / event calls become host timers.  Never a measurement; the product engine itself has no CPU path.
DEVICE_KIND = os.environ.get("MIFWT_BENCH_DEVICE", "cuda")


def sync():
    if DEVICE_KIND == "cuda":
        torch.cuda.synchronize()


class _HostEvent:
    def record(self):
        self.t = time.perf_counter()

    def elapsed_time(self, other):
        return (other.t - self.t) * 1e3


def new_event():
    return torch.cuda.Event(enable_timing=True) if DEVICE_KIND == "cuda" else _HostEvent()


HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md: 8.0 TB/s; 6.29 TB/s measured copy)

WORKLOADS = {
    # name: (fn, shape, wavelet, level, mode, dtype)
    "wavedec2_db4_L3_64x1024x1024_f32": ("wavedec2", (64, 1024, 1024), "db4", 3, "reflect", torch.float32),
    "wavedec3_db2_L3_8x256x256x256_f32": ("wavedec3", (8, 256, 256, 256), "db2", 3, "zero", torch.float32),
    "wavedec2_db8_L4_64x4096x4096_f32": ("wavedec2", (64, 4096, 4096), "db8", 4, "reflect", torch.float32),
    # BASELINE configs[4] at a 32-image slice of the 128 (the path is linear in the batch): f16 storage extension
    "fswavedec2_sym16_L5_32x8192x8192_f16": ("fswavedec2", (32, 8192, 8192), "sym16", 5, "reflect", torch.float16),
    # ... and its reconstruction (matrix-core synthesis kernel, id 23)
    "fswaverec2_sym16_L5_32x8192x8192_f16": ("fswaverec2", (32, 8192, 8192), "sym16", 5, "reflect", torch.float16),
    # BASELINE configs[4] at its stated size (17 GB per input buffer)
    "fswavedec2_sym16_L5_128x8192x8192_f16": ("fswavedec2", (128, 8192, 8192), "sym16", 5, "reflect", torch.float16),
    # the reference's own 1-D speed test shape (examples/speed_tests/timeitconv_1d.py:16-36)
    "wavedec_db5_L10_32x1000000_f32": ("wavedec", (32, 1000000), "db5", 10, "periodic", torch.float32),
    # batches of image patches: the whole pyramid in one launch (kernel id 20)
    "wavedec2_db2_L3_4096x64x64_f32": ("wavedec2", (4096, 64, 64), "db2", 3, "reflect", torch.float32),
    "wavedec2_db2_L2_16384x32x32_f32": ("wavedec2", (16384, 32, 32), "db2", 2, "reflect", torch.float32),
    # the round trip's second half on config 2's coefficients: one streaming launch (kernel id 22)
    "waverec2_db4_L3_64x1024x1024_f32": ("waverec2", (64, 1024, 1024), "db4", 3, "reflect", torch.float32),
    "waverec2_db8_L4_64x4096x4096_f32": ("waverec2", (64, 4096, 4096), "db8", 4, "reflect", torch.float32),
    # config 2 with gradients: forward (one launch, kernel 16, as a differentiable op) + backward w.r.t. the data (per-level adjoints)
    "wavedec2_bwd_db4_L3_64x1024x1024_f32": ("wavedec2_bwd", (64, 1024, 1024), "db4", 3, "reflect", torch.float32),
    "wavedec2_bwd_db4_L3_64x1024x1024_f32_zero": ("wavedec2_bwd", (64, 1024, 1024), "db4", 3, "zero", torch.float32),
    # ... and the reconstruction with gradients w.r.t. every coefficient tensor (forward: kernel 22; backward: zero-mode analysis kernels)
    "waverec2_bwd_db4_L3_64x1024x1024_f32": ("waverec2_bwd", (64, 1024, 1024), "db4", 3, "reflect", torch.float32),
    # the other reconstructions (kernel ids 10, 18 / 15, 21)
    "waverec3_db2_L3_8x256x256x256_f32": ("waverec3", (8, 256, 256, 256), "db2", 3, "zero", torch.float32),
    "waverec_db5_L10_32x1000000_f32": ("waverec", (32, 1000000), "db5", 10, "periodic", torch.float32),
    "waverec2_db2_L3_4096x64x64_f32": ("waverec2", (4096, 64, 64), "db2", 3, "reflect", torch.float32),
    "waverec2_db5_L5_32x1000x1000_f32_periodic": ("waverec2", (32, 1000, 1000), "db5", 5, "periodic", torch.float32),
    # the reference's own published 2-D / separable / 3-D speed-test shapes (examples/speed_tests/timeitconv_2d.py:38-57,
    # timeitconv_2d_separable.py:43-85, timeitconv_3d.py:54-64)
    "wavedec2_db5_L5_32x1000x1000_f32_periodic": ("wavedec2", (32, 1000, 1000), "db5", 5, "periodic", torch.float32),
    "fswavedec2_db5_L5_32x1000x1000_f32_periodic": ("fswavedec2", (32, 1000, 1000), "db5", 5, "periodic", torch.float32),
    "wavedec3_db5_L3_32x100x100x100_f32_periodic": ("wavedec3", (32, 100, 100, 100), "db5", 3, "periodic", torch.float32),
    # the reference's second dtype (src/ptwt/constants.py:27): config 2 / config 3 in double precision
    "wavedec2_db4_L3_64x1024x1024_f64": ("wavedec2", (64, 1024, 1024), "db4", 3, "reflect", torch.float64),
    "waverec2_db4_L3_64x1024x1024_f64": ("waverec2", (64, 1024, 1024), "db4", 3, "reflect", torch.float64),
    "wavedec3_db2_L3_8x256x256x256_f64": ("wavedec3", (8, 256, 256, 256), "db2", 3, "zero", torch.float64),
    "waverec3_db2_L3_8x256x256x256_f64": ("waverec3", (8, 256, 256, 256), "db2", 3, "zero", torch.float64),
    # dry runs of the control flow (MIFWT_BENCH_DEVICE=cpu), not a benchmark shape
    "dryrun_wavedec2_db4_L2_6x96x96_f32": ("wavedec2", (6, 96, 96), "db4", 2, "reflect", torch.float32),
}


def level_extents(shape, flen, level):
    """Per-level sub-band extents of the transformed axes."""
    cur, out = list(shape), []
    for _ in range(level):
        cur = [(n + flen - 1) // 2 for n in cur]
        out.append(tuple(cur))
    return out


def prod(xs):
    p = 1
    for v in xs:
        p *= v
    return p


def algorithmic_bytes(batch, sig, flen, level, esize):
    """compulsory = input once + every returned coefficient once; per_level adds the
    write + re-read of the intermediate approximations; level1 = what the dominant kernel moves."""
    nd = len(sig)
    exts = level_extents(sig, flen, level)
    nb = 1 << nd
    compulsory = prod(sig) + sum((nb - 1) * prod(e) for e in exts) + prod(exts[-1])
    per_level = 0
    cur = sig
    for e in exts:
        per_level += prod(cur) + nb * prod(e)
        cur = e
    level1 = prod(sig) + nb * prod(exts[0])
    # two-levels-per-launch kernel (mifwt_dwt2_fwd_pair): input + level-1 details + all four level-2 bands
    pair12 = prod(sig) + (nb - 1) * prod(exts[0]) + nb * prod(exts[1]) if len(exts) > 1 else level1
    return (esize * batch * compulsory, esize * batch * per_level, esize * batch * level1, esize * batch * pair12)


def _flatten(coeffs):
    out = []
    for i, c in enumerate(coeffs):
        if isinstance(c, torch.Tensor):
            out.append((str(i), c))
        elif isinstance(c, dict):
            out.extend((f"{i}_{k}", v) for k, v in c.items())
        else:
            out.extend((f"{i}_{j}", v) for j, v in enumerate(c))
    return out


DUMP_BUDGET_BYTES = 48 << 20  # --dump-outputs: at most this much in all


def dump_outputs(out, path, budget=DUMP_BUDGET_BYTES):
    """--dump-outputs: what a caller of the timed path received from its last step, one ``path/<name>.npy`` per returned tensor
    (``out`` for a single tensor, ``out_<position>`` in a coefficient list or gradient tuple), float64 kept, every other dtype
    written as float32.  Over ``budget`` bytes in all, every array is cut to the same fraction of its elements, at positions drawn
    from a fixed seed (the same positions in every run with the same arguments), and written as the 1-D array of those elements
    in ascending flat order.  Returns {name: shape written}."""
    import numpy as np

    named = [("out", out)] if isinstance(out, torch.Tensor) else [("out_" + n, t) for n, t in _flatten(out)]
    named = [(n, t.detach()) for n, t in named]
    wdtype = [torch.float64 if t.dtype == torch.float64 else torch.float32 for _, t in named]
    total = sum(t.numel() * torch.empty(0, dtype=d).element_size() for (_, t), d in zip(named, wdtype))
    os.makedirs(path, exist_ok=True)
    written = {}
    for j, ((name, t), d) in enumerate(zip(named, wdtype)):
        if total > budget:
            k = max(1, t.numel() * budget // total)
            flat = torch.randint(t.numel(), (k,), generator=torch.Generator().manual_seed(20240 + j)).sort().values
            # (multi-dimensional indices: the coefficient tensors are strided views of level buffers, no dense copy of them)
            t = t[torch.unravel_index(flat.to(t.device), t.shape)]
        a = t.to(d).cpu().numpy()
        np.save(os.path.join(path, name + ".npy"), a)
        written[name] = list(a.shape)
    return written


def cpu_baseline(fn, shape, wavelet, level, mode, dtype):
    """The reference's CPU op sequence (oracle/torch_cpu_port.py) on this host's cores, on a bounded sample of the same workload:
    a slice of the batch sized to about 64 Mi samples (the path is linear in the batch), at most ~20 s of work."""
    from oracle import torch_cpu_port as P

    ports = {"wavedec2": P.wavedec2, "wavedec": P.wavedec, "wavedec3": P.wavedec3, "fswavedec2": P.fswavedec2, "waverec2": P.waverec2,
             "waverec": P.waverec, "waverec3": P.waverec3, "fswaverec2": P.fswaverec2}
    bwd = fn.endswith("_bwd")
    if bwd:
        fn = fn[:-4]
    if fn not in ports:
        return None
    port = ports[fn]
    cores = os.cpu_count() or 1
    per_item = prod(shape[1:])
    sample_b = max(1, min(shape[0], (64 << 20) // per_item))
    cdtype = torch.float32 if dtype == torch.float16 else dtype  # (the reference has no half path on the CPU: conv in fp32)
    x = torch.randn(sample_b, *shape[1:], dtype=cdtype)
    if fn == "waverec2" and not bwd:
        arg = P.wavedec2(x, wavelet, mode=mode, level=level)
        run = lambda sl: port(tuple([arg[0][sl]] + [tuple(t[sl] for t in lv) for lv in arg[1:]]), wavelet)  # noqa: E731
    elif fn == "fswaverec2":
        arg = P.fswavedec2(x, wavelet, mode=mode, level=level)
        run = lambda sl: port(tuple([arg[0][sl]] + [{k: v[sl] for k, v in d.items()} for d in arg[1:]]), wavelet)  # noqa: E731
    elif fn == "waverec":
        arg = P.wavedec(x, wavelet, mode=mode, level=level)
        run = lambda sl: port([t[sl] for t in arg], wavelet)  # noqa: E731
    elif fn == "waverec3":
        arg = P.wavedec3(x, wavelet, mode=mode, level=level)
        run = lambda sl: port(tuple([arg[0][sl]] + [{k: v[sl] for k, v in d.items()} for d in arg[1:]]), wavelet)  # noqa: E731
    elif bwd and fn == "waverec2":
        arg = P.wavedec2(x, wavelet, mode=mode, level=level)

        def run(sl):  # forward + backward w.r.t. every coefficient tensor through ATen's autograd
            leaves = [arg[0][sl].clone().requires_grad_(True)] + [t[sl].clone().requires_grad_(True) for lv in arg[1:] for t in lv]
            y = port(tuple([leaves[0]] + [tuple(leaves[1 + 3 * k : 4 + 3 * k]) for k in range(len(arg) - 1)]), wavelet)
            torch.autograd.grad(y, leaves, torch.ones_like(y))
    elif bwd:
        def run(sl):  # forward + backward w.r.t. the data through ATen's autograd, as the reference does it
            xs = x[sl].clone().requires_grad_(True)
            outs = [t for _, t in _flatten(port(xs, wavelet, mode=mode, level=level))]
            torch.autograd.grad(outs, xs, [torch.ones_like(t) for t in outs])
    else:
        run = lambda sl: port(x[sl], wavelet, mode=mode, level=level)  # noqa: E731
    # oneDNN's conv does not scale to every core of a big host: probe a few thread counts on a small slice
    # and keep the fastest (reported as "cores")
    probe = slice(0, max(1, sample_b // 8))
    best = (float("inf"), cores)
    for nt in sorted({cores, min(cores, 128), min(cores, 64), min(cores, 32), min(cores, 16)}):
        torch.set_num_threads(nt)
        run(slice(0, max(1, sample_b // 16)))  # warm-up (oneDNN primitive creation)
        t0 = time.perf_counter()
        run(probe)
        best = min(best, (time.perf_counter() - t0, nt))
    torch.set_num_threads(best[1])
    times = []
    t_end = time.perf_counter() + 20.0
    while len(times) < 5 and (time.perf_counter() < t_end or not times):
        t0 = time.perf_counter()
        run(slice(0, sample_b))
        times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    return {
        "value": round(sample_b * per_item / med / 1e6, 2),
        "unit": "Msamples/s",
        "cores": torch.get_num_threads(),
        "kind": "port",
        "sample": f"{sample_b}x{'x'.join(map(str, shape[1:]))} {str(cdtype).split('.')[-1]} of the {shape[0]} batch elements, {fn} {wavelet} level {level} {mode}, "
                  f"median of {len(times)} runs (min {min(times):.4f}s, median {med:.4f}s), best of the probed thread counts "
                  f"on a {cores}-core host; the ATen ops of ptwt's CPU path for this function (oracle/torch_cpu_port.py; "
                  "/root/reference itself cannot travel to the GPU box)",
    }


def profiled_traffic(workload, kernel_label=""):
    """(HBM bytes per launch of the dominant kernel, name of the committed PMC summary it comes from): rocprofv3 --pmc
    FETCH_SIZE / WRITE_SIZE in separate passes, FETCH_SIZE x2 gfx950 correction (tools/pmc_workload.sh, tools/gpu_pmc_pyr.sh +
    tools/summarize_prof.py).  PMC counters cannot be collected from inside this process, so the value is the one measured
    when the newest profile of the SAME workload and kernel under profiles/ was taken; (None, None) if there is none."""
    pdir = os.path.join(ROOT, "profiles")
    names = sorted(os.listdir(pdir), reverse=True) if os.path.isdir(pdir) else []
    for name in names:  # per-workload summaries (round 3 on)
        if name.endswith(f"_pmc_{workload}.json"):
            try:
                with open(os.path.join(pdir, name)) as f:
                    prof = json.load(f)
                token = (kernel_label.split() or [""])[0]
                if token.endswith("_kernel") and token not in prof.get("kernel", ""):
                    continue  # (a summary taken when another kernel served this workload: not this launch's traffic)
                return prof.get("hbm_traffic_bytes"), "profiles/" + name
            except Exception:
                return None, None
    if workload != "wavedec2_db4_L3_64x1024x1024_f32":
        return None, None
    for name in names:
        if name.endswith("_pmc_level1.json") and not name.startswith("r01a"):
            try:
                with open(os.path.join(pdir, name)) as f:
                    prof = json.load(f)
                fam = next((k for k in ("pyr", "roll", "pair", "tile") if k in kernel_label), "tile")
                if fam not in prof.get("kernel", ""):
                    continue
                return prof.get("hbm_traffic_bytes"), "profiles/" + name
            except Exception:
                return None, None
    return None, None


# What else the default run times after the headline line's own measurements (whole calls, a few seconds in total): the other
# BASELINE configs' per-GPU shapes, both directions, so that they are driver-timed figures and not builder-run ones.
SECONDARY = ["waverec2_db4_L3_64x1024x1024_f32", "wavedec3_db2_L3_8x256x256x256_f32", "waverec3_db2_L3_8x256x256x256_f32",
             "wavedec2_db8_L4_64x4096x4096_f32", "waverec2_db8_L4_64x4096x4096_f32", "wavedec2_bwd_db4_L3_64x1024x1024_f32",
             "waverec2_bwd_db4_L3_64x1024x1024_f32",
             # round 5: config 5's per-GPU slice both ways, the f64 forms of configs 2 / 3, the reference's own published shapes
             "fswavedec2_sym16_L5_32x8192x8192_f16", "fswaverec2_sym16_L5_32x8192x8192_f16",
             "wavedec2_db4_L3_64x1024x1024_f64", "wavedec3_db2_L3_8x256x256x256_f64", "waverec3_db2_L3_8x256x256x256_f64",
             "wavedec2_db5_L5_32x1000x1000_f32_periodic", "wavedec3_db5_L3_32x100x100x100_f32_periodic"]


def secondary_lines(dev, steps=20, warmup=5, buffers=3):
    """[{workload, ms_per_step, frac, ...}] for the SECONDARY workloads: K whole calls back to back on rotating inputs resident in
    HBM (results dropped, as in the headline loop), host clock around sync()s; frac = compulsory bytes / time / 8 TB/s."""
    import ptwt_amd

    out = []
    for name in SECONDARY:
        fn_name, shape, wavelet, level, mode, dtype = WORKLOADS[name]
        half_scope = ptwt_amd.half_storage(dtype == torch.float16)  # (fp16 storage is an engine extension, scoped to this workload)
        half_scope.__enter__()
        try:
            bwd = fn_name.endswith("_bwd")
            fn = getattr(ptwt_amd, fn_name[:-4] if bwd else fn_name)
            xs = [torch.randn(*shape, dtype=torch.float32 if dtype == torch.float16 else dtype, device=dev).to(dtype) for _ in range(buffers)]
            if bwd and "rec" in fn_name:  # (2-D containers: the approximation, then three detail bands per level)
                ana = getattr(ptwt_amd, fn_name[:-4].replace("rec", "dec"))
                with torch.no_grad():
                    sets = [ana(x, wavelet, mode=mode, level=level) for x in xs]
                args_ = [[t.contiguous().requires_grad_(True) for _, t in _flatten(c)] for c in sets]
                del sets, xs
                gout = torch.randn(*shape, dtype=dtype, device=dev)

                def call(lv):
                    y = fn((lv[0], *[tuple(lv[1 + 3 * k : 4 + 3 * k]) for k in range((len(lv) - 1) // 3)]), wavelet)
                    return torch.autograd.grad(y, lv, gout)
            elif bwd:
                args_ = [x.requires_grad_(True) for x in xs]
                with torch.no_grad():
                    gouts = [torch.randn_like(t) for _, t in _flatten(fn(xs[0], wavelet, mode=mode, level=level))]
                call = lambda a: torch.autograd.grad([t for _, t in _flatten(fn(a, wavelet, mode=mode, level=level))], a, gouts)  # noqa: E731
            elif "rec" in fn_name:
                ana = getattr(ptwt_amd, fn_name.replace("rec", "dec"))
                args_ = [ana(x, wavelet, mode=mode, level=level) for x in xs]
                del xs
                call = lambda a: fn(a, wavelet)  # noqa: E731
            else:
                args_ = xs
                call = lambda a: fn(a, wavelet, mode=mode, level=level)  # noqa: E731
            for i in range(warmup):
                call(args_[i % buffers])
            sync()
            # a first short loop sizes the timed one to ~60 ms (a 20-step loop of a 0.1 ms call is over before the clocks settle:
            # 0.372 against 0.338 ms for wavedec3 in round 4's first runs), and doubles as the warm-up
            t0 = time.perf_counter()
            for i in range(steps):
                call(args_[i % buffers])
            sync()
            est = (time.perf_counter() - t0) / steps
            n_timed = max(steps, min(400, int(0.06 / max(est, 1e-6))))  # (per workload: a fast one must not lengthen the slow ones' loops)
            t0 = time.perf_counter()
            for i in range(n_timed):
                call(args_[i % buffers])
            sync()
            ms = (time.perf_counter() - t0) / n_timed * 1e3
            flen = len(ptwt_amd._wavelets.as_wavelet(wavelet))
            comp_b = algorithmic_bytes(shape[0], shape[1:], flen, level, torch.empty(0, dtype=dtype).element_size())[0] * (2 if bwd else 1)
            out.append({"workload": name, "ms_per_step": round(ms, 4), "steps": n_timed, "compulsory_bytes": comp_b,
                        "Msamples_per_s": round(prod(shape) / ms / 1e3, 1),
                        "frac": round(comp_b / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)})
            del args_
        except Exception as exc:  # never let a secondary figure break the benchmark line
            out.append({"workload": name, "error": repr(exc)[:200]})
        finally:
            half_scope.__exit__(None, None, None)
        if DEVICE_KIND == "cuda":
            torch.cuda.empty_cache()
    # a learnable-wavelet training step (the reason the reference keeps its taps in the autograd graph, src/ptwt/_util.py:115-132;
    # examples/network_compression/wavelet_linear.py:118,150): wavedec2 of config 2's batch with the four filters as leaf tensors on the
    # GPU, forward + backward w.r.t. the data AND the decomposition filters; taps read by the kernels from device memory (no host
    # synchronisation), and the same step with the taps read back to the host per call
    if DEVICE_KIND == "cuda":
        name = "wavedec2_learnable_step_db4_L3_64x1024x1024_f32"
        try:
            from ptwt_amd import _wavelets

            wv = _wavelets.as_wavelet("db4")
            x = torch.randn(64, 1024, 1024, device=dev)
            res = {}
            for how in ("auto", "never"):
                ptwt_amd.set_device_taps(how)
                taps = [torch.tensor(list(f), dtype=torch.float64, device=dev, requires_grad=True) for f in wv.filter_bank]

                def tstep():
                    xx = x.detach().requires_grad_(True)
                    c = ptwt_amd.wavedec2(xx, tuple(taps), mode="reflect", level=3)
                    loss = c[0].square().mean() + sum(t.square().mean() for lv in c[1:] for t in lv)
                    return torch.autograd.grad(loss, [xx] + taps[:2])

                for _ in range(3):
                    tstep()
                sync()
                t0 = time.perf_counter()
                for _ in range(10):
                    tstep()
                sync()
                res[how] = (time.perf_counter() - t0) / 10 * 1e3
            out.append({"workload": name, "ms_per_step": round(res["auto"], 3), "host_taps_ms_per_step": round(res["never"], 3),
                        "note": "forward + backward w.r.t. data and dec filters (leaf tensors on the GPU); ms_per_step: taps read by the fused kernels "
                                "from device memory, no synchronisation; host_taps: the bank copied to the host per call (start of round 6, first "
                                "tap-gradient kernel + transposed copies: 24.2 ms)"})
        except Exception as exc:
            out.append({"workload": name, "error": repr(exc)[:200]})
        finally:
            ptwt_amd.set_device_taps("auto")
            torch.cuda.empty_cache()
    # launch-bound calls: the same call sequence eager and replayed from a HIP graph (ptwt_amd.capture) — host time is what the
    # eager call costs on a small batch, the replay runs at the kernels' own time
    if DEVICE_KIND == "cuda":
        for shape, wavelet, level, mode in (((16, 64, 64), "db2", 3, "reflect"), ((8, 256, 256), "db4", 4, "symmetric")):
            name = f"waverec2_of_wavedec2_{wavelet}_L{level}_{'x'.join(map(str, shape))}_f32_{mode}"
            try:
                x = torch.randn(*shape, device=dev)
                fn = lambda t: ptwt_amd.waverec2(ptwt_amd.wavedec2(t, wavelet, mode=mode, level=level), wavelet)  # noqa: E731
                cap = ptwt_amd.capture(fn, x)

                def per_call(f, n=200):
                    for _ in range(20):
                        f()
                    sync()
                    t0 = time.perf_counter()
                    for _ in range(n):
                        f()
                    sync()
                    return (time.perf_counter() - t0) / n * 1e3

                out.append({"workload": name, "eager_ms_per_step": round(per_call(lambda: fn(x)), 4),
                            "graph_replay_ms_per_step": round(per_call(cap.replay), 4),
                            "note": "wavedec2 + waverec2 per step; replay = one HIP graph launch of the same kernels (bit-identical)"})
                del cap
            except Exception as exc:
                out.append({"workload": name, "error": repr(exc)[:200]})
    return out


# headline workload -> the workload of the N > 1 "config4_shard" leg (the dry-run workload maps to itself: control flow only)
SCALING_SHARD = {"wavedec2_db4_L3_64x1024x1024_f32": "wavedec2_db8_L4_64x4096x4096_f32",
                 "dryrun_wavedec2_db4_L2_6x96x96_f32": "dryrun_wavedec2_db4_L2_6x96x96_f32"}


def scaling_shard_leg(workload, dev, dist, backend, world, steps=10, warmup=3):
    """Every rank: `steps` whole calls of `workload` on its own shard between barriers, max over ranks; then the all-gather that would
    replicate the coefficients on every rank (one collective per level buffer, ptwt_amd.distributed.gather_coeffs).  Returns the
    dict rank 0 prints under "config4_shard" (every rank must call this: it holds collectives)."""
    import ptwt_amd
    from ptwt_amd import distributed as D

    fn_name, shape, wavelet, level, mode, dtype = WORKLOADS[workload]
    fn = getattr(ptwt_amd, fn_name)
    flen = len(ptwt_amd._wavelets.as_wavelet(wavelet))
    info = {"workload": workload, "api": f"ptwt_amd.{fn_name}(x, '{wavelet}', mode='{mode}', level={level})", "per_gpu_shape": list(shape),
            "global_shape": [shape[0] * world] + list(shape[1:]), "n_gpus": world, "steps": steps, "scaling": "weak"}
    def all_ok(ok):  # (a rank that failed locally must not leave the others waiting at a barrier)
        f = torch.tensor([1 if ok else 0], dtype=torch.int32, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(f, op=dist.ReduceOp.MIN)
        return bool(f.item())

    xs, err = None, None
    try:
        xs = [torch.randn(*shape, dtype=dtype, device=dev) for _ in range(2)]
        for i in range(warmup):
            fn(xs[i & 1], wavelet, mode=mode, level=level)
        sync()
    except Exception as exc:
        err = repr(exc)[:300]
    if not all_ok(err is None):
        info["error"] = err or "another rank failed in the warm-up"
        return info
    try:
        dist.barrier()
        t0 = time.perf_counter()
        for i in range(steps):
            fn(xs[i & 1], wavelet, mode=mode, level=level)
        sync()
        dist.barrier()
        t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ms = float(t.item()) / steps * 1e3
        comp_b = algorithmic_bytes(shape[0], shape[1:], flen, level, torch.empty(0, dtype=dtype).element_size())[0]
        info.update(ms_per_step=round(ms, 4), Msamples_per_s=round(prod(shape) * world / (ms * 1e-3) / 1e6, 1), compulsory_bytes_per_gpu=comp_b,
                    frac_of_hbm_peak_per_gpu=round(comp_b / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4))
        # the gather, outside the transform's timing: one warm-up (communicator set-up), one timed repetition
        coeffs = fn(xs[0], wavelet, mode=mode, level=level)
        del xs
        D.gather_coeffs(coeffs)
        sync()
        dist.barrier()
        tg = time.perf_counter()
        full = D.gather_coeffs(coeffs)
        sync()
        dist.barrier()
        tg = time.perf_counter() - tg
        nbytes = sum(v.numel() * v.element_size() for _, v in _flatten(coeffs))
        info["coefficient_gather"] = {"ms": round(tg * 1e3, 3), "bytes_per_rank": nbytes, "collectives": "one all_gather_into_tensor per level buffer",
                                      "GBps_per_rank_in": round(nbytes * (world - 1) / tg / 1e9, 1)}
        del full
    except Exception as exc:  # (an optional leg never breaks the benchmark line — but it must not hide a hang either: barriers above)
        info["error"] = repr(exc)[:300]
    return info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--spinup-ms", type=float, default=30.0,
                    help="untimed spin-up before the W warm-up steps: the GPU leaves its idle power state only after some "
                         "milliseconds of load (measured: 0.172 ms/step over the first 50 steps vs 0.157 steady)")
    ap.add_argument("--workload", default="wavedec2_db4_L3_64x1024x1024_f32", choices=sorted(WORKLOADS))
    ap.add_argument("--buffers", type=int, default=3, help="distinct input buffers rotated to defeat the 256 MiB Infinity Cache")
    ap.add_argument("--full", action="store_true",
                    help="after the headline steps also run everything else the line can report: roofline and per-kernel legs, rotating-output "
                         "and collector-on loops, secondary workloads, CPU baseline, N > 1 shard leg (a plain run times the steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float32, float64 for f64 workloads; a fixed, seeded "
                         "sample of every array when all of it exceeds 48 MiB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the short list of other workloads timed after the headline "
                                                                "(N = 1) and the shard leg (N > 1)")
    ap.add_argument("--gather", action="store_true",
                    help="N > 1: also time (outside the timed region) the all-gather that would replicate the coefficients on "
                         "every rank; opt-in because it cannot be exercised on the one-GPU development boxes")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1
    if args.gpus != world and distributed:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if args.gpus > 1 and not distributed:
        raise SystemExit("for --gpus > 1 launch with: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...")

    import __graft_entry__ as entry

    if rank == 0:
        entry.build(verbose=False)
    # MIFWT_BENCH_BACKEND=gloo + MIFWT_BENCH_SAME_DEVICE=1: dry run of the N > 1 control flow on a one-GPU box
    # (all ranks on cuda:0, collectives over gloo on host tensors); the real runs use RCCL, one GPU per rank.
    backend = os.environ.get("MIFWT_BENCH_BACKEND", "nccl")
    dev_index = 0 if os.environ.get("MIFWT_BENCH_SAME_DEVICE") == "1" else local_rank
    if DEVICE_KIND == "cuda":
        torch.cuda.set_device(dev_index)
        dev = torch.device("cuda", dev_index)
    else:
        dev = torch.device("cpu")
    if distributed:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        dist.barrier()
    if rank != 0:
        entry.build(verbose=False)

    import ptwt_amd
    from ptwt_amd import _engine

    fn_name, shape, wavelet, level, mode, dtype = WORKLOADS[args.workload]
    is_bwd = fn_name.endswith("_bwd")
    fn = getattr(ptwt_amd, fn_name[:-4] if is_bwd else fn_name)
    if dtype == torch.float16:
        ptwt_amd.set_half_storage(True)
    flen = len(ptwt_amd._wavelets.as_wavelet(wavelet))
    torch.manual_seed(1234 + rank)
    def make_input():
        if prod(shape) < (1 << 31):
            return torch.randn(*shape, dtype=torch.float32, device=dev).to(dtype)
        out = torch.empty(*shape, dtype=dtype, device=dev)  # (big batches: no full-size fp32 temporary)
        for i in range(shape[0]):
            out[i] = torch.randn(*shape[1:], dtype=torch.float32, device=dev).to(dtype)
        return out

    is_rec = "rec" in fn_name  # a reconstruction: the inputs are coefficient sets (made by the matching analysis, untimed)
    if is_rec and is_bwd:
        ana = getattr(ptwt_amd, fn_name[:-4].replace("rec", "dec"))
        with torch.no_grad():
            sets = [ana(make_input(), wavelet, mode=mode, level=level) for _ in range(max(1, args.buffers))]
        # every coefficient tensor a dense leaf of its own (the analysis returns views of level buffers)
        bufs = [[t.contiguous().requires_grad_(True) for _, t in _flatten(c)] for c in sets]
        del sets
        gout = torch.randn(*shape, dtype=dtype, device=dev)

        def step(i):
            lv = bufs[i % len(bufs)]
            y = fn((lv[0], *[tuple(lv[1 + 3 * k : 4 + 3 * k]) for k in range((len(lv) - 1) // 3)]), wavelet)
            return torch.autograd.grad(y, lv, gout)
    elif is_rec:
        ana = getattr(ptwt_amd, fn_name.replace("rec", "dec"))
        bufs = [ana(make_input(), wavelet, mode=mode, level=level) for _ in range(max(1, args.buffers))]

        def step(i):
            return fn(bufs[i % len(bufs)], wavelet)
    elif is_bwd:
        # forward + backward w.r.t. the data: the coefficients' gradients (one fixed set, resident) in, the input's gradient out
        bufs = [make_input().requires_grad_(True) for _ in range(max(1, args.buffers))]
        with torch.no_grad():
            gouts = [torch.randn_like(t) for _, t in _flatten(fn(bufs[0], wavelet, mode=mode, level=level))]

        def step(i):
            xb = bufs[i % len(bufs)]
            outs = [t for _, t in _flatten(fn(xb, wavelet, mode=mode, level=level))]
            return torch.autograd.grad(outs, xb, gouts)
    else:
        bufs = [make_input() for _ in range(max(1, args.buffers))]

        def step(i):
            return fn(bufs[i % len(bufs)], wavelet, mode=mode, level=level)

    # spin-up (untimed, reported in the JSON): bring the device out of its idle clocks before the W warm-up steps
    spin_steps = 0
    t_spin = time.perf_counter()
    while (time.perf_counter() - t_spin) * 1e3 < args.spinup_ms:
        step(spin_steps)
        spin_steps += 1
        if spin_steps % 16 == 0:
            sync()
    # (as timeit does, the interpreter's cyclic collector is kept out of the timed steps: a full pass with torch loaded is a 35-40 ms
    # pause, and it lands in a 100-step window every few thousand calls whatever the calls do.  Not preceded by gc.collect(): the 200
    # steps after a collection ran 10 % slower in every trial — 0.1165 against 0.1036-0.1044 ms per step on config 2, same box,
    # alternating; MIFWT_BENCH_GC=1 leaves the collector on, =3 collects first)
    if os.environ.get("MIFWT_BENCH_GC") == "3":
        gc.collect()
    if os.environ.get("MIFWT_BENCH_GC") != "1":
        gc.disable()
    for i in range(args.warmup):
        step(i)
    sync()
    if distributed:
        dist.barrier()
    sync()

    t0 = time.perf_counter()
    for i in range(args.steps - 1):
        step(i)
    last = step(args.steps - 1)  # (only the last result is kept: every other step's output block is freed as before)
    sync()
    if distributed:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0

    gc.enable()
    if args.dump_outputs and rank == 0:
        dump_outputs(last, args.dump_outputs)
    del last

    if args.full:
        # Roofline leg: the same K steps once more with a HIP event pair around every level launch, recorded on
        # the launch stream.  It is a separate pass because hipEventRecord inserts a barrier packet into the
        # queue: inside the headline region it cost 35 % of the throughput (0.238 vs 0.176 ms/step measured).
        _engine.level_events = []
        for i in range(args.steps):
            step(i)
        sync()
        events, _engine.level_events = _engine.level_events, None

        # Dominant-kernel leg: the first launch of a call (the multi-level kernel where it serves the call), 10 batches of 20
        # launches back to back on the launch stream, one HIP event pair per batch (an event pair around every launch adds a
        # barrier packet on each side of the kernel: +5-8 % on a 100 us kernel).  The count does not depend on --steps; the
        # median batch is the figure, comparable with the rocprofv3 kernel-trace average under profiles/.
        lvl1_b2b_ms = lvl1_b2b_min = None
        lbufs = bufs  # inputs of the dominant-launch leg
        fused_levels = 1
        first_kid = events[0][1] if events else -1
        launch = None
        call_is_launch = False
        if is_rec and not is_bwd and events and len({e[2] for e in events}) == 1:
            # the whole reconstruction is ONE launch (the streaming / small-plane multi-level kernels): the call is the launch
            first_kid = events[-1][1]
            fused_levels = level
            launch = lambda b: fn(b, wavelet)  # noqa: E731
            call_is_launch = True
        elif fn_name in ("wavedec2", "fswavedec2", "wavedec3", "wavedec", "wavedec2_bwd"):
            taps = ptwt_amd._wavelets.host_taps(wavelet)
            if is_bwd:
                lbufs = [b.detach() for b in bufs]  # (the launch leg below calls the engine directly; `step` keeps the leaves)
            mode_id = _engine.MODE_IDS[mode]
            if first_kid in (_engine.KID_PYRAMID, _engine.KID_SMALL):
                fused_levels = len(_engine.ENGINE.analysis_pyramid(lbufs[0], taps[0], taps[1], mode_id, level))
                launch = lambda b: _engine.ENGINE.analysis_pyramid(b, taps[0], taps[1], mode_id, level)  # noqa: E731
            elif first_kid == _engine.KID_PAIR:
                fused_levels = 2
                launch = lambda b: _engine.ENGINE.analysis_pair(b, taps[0], taps[1], mode_id)  # noqa: E731
            elif first_kid == _engine.KID_LONG:
                fused_levels = len(_engine.ENGINE.analysis_tail(lbufs[0], taps[0], taps[1], mode_id, level))
                launch = lambda b: _engine.ENGINE.analysis_tail(b, taps[0], taps[1], mode_id, level)  # noqa: E731
            else:
                launch = lambda b: _engine.ENGINE.analysis(b, taps[0], taps[1], mode_id)  # noqa: E731
        if launch is not None:
            for i in range(5):
                launch(lbufs[i % len(lbufs)])
            sync()
            batches = []
            for _b in range(10):
                e0, e1 = new_event(), new_event()
                e0.record()
                for i in range(20):
                    launch(lbufs[i % len(lbufs)])
                e1.record()
                sync()
                batches.append(e0.elapsed_time(e1) / 20)
            lvl1_b2b_ms, lvl1_b2b_min = statistics.median(batches), min(batches)

        # The K timed steps drop every result, so the caching allocator hands each step the SAME output block and part of the rewritten
        # output lives in the 256 MiB Infinity Cache.  Second figure, reported next to the headline: the same K steps with the last
        # `--buffers` results kept alive, i.e. rotating output sets as well as rotating inputs (config 2: ~8 % slower).
        # (these two loops run AFTER the roofline legs: the rotating loop leaves three freed output sets in the caching allocator, and the
        # launches that follow would cycle through them — the dominant-kernel leg then measured 0.1076 ms against 0.1048 ms per whole call
        # and failed its own consistency check)
        if os.environ.get("MIFWT_BENCH_GC") != "1":
            gc.disable()
        held = [None] * max(1, args.buffers)
        for i in range(max(len(held), min(args.warmup, 10))):
            held[i % len(held)] = step(i)
        sync()
        t1 = time.perf_counter()
        for i in range(args.steps):
            held[i % len(held)] = step(i)
        sync()
        rotating_ms = (time.perf_counter() - t1) / args.steps * 1e3
        del held
        gc.enable()
        # ... and with the interpreter's cyclic collector left on (how BENCH_r01 / r02 were timed)
        for i in range(3):
            step(i)
        sync()
        t1 = time.perf_counter()
        for i in range(args.steps):
            step(i)
        sync()
        gc_on_ms = (time.perf_counter() - t1) / args.steps * 1e3

    # Optional, outside the timed region (N > 1): what replicating the coefficients on every rank would cost — one
    # all_gather_into_tensor per level buffer over RCCL / xGMI (ptwt_amd.distributed.gather_coeffs).  Reported, never part
    # of `value`: the transform itself needs no collective.
    gather_info = None
    if distributed and backend == "nccl" and args.gather:
        try:
            from ptwt_amd import distributed as D

            coeffs = step(0)
            D.gather_coeffs(coeffs)  # warm-up (communicator set-up)
            sync()
            dist.barrier()
            tg = time.perf_counter()
            reps = 3
            for _ in range(reps):
                full = D.gather_coeffs(coeffs)
            sync()
            dist.barrier()
            tg = (time.perf_counter() - tg) / reps
            nbytes = sum(v.numel() * v.element_size() for _, v in _flatten(coeffs))
            gather_info = {"ms": round(tg * 1e3, 3), "bytes_per_rank": nbytes, "collectives": "one all_gather_into_tensor per level buffer",
                           "GBps_per_rank_in": round(nbytes * (world - 1) / tg / 1e9, 1)}
            del full
        except Exception as exc:  # never let the optional leg break the benchmark line
            gather_info = {"error": repr(exc)[:200]}

    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # N > 1, default workload: ALSO the configuration BASELINE.json quotes the multi-GPU split on — configs[3], wavedec2 db8 level 4 on
    # 512 x 4096^2 over 8 GPUs — as its per-GPU shard of 64 images on every rank (weak scaling as the headline: at N = 8 this IS that
    # configuration), max over ranks, and the RCCL gather of its coefficient lists (north_star: "RCCL over xGMI used only to gather the
    # coefficient lists"), timed on its own.  Reported under "config4_shard", never part of `value`.
    shard_info = None
    if distributed and args.full and not args.no_secondary and args.workload in SCALING_SHARD:
        shard_info = scaling_shard_leg(SCALING_SHARD[args.workload], dev, dist, backend, world)

    if rank == 0:
        samples_per_step = prod(shape) * world
        ms_per_step = elapsed / args.steps * 1e3
        esize = torch.empty(0, dtype=dtype).element_size()
        comp_b, perlvl_b, lvl1_b, pair_b = algorithmic_bytes(shape[0], shape[1:], flen, level, esize)
        if is_bwd:  # the backward reads every coefficient's gradient once and writes the input's gradient once: the same bytes again
            comp_b, perlvl_b = 2 * comp_b, 2 * perlvl_b
        result = {
            "metric": "Msamples/s",
            "value": round(samples_per_step / (elapsed / args.steps) / 1e6, 1),
            "unit": "Msamples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": {torch.float32: "f32", torch.float64: "f64", torch.float16: "f16 storage / f32 arithmetic"}[dtype],
            "data": "synthetic (torch.randn, %d rotating input buffers resident in HBM)" % len(bufs),
            "spinup_steps": spin_steps,
            "gc": "cyclic collector disabled during the warm-up and the K timed steps (as timeit does)",
            "config": {
                "workload": args.workload,
                "api": (f"torch.autograd.grad(ptwt_amd.{fn_name[:-4]}(x, '{wavelet}', mode='{mode}', level={level}), x, grad_outputs)" if is_bwd
                        else f"ptwt_amd.{fn_name}(x, '{wavelet}', mode='{mode}', level={level})"),
                "per_gpu_shape": list(shape),
                "parallelism": f"batch-sharded x{world}, no data-path collective",
            },
            "whole_call": {
                "compulsory_bytes": comp_b,
                "per_level_bytes": perlvl_b,
                "achieved_GBps_compulsory": round(comp_b / (ms_per_step * 1e-3) / 1e9, 1),
                "frac_of_hbm_peak": round(comp_b / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            },
        }
        if args.full:
            # dominant kernel = the level-1 analysis launch (largest signal extent); durations from HIP events
            # recorded on the launch stream inside the timed region
            lvl1 = [s.elapsed_time(e) for (tag, kid, ext, s, e) in events if tag in ("fwd", "inv") and tuple(ext) == tuple(shape[1:])]
            per_level_ms = {}
            for tag, kid, ext, s, e in events:
                per_level_ms.setdefault(("adjoint " if tag.endswith("_adj") else "") + "x".join(map(str, ext)), []).append(s.elapsed_time(e))
            kid1 = next((kid for (tag, kid, ext, s, e) in events if tag in ("fwd", "inv") and tuple(ext) == tuple(shape[1:])), -1)
            if kid1 == _engine.KID_PAIR:
                lvl1_b = pair_b
            if kid1 == _engine.KID_INV_PYRAMID:
                fused_levels = min(3, level)
            if kid1 in (_engine.KID_PYRAMID, _engine.KID_LONG, _engine.KID_SMALL, _engine.KID_INV_PYRAMID, _engine.KID_INV_SMALL):
                # input + the detail bands of the fused levels + the approximation of the last fused one (a reconstruction: the same bytes,
                # read and written the other way round)
                lvl1_b = algorithmic_bytes(shape[0], shape[1:], flen, fused_levels, esize)[0]
            klabel = {1: "dwt2_fwd_stream_kernel (level 1)", 7: "dwt2_fwd_tile_kernel (level 1)", 0: "generic axis kernels (level 1)",
                      3: "streaming axis kernels (level 1)", 5: "composed 3-D level 1: fused 2-D kernel over all depth slices + depth pass (two launches; traffic = both)", 9: "dwt3_fwd_tile_kernel (level 1)", 24: "dwt3_fwd_walk_kernel (level 1)", 25: "idwt3_walk_kernel (finest level)",
                      11: "dwt2_fwd_mfma_walk_kernel (level 1)", 23: "idwt2_mfma_walk_kernel (finest level)",
                      12: ("dwt2_fwd_roll_kernel" if flen >= 8 else "dwt2_fwd_pair_kernel") + " (levels 1+2 in one launch)",
                      16: f"dwt2_fwd_pyr_kernel (levels 1-{fused_levels} in one launch)",
                      17: f"dwt1_long_kernel (levels 1-{fused_levels} in one launch)",
                      20: f"dwt2_fwd_small_kernel (levels 1-{fused_levels} in one launch, a workgroup per image)",
                      22: f"idwt2_pyr_kernel (the {fused_levels} finest synthesis levels in one launch)",
                      21: f"idwt2_small_kernel (all {fused_levels} synthesis levels in one launch, a workgroup per image)",
                      13: "idwt2_pair_kernel (two synthesis levels in one launch)", 8: "idwt2_tile_kernel (finest level)",
                      2: "dwt2_inv_stream_kernel (finest level)", 10: "idwt3_tile_kernel (finest level)", 6: "depth pass + fused 2-D planes (finest level)",
                      18: "idwt1_long_kernel (the finest levels in one launch)", 15: "idwt1_tail_kernel (the coarse levels in one launch)",
                      4: "streaming axis kernels (finest level)"}.get(kid1, f"kernel id {kid1} (level 1)")
            per_launch_event_ms = sum(lvl1) / max(1, len(lvl1))
            avg_ms = lvl1_b2b_ms if lvl1_b2b_ms else per_launch_event_ms
            timing_note = ("median of 10 batches of 20 back-to-back launches of that kernel on the launch stream, one HIP event pair per batch "
                           f"(same rotating inputs; independent of --steps); with an event pair around every launch inside whole calls: {per_launch_event_ms:.4f} ms")
            # (one fixed definition: the median 20-launch batch, also for calls that ARE one launch — round 3 took the better of this and
            # ms_per_step for those, which biased the fraction towards the optimistic figure; both are in the line)
            achieved = lvl1_b / (avg_ms * 1e-3) / 1e9 if avg_ms > 0 else 0.0
            traffic, traffic_src = profiled_traffic(args.workload, klabel)
            # the dominant kernel is one launch of a step: its steady-state duration cannot exceed the step's
            # (two separately timed loops of the same launches differ by 2-3 % from run to run — 0.1060 against 0.1037 ms in one round-4 run —
            # so the flag allows 5 %, recorded in the line as consistency_slack; beyond it `frac` is null and the figure moves to
            # `frac_unchecked`)
            kConsistencySlack = 1.05
            consistent = avg_ms <= ms_per_step * kConsistencySlack
            result["whole_call"].update({
                "level_kernel_ms": {k: round(sum(v) / len(v), 4) for k, v in per_level_ms.items()},
                "rotating_outputs_ms": round(rotating_ms, 4),
                "rotating_outputs_frac_of_hbm_peak": round(comp_b / (rotating_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "rotating_outputs_note": f"the same K steps with the last {max(1, args.buffers)} results kept alive (rotating output sets); ms_per_step drops "
                                         "every result, so each step rewrites one output allocation and part of it stays in the 256 MiB Infinity Cache",
                "gc_enabled_ms": round(gc_on_ms, 4),
            })
            result["roofline"] = {
                "kernel": klabel,
                "bound": "hbm",
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                # (None when the dominant launch, timed in its own loop, came out longer than the whole step by more than the slack: an
                # inconsistent measurement must not read like a good one; the figure is then under frac_unchecked)
                "frac": round(achieved / HBM_PEAK_GBS, 4) if consistent else None,
                "frac_unchecked": round(achieved / HBM_PEAK_GBS, 4),
                "consistent": consistent,
                "consistency_slack": kConsistencySlack,
                "algorithmic_bytes_per_launch": lvl1_b,
                "avg_launch_ms": round(avg_ms, 4),
                "min_launch_ms": round(lvl1_b2b_min, 4) if lvl1_b2b_min else None,
                "timing": timing_note,
                "traffic": traffic,
                "traffic_source": (traffic_src + " (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE per launch of this kernel, not measured in this run)") if traffic_src else None,
            }
        if gather_info is not None:
            result["coefficient_gather"] = gather_info
        if shard_info is not None:
            result["config4_shard"] = shard_info
        if args.full and world == 1 and not args.no_secondary and args.workload == "wavedec2_db4_L3_64x1024x1024_f32" and DEVICE_KIND == "cuda":
            del bufs
            torch.cuda.empty_cache()
            if os.environ.get("MIFWT_BENCH_GC") != "1":
                gc.disable()  # (as in the headline loop: a collector pass inside a 60 ms loop is half its time)
            result["secondary"] = secondary_lines(dev)
            gc.enable()
        if args.full and world == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline(fn_name, shape, wavelet, level, mode, dtype)
        print(json.dumps(result), flush=True)
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
