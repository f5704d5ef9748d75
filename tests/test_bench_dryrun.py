"""CPU-tier dry runs of ``bench.py``'s control flow (no GPU, no measurement): N = 1 directly, N = 2 under
``python -m torch.distributed.run`` with the gloo backend — the way the driver launches the multi-GPU bench, so the first real
8-GPU run cannot die in argument / rendezvous / reduction code.  The transform itself runs on the tests' numpy stand-in."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOAD = "dryrun_wavedec2_db4_L2_6x96x96_f32"


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out  # rank 0 prints ONE line
    return json.loads(lines[0])


def _env():
    env = dict(os.environ)
    env.update(MIFWT_BENCH_BACKEND="gloo", MIFWT_BENCH_DEVICE="cpu", PYTHONPATH=ROOT, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def _check(res, n):
    assert res["n_gpus"] == n and res["steps"] == 2 and res["warmup"] == 1
    assert res["unit"] == "Msamples/s" and res["higher_is_better"] is True and res["scaling"] == "weak"
    assert res["config"]["workload"] == WORKLOAD and res["config"]["parallelism"].startswith(f"batch-sharded x{n}")
    assert res["value"] > 0 and res["ms_per_step"] > 0
    # whole-job aggregate: N shards of 6 x 96 x 96 samples per step
    assert abs(res["value"] - n * 6 * 96 * 96 / (res["ms_per_step"] * 1e-3) / 1e6) <= 0.02 * res["value"] + 0.1
    assert set(res["roofline"]) >= {"bound", "achieved", "peak", "unit", "frac", "traffic"}


def test_bench_single_process_dry_run():
    cmd = [sys.executable, os.path.join(ROOT, "tests", "_bench_dryrun.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--spinup-ms", "0", "--workload", WORKLOAD, "--no-cpu-baseline", "--full"]
    p = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    _check(_json_line(p.stdout), 1)


def test_bench_two_ranks_gloo_dry_run():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "_bench_dryrun.py"), "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--spinup-ms", "0", "--workload", WORKLOAD, "--full"]
    p = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    res = _json_line(p.stdout)
    _check(res, 2)
    assert "cpu_baseline" not in res  # N = 1 only
    # the N > 1 line also answers BASELINE's scaling question: the per-GPU shard of the multi-GPU configuration on every rank (here: the
    # dry-run stand-in of it) and the gather of its coefficient lists
    sh = res["config4_shard"]
    assert "error" not in sh, sh
    assert sh["n_gpus"] == 2 and sh["scaling"] == "weak" and sh["global_shape"][0] == 2 * sh["per_gpu_shape"][0]
    assert sh["ms_per_step"] > 0 and sh["Msamples_per_s"] > 0
    g = sh["coefficient_gather"]
    assert g["ms"] > 0 and g["bytes_per_rank"] > 0 and "all_gather" in g["collectives"]


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """Without --full the line holds the headline figures only (no roofline, per-kernel, secondary or CPU-baseline legs), --steps is
    the number of timed steps, and --dump-outputs writes what the last step returned — the same arrays from run to run."""
    import numpy as np

    dumps = []
    for run in range(2):
        out = tmp_path / f"run{run}"
        cmd = [sys.executable, os.path.join(ROOT, "tests", "_bench_dryrun.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
               "--spinup-ms", "0", "--workload", WORKLOAD, "--dump-outputs", str(out)]
        p = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        res = _json_line(p.stdout)
        assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0 and res["value"] > 0
        assert res["metric"] == res["unit"] == "Msamples/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
        assert not {"roofline", "secondary", "cpu_baseline", "config4_shard"} & set(res), sorted(res)
        assert "level_kernel_ms" not in res["whole_call"] and "rotating_outputs_ms" not in res["whole_call"]
        dumps.append({f.name: np.load(f) for f in sorted(out.iterdir())})
    # wavedec2 level 2 of 6 x 96 x 96: the approximation and three detail bands per level, as the caller receives them
    assert sorted(dumps[0]) == ["out_0.npy"] + [f"out_{lv}_{k}.npy" for lv in (1, 2) for k in range(3)]
    assert dumps[0]["out_0.npy"].shape == dumps[0]["out_1_0.npy"].shape == (6, 29, 29) and dumps[0]["out_2_0.npy"].shape == (6, 51, 51)
    for name, a in dumps[0].items():
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, dumps[1][name]), name


def test_dump_outputs_samples_large_outputs_at_fixed_positions(tmp_path):
    """Over the byte budget every array is cut to the same fraction, at positions that depend only on the array's place and size:
    a strided view and a dense copy of the same values give the same sample, and so does a second call."""
    import numpy as np
    import torch

    import bench

    g = torch.Generator().manual_seed(3)
    buf = torch.randn(4, 2, 40, 50, generator=g, dtype=torch.float64)
    coeffs = [torch.randn(4, 20, 25, generator=g), (buf[:, 0], buf[:, 1, :, :30])]  # (views of a level buffer, as the engine returns)
    dense = [coeffs[0], tuple(t.contiguous() for t in coeffs[1])]
    full_bytes = (4 * 20 * 25) * 4 + (4 * 40 * 50 + 4 * 40 * 30) * 8
    shapes = bench.dump_outputs(coeffs, str(tmp_path / "a"), budget=full_bytes // 4)
    bench.dump_outputs(dense, str(tmp_path / "b"), budget=full_bytes // 4)
    bench.dump_outputs(coeffs, str(tmp_path / "c"), budget=full_bytes // 4)
    assert shapes == {"out_0": [500], "out_1_0": [2000], "out_1_1": [1200]}
    total = 0
    for name in shapes:
        a = np.load(tmp_path / "a" / (name + ".npy"))
        total += a.nbytes
        assert a.dtype == (np.float32 if name == "out_0" else np.float64)
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy"))) and np.array_equal(a, np.load(tmp_path / "c" / (name + ".npy")))
        src = {"out_0": coeffs[0], "out_1_0": coeffs[1][0], "out_1_1": coeffs[1][1]}[name].numpy()
        assert np.isin(a, src).all()  # (elements of the array itself, nothing computed)
    assert total <= full_bytes // 4
    # under the budget: every array whole, in its own shape
    assert bench.dump_outputs(coeffs, str(tmp_path / "d")) == {"out_0": [4, 20, 25], "out_1_0": [4, 40, 50], "out_1_1": [4, 40, 30]}
    assert np.array_equal(np.load(tmp_path / "d" / "out_1_1.npy"), coeffs[1][1].numpy())


def test_bench_rejects_mismatched_world():
    cmd = [sys.executable, os.path.join(ROOT, "tests", "_bench_dryrun.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
           "--workload", WORKLOAD]
    p = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "torch.distributed.run" in (p.stderr + p.stdout)
