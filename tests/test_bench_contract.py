"""bench.py's contract with the driver: one JSON line on stdout with the agreed keys; no GPU, no number."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("this container has a GPU")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1"], capture_output=True, text=True,
                         timeout=300, cwd=ROOT)
    assert res.returncode != 0 and res.stdout.strip() == "" and "needs a GPU" in res.stderr


@pytest.mark.gpu
def test_bench_prints_exactly_one_json_line_with_the_contract_keys(gpu):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--size", "64", "--steps", "4", "--warmup", "2", "--cpu-seconds", "1",
                          "--cpu-size", "32", "--preheat-ms", "5"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, res.stdout[:500]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["unit"] == "MLUPS" and d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "64^3" in d["config"]["workload"] and "model" not in d["config"] and d["config"]["state_finite"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic"] is None and "64" in r["traffic_source"] or r["traffic"] is None      # traffic.json is for 256^3 only
    assert abs(r["achieved"] - 216 * 64 ** 3 / (r["kernel_ms"] * 1e-3) / 1e9) / r["achieved"] < 1e-2
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["unit"] == "MLUPS" and c["cores"] >= 1 and c["value"] > 0 and "32^3" in c["sample"]
    assert abs(d["value"] - 64 ** 3 * 4 / (d["ms_per_step"] * 4 * 1e-3) / 1e6) / d["value"] < 1e-2


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_sample_is_fixed_and_within_budget():
    """--dump-outputs: the sampled blocks depend on the arguments only, stay inside the owned blocks, and the files fit in 64 MB"""
    import numpy as np
    bench = _bench_module()
    a, b = bench.dump_sample(32 ** 3, 0, 1), bench.dump_sample(32 ** 3, 0, 1)
    assert np.array_equal(a, b) and a.size == bench.DUMP_BLOCKS and np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 32 ** 3
    assert np.array_equal(bench.dump_sample(100, 0, 1), np.arange(100))
    per_rank = [bench.dump_sample(64 ** 3, r, 8) for r in range(8)]
    assert sum(s.size for s in per_rank) <= bench.DUMP_BLOCKS and not np.array_equal(per_rank[0], per_rank[1])
    assert bench.DUMP_BLOCKS * (8 ** 3 * (27 + 3 + 1) * 4 + 8) <= 64e6


def test_bench_rejects_zero_steps():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert res.returncode != 0 and res.stdout.strip() == "" and "--steps" in res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [3, 4])
def test_bench_dumps_the_state_of_its_last_timed_step(gpu, tmp_path, steps):
    """--dump-outputs after --warmup 2 --steps K: the sampled blocks' f, vel, rho are those of the CPU oracle after exactly 2 + K steps
    of the same box, bit for bit (odd and even K: both output buffers). 72^3 = 729 blocks, more than DUMP_BLOCKS: the sample is drawn."""
    import numpy as np
    from open_ludwig_amd import cases
    from oracle import oracle
    out = tmp_path / "dump"
    res = _run_bench("--size", "72", "--steps", str(steps), "--warmup", "2", "--cpu-seconds", "0", "--eager-rho-steps", "0",
                     "--preheat-ms", "5", "--dump-outputs", str(out))
    assert res.returncode == 0, res.stderr[-2000:]
    assert json.loads(res.stdout.strip())["steps"] == steps
    files = sorted(os.listdir(out))
    assert files == ["block.npy", "f.npy", "rho.npy", "vel.npy"]
    assert sum(os.path.getsize(out / f) for f in files) <= 64e6
    d = {f[:-4]: np.load(out / f) for f in files}
    assert d["block"].dtype == np.float64 and all(d[k].dtype == np.float32 for k in ("f", "vel", "rho"))
    blocks = d["block"].astype(np.int64)
    assert blocks.size == 512 and np.all(np.diff(blocks) > 0) and blocks[-1] < 9 ** 3
    grids, params = cases.periodic_box((9, 9, 9))
    oracle.execute_timestep_batch(grids, 1, 2 + steps, np.float32(0.0), params)
    fn, vn = oracle.newest_buffers(0, 2 + steps)
    for name, field in (("f", fn), ("vel", vn), ("rho", "rho")):
        want = getattr(grids[0], field)[:, :, :, blocks]
        assert d[name].shape == want.shape and np.array_equal(d[name], want), f"{name}: bench dump != oracle after {2 + steps} steps"


def _run_bench(*argv, env=None, timeout=600):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=timeout, cwd=ROOT,
                          env=dict(os.environ, **(env or {})))


def test_bench_starts_its_own_ranks_from_a_plain_call():
    """`python3 bench.py --gpus 2` with no WORLD_SIZE in the environment (the form the driver uses for N = 1) starts two ranks as a
    child torch.distributed.run. --plan-only stops after the rendezvous and the halo plan - no GPU needed - and rank 0's ONE JSON line
    carries the backend's own world size; both scaling modes."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    for mode, size, box, brick in (("weak", "32", [32, 32, 64], [4, 4, 4]), ("strong", "64", [64, 64, 64], [8, 8, 4])):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--scaling", mode, "--size", size, "--plan-only"],
                             capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
        assert res.returncode == 0, res.stderr[-2000:]
        lines = [l for l in res.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, res.stdout[:500]
        d = json.loads(lines[0])
        assert d["value"] is None and d["plan_only"] is True and d["n_gpus"] == 2 and d["scaling"] == mode
        assert d["comm"]["backend_world_size"] == 2 and d["comm"]["rank_grid"] == [1, 1, 2] and d["comm"]["blocks_per_rank"] == brick
        assert d["config"]["global_box_cells"] == box and mode.upper() in d["config"]["workload"]
        assert d["comm"]["halo_bytes_per_rank_per_step"][0] == d["comm"]["halo_bytes_per_rank_per_step"][1] > 0


def test_self_launched_ranks_fail_loudly_without_gpus():
    import torch
    if torch.cuda.is_available():
        pytest.skip("this container has a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--size", "32", "--steps", "2", "--warmup", "1"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert res.returncode != 0 and res.stdout.strip() == "" and "needs a GPU" in res.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("mode,size", [("weak", "64"), ("strong", "64")])
def test_self_launched_two_rank_rehearsal_on_one_gpu(gpu, mode, size):
    """The whole N > 1 bench path from a plain `python3 bench.py --gpus 2`: two ranks on this box's one GPU (gloo + host-staged
    messages: RCCL refuses two ranks on a device), ONE JSON line, the backend reports world size 2, the state stays finite."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["LUDWIG_BENCH_FORCE_DEVICE"] = "0"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--scaling", mode, "--size", size, "--steps", "4", "--warmup", "2",
                          "--preheat-ms", "5"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, res.stdout[:500]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == mode and d["comm"]["backend_world_size"] == 2 and d["config"]["state_finite"]
    cells = 2 * 64 ** 3 if mode == "weak" else 64 ** 3
    assert d["config"]["global_cells"] == cells
    assert abs(d["value"] - cells * 4 / (d["ms_per_step"] * 4 * 1e-3) / 1e6) / d["value"] < 1e-2
