"""bench.py prints one JSON line with the fields the driver reads (a small ensemble, a few windows)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_has_the_contract_fields(gpu):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--chains", "4096",
                        "--no-cpu-baseline", "--no-ess", "--no-extras"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):   # cpu_baseline: skipped here (12 s of host work)
        assert key in out, key
    assert out["unit"] == "chain-steps/s" and out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1
    assert out["higher_is_better"] is True and out["scaling"] == "weak" and out["vs_baseline"] is None
    assert out["dtype"] == "f64" and out["data"] == "synthetic" and "workload" in out["config"]
    roof = out["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "fp64_issue_frac", "measured_hbm_GBps"):
        assert key in roof, key
    assert roof["bound"] == "hbm" and roof["peak"] == 8000.0 and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-12
    # value = chain-steps of the timed windows / wall time
    assert abs(out["value"] - 4096 * out["config"]["window"] * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]


@pytest.mark.gpu
def test_bench_config_5_line(gpu):
    """`bench.py --config c5`: the sharded TSimpleHMC config through distributed.run_windows over HmcBackend, one rank."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c5", "--steps", "2", "--warmup", "1",
                        "--chains", "1024", "--dim", "80", "--window", "4"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["unit"] == "trajectories/s" and out["config"]["baseline_config"] == 5 and out["n_gpus"] == 1
    assert out["covariance_updates"] >= 1 and 0.0 < out["accept_rate"] <= 1.0
    assert abs(out["value"] - 1024 * 4 * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    assert out["roofline"]["bound"] == "mfma" and out["roofline"]["frac"] > 0.0


def _bench_line(args, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_same_outputs_twice(gpu, tmp_path):
    """A plain run (no --full) times the headline only; --dump-outputs writes the caller's arrays after the last timed
    window, and two runs with the same arguments write the same bits."""
    import numpy as np
    args = ["--steps", "2", "--warmup", "1", "--chains", "4096"]
    dumps = []
    for k in range(2):
        out = _bench_line(args + ["--dump-outputs", str(tmp_path / ("out%d" % k))], tmp_path)
        assert out["steps"] == 2 and out["ms_per_step"] > 0.0 and out["unit"] == "chain-steps/s" and out["dtype"] == "f64"
        assert "extra" not in out and "cpu_baseline" not in out and out["ess_per_chain_step"] is None
        dumps.append({f[:-4]: np.load(tmp_path / ("out%d" % k) / f) for f in os.listdir(tmp_path / ("out%d" % k))})
    a, b = dumps
    assert sorted(a) == ["accepted", "accepted_loglikelihood", "covariance", "decomposition", "naccept", "sigma"]
    assert a["accepted"].shape == (50, 4096) and a["accepted_loglikelihood"].shape == (4096,)
    assert a["covariance"].shape == (50, 50) and a["decomposition"].shape == (50, 50)
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in a.values())
    assert 0 < a["naccept"].sum() <= 4096 * 3 * 256
    assert sorted(b) == sorted(a) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
def test_full_bench_run_keeps_the_ess(gpu, tmp_path):
    """The ESS trace (like the extras and the CPU baseline) runs only under --full."""
    out = _bench_line(["--steps", "2", "--warmup", "1", "--chains", "4096", "--full", "--no-extras", "--no-cpu-baseline"],
                      tmp_path)
    assert out["ess_per_chain_step"] is not None and out["ess_per_chain_step"] > 0.0
    assert abs(out["ess_per_s"] - out["ess_per_chain_step"] * out["value"]) < 1e-9 * out["ess_per_s"]
    assert "extra" not in out and "cpu_baseline" not in out


def test_dump_outputs_keeps_a_fixed_sample_under_the_limit(tmp_path):
    """--dump-outputs: over the size limit, the per-chain arrays keep the same seeded sample of chains every time."""
    import numpy as np
    import bench
    x = np.arange(7 * 1000, dtype=np.float64).reshape(7, 1000)
    names = bench.dump_outputs(str(tmp_path / "all"), {"x": x, "n": np.arange(1000, dtype=np.int32)}, {"c": np.eye(3)}, 1000)
    assert names == ["c", "n", "x"] and np.array_equal(np.load(tmp_path / "all" / "x.npy"), x)
    assert np.load(tmp_path / "all" / "n.npy").dtype == np.float64
    for d in ("s0", "s1"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "n": np.arange(1000, dtype=np.int32)}, {"c": np.eye(3)}, 1000,
                           limit=40000)
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 40000
    idx = np.load(tmp_path / "s0" / "chain_index.npy")
    assert 0 < len(idx) < 1000 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "s1" / "chain_index.npy"))
    assert np.array_equal(np.load(tmp_path / "s0" / "x.npy"), x[:, idx.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "s0" / "n.npy"), idx)


# ---- `python bench.py --gpus N` launches its own ranks (no GPU needed for the logic) ----
def test_rank_environments(smcmc):
    envs = smcmc.distributed.rank_environments(4, 29511, {"PATH": "/bin", "WORLD_SIZE": "9"})
    assert [e["RANK"] for e in envs] == ["0", "1", "2", "3"] == [e["LOCAL_RANK"] for e in envs]
    assert all(e["WORLD_SIZE"] == "4" and e["LOCAL_WORLD_SIZE"] == "4" for e in envs)
    assert all(e["MASTER_ADDR"] == "127.0.0.1" and e["MASTER_PORT"] == "29511" and e["PATH"] == "/bin" for e in envs)
    assert all(e["HSA_ENABLE_IPC_MODE_LEGACY"] == "0" for e in envs)       # dmabuf IPC, or RCCL cannot share buffers
    assert smcmc.distributed.rank_environments(1, 1, {"HSA_ENABLE_IPC_MODE_LEGACY": "1"})[0]["HSA_ENABLE_IPC_MODE_LEGACY"] == "1"
    with pytest.raises(ValueError):
        smcmc.distributed.rank_environments(0, 1)


def test_local_launcher_starts_one_process_per_rank(smcmc, tmp_path):
    """The launcher bench.py uses: N child processes with the ranks' environments, rank 0's stdout handed back, the
    worst exit code reported; fewer devices than ranks is refused before anything starts."""
    script = tmp_path / "rank.py"
    script.write_text("import os, sys\n"
                      "r, w = os.environ['RANK'], os.environ['WORLD_SIZE']\n"
                      "open(os.path.join(sys.argv[1], 'rank' + r), 'w').write(w + ' ' + os.environ['LOCAL_RANK'] + ' ' + os.environ['MASTER_PORT'])\n"
                      "print('line from rank', r)\n"
                      "sys.exit(3 if r == sys.argv[2] else 0)\n")
    code, out = smcmc.distributed.launch_local_ranks([sys.executable, str(script), str(tmp_path), "none"], 3, 8)
    assert code == 0 and out.strip() == "line from rank 0"
    seen = sorted(f for f in os.listdir(tmp_path) if f.startswith("rank") and not f.endswith(".py"))
    assert seen == ["rank0", "rank1", "rank2"]
    ports = {open(tmp_path / f).read().split()[2] for f in seen}
    assert len(ports) == 1 and all(open(tmp_path / f).read().split()[:2] == ["3", f[4:]] for f in seen)
    code, _ = smcmc.distributed.launch_local_ranks([sys.executable, str(script), str(tmp_path), "2"], 3, 8)
    assert code == 3                                                       # a failing rank fails the launch
    with pytest.raises(RuntimeError):
        smcmc.distributed.launch_local_ranks([sys.executable, str(script), str(tmp_path), "none"], 4, 2)


def test_bench_refuses_more_ranks_than_gpus_before_touching_one():
    """`python bench.py --gpus 64` on any box: a clear message and a non-zero exit code, no HIP initialisation."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "64", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0
    assert "64 ranks asked for" in r.stderr and "GPU(s) visible" in r.stderr
    assert "{" not in r.stdout
    # and a WORLD_SIZE that disagrees with --gpus is a usage error, not a silent single-rank run
    env["WORLD_SIZE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
