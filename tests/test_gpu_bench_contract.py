"""bench.py's output contract (task statement): one JSON line on rank 0 with the agreed keys, the roofline of
the dominant kernel measured live, and the CPU baseline at N = 1.  Runs the real script on the GPU, short."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys(tmp_path):
    dump = tmp_path / "outputs"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--dump-outputs", str(dump)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in j, k
    assert j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1
    assert j["unit"] == "solves/s" and j["higher_is_better"] is True and j["scaling"] == "weak"
    assert j["vs_baseline"] is None and j["dtype"] == "f64" and j["data"] == "synthetic"
    assert "workload" in j["config"] and "model" not in j["config"]
    assert j["value"] > 10000  # the north star's floor for configs[1]
    assert abs(j["value"] - 1024 * 1e3 / j["ms_per_step"]) / j["value"] < 1e-6
    r = j["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["kernel"] in ("k_backward", "k_rollout", "k_backward_rollout", "k_round")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert r["launches"] >= r["timed_launches"] > 0 and r["avg_launch_us"] > 1.0
    c = j["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] == "port" and c["value"] > 0 and c["parity_max_rel_cost_err"] < 1e-9
    # the metric as SURVEY.md section 8(d) words it (host buffers in -> host buffers out), beside `value`, never it
    h = j["host_to_host"]
    assert h["unit"] == "solves/s" and 0 < h["value"] < j["value"] * 1.05 and h["parity_with_device_path"] is True
    assert h["bytes_in"] == 1024 * 100 * 18 * 8 and h["pageable_buffers"]["value"] > 0
    # (medians of interleaved calls, first of the extra legs: pinned buffers are not slower than pageable ones, and the host-buffer
    # call costs more than the device-resident call of the same moment, by less than a millisecond)
    assert h["ms_per_solve"] <= h["pageable_buffers"]["ms_per_solve"] * 1.02
    assert 0.0 < h["over_device_resident_ms"] < 1.0 and h["ms_p90"] >= h["ms_per_solve"]
    # the reference's own call pattern (one problem per call through the binding) and the reference-faithful kernel are on the line
    ss, rf = j["single_solve"], j["reference_faithful"]
    assert ss["populate_debug_on"]["debug_entries"] == 100 and ss["populate_debug_off"]["debug_entries"] == 0
    assert ss["c_abi"]["debug_on_over_off"] < 1.10, ss["c_abi"]          # the device-side debug ring: within 10 % of debug off
    assert abs(ss["final_cost"] - ss["cpu_oracle_one_core"]["final_cost"]) / ss["final_cost"] < 1e-3   # (configs[0] is chaotic: DESIGN.md section 2)
    f1 = rf["symmetric_weights_force_general_1"]
    assert f1["max_rel_cost_diff_vs_oracle"] < 1e-9 and f1["same_status_iters_as_oracle"] == f1["oracle_sample"]
    assert f1["value"] * 2.2 > j["value"]                              # (round 5: 1.9 x behind the default kernels; 2.6 x in round 4)
    assert rf["non_symmetric_Q"]["one_backward_pass_vs_oracle"]["max_gain_diff_over_largest_gain"] < 1e-9
    # the saturated machine: B = 8192 in the same run, per-kernel launch times and roofline fractions
    lb = j["large_batch"]
    assert lb["value"] > j["value"] and lb["status_counts"][2] == 0 and lb["status_counts"][3] == 0
    for k in ("k_backward", "k_rollout"):
        assert lb["kernels"][k]["avg_launch_us"] > 1.0 and 0 < lb["kernels"][k]["fp64_frac"] < 1 and 0 < lb["kernels"][k]["hbm_frac"] < 1
    # --dump-outputs: the last timed step's results, float64, every problem (1024 x 100 knots fits the limit), the same
    # solve the line's status and iteration counts describe
    d = {n: np.load(dump / (n + ".npy")) for n in ("traj", "cost", "status", "iters", "n_bwd", "n_fwd", "rows")}
    assert all(a.dtype == np.float64 for a in d.values())
    assert d["traj"].shape == (1024, 100, 18) and d["cost"].shape == (1024,) and (d["rows"] == np.arange(1024)).all()
    assert np.isfinite(d["traj"]).all() and (d["cost"] > 0).all()
    assert np.bincount(d["status"].astype(np.int64), minlength=4).tolist() == j["status_counts"]
    assert d["iters"].max() == j["iters_max"] and abs(d["iters"].mean() - j["iters_mean"]) < 1e-9
    assert sum(f.stat().st_size for f in dump.iterdir()) <= 64 << 20


def test_dump_outputs_keeps_a_fixed_sample_under_the_limit(tmp_path):  # (no GPU needed: runs in the CPU suite)
    """bench.py --dump-outputs: a batch whose results exceed 64 MB is cut to the same seeded rows every time, float64"""
    spec = importlib.util.spec_from_file_location("bench_for_dump_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    B = 8192
    arrays = dict(traj=np.arange(B * 100 * 18, dtype=np.float64).reshape(B, 100, 18), cost=np.arange(B, dtype=np.float64),
                  status=np.arange(B, dtype=np.int32) % 4)
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(d), arrays)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("traj", "cost", "status", "rows")}
    b = {n: np.load(tmp_path / "b" / (n + ".npy")) for n in ("traj", "cost", "status", "rows")}
    assert all(v.dtype == np.float64 for v in a.values())
    assert all(np.array_equal(a[n], b[n]) for n in a)
    rows = a["rows"].astype(np.int64)
    assert 0 < len(rows) < B and (np.diff(rows) > 0).all()
    assert np.array_equal(a["cost"], rows) and np.array_equal(a["traj"], arrays["traj"][rows]) and np.array_equal(a["status"], rows % 4)
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20


@pytest.mark.gpu
@pytest.mark.parametrize("shards", ["same", "distinct"])
def test_two_rank_code_path_on_one_gpu(shards):
    """bench.py --gpus 2, with the test hook that puts both ranks on GPU 0 over gloo.  'distinct' (the default weak-scaling
    workload: N x 1024 distinct problems per step, rotating assignment) is started with NO launcher -- `python bench.py --gpus 2`
    must be a two-rank run by itself (it starts torch.distributed.run as a child process) -- and carries the `sharded_c_abi`
    object: the same step through qilqr_solve_batch_sharded_device in one process, bit-identical costs.  'same' (the diagnostic
    in which every rank solves the N = 1 line's problems) is started the way the driver starts N > 1 (torch.distributed.run, one
    process per rank).  Both: the gather to rank 0 inside the timed region, max-over-ranks timing, one JSON line from rank 0."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["QILQR_BENCH_ONE_DEVICE_TEST"] = "1"
    if shards == "distinct":
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1"]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--shards", "same"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 4 and j["scaling"] == "weak"
    assert j["cpu_baseline"] is None  # rank 0 at N = 1 only
    assert abs(j["value"] - 2 * 1024 * 1e3 / j["ms_per_step"]) / j["value"] < 1e-6
    if shards == "same":
        assert "problems of the N = 1 line" in j["config"]["shard_assignment"]
        assert j["shard_rounds"][0] == j["shard_rounds"][1]  # the same problems on every rank
    else:  # the default
        assert j["config"]["shard_assignment"].startswith("distinct") and "shard (r + step) mod 2" in j["config"]["shard_assignment"]
        assert j["shard_rounds"][0] != j["shard_rounds"][1]  # shards 0 and 1 of the generator: 33 and 31 rollouts for their slowest problems
    assert len(j["shard_rounds"]) == 2 and min(j["shard_rounds"]) > 10
    assert j["iters_max"] == 32  # the last solve of the run is the same-shard leg's: configs[1]'s slowest problem (BENCH line of N = 1)
    ss = j["same_shard"]
    assert ss["value"] > 0 and ss["one_rank_alone_value"] > 0 and 0 < ss["machine_efficiency"] < 1.5
    assert j["status_counts"][2] == 0 and j["status_counts"][3] == 0  # every problem of the last shard converged
    assert j["gather_ms"] > 0 and j["host_to_host"] is None and j["large_batch"] is None
    sa = j["sharded_c_abi"]
    assert "error" not in sa, sa
    assert sa["devices"] == [0, 0] and sa["batch_total"] == 2048 and sa["value"] > 10000 and sa["exposed_gather_ms"] >= 0.0
    assert sa["status_counts"][2] == 0 and sa["status_counts"][3] == 0
    if shards == "distinct":  # the same 2048 problems, shard by shard in the same kernel regime: the same bits
        assert sa["same_costs_as_rank_per_gpu_gather"] is True, sa


def test_a_rank_environment_that_contradicts_gpus_is_refused():  # (no GPU needed: runs in the CPU suite)
    """WORLD_SIZE from a launcher and --gpus disagree: bench.py exits non-zero before it touches anything (VERDICT r04 missing #1:
    `--gpus 8` under no launcher used to print an n_gpus: 1 line with rc 0)"""
    env = dict(os.environ, WORLD_SIZE="3", RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, timeout=60, cwd=ROOT, env=env)
    assert out.returncode == 2 and "WORLD_SIZE" in out.stderr and out.stdout.strip() == ""


def test_preflight_refuses_more_ranks_than_devices_and_launcher_sets_gpus():  # (no GPU needed: runs in the CPU suite)
    """`python bench.py --gpus N` asks a throw-away child process how many devices there are BEFORE it starts N ranks,
    and says so in a sentence with exit code 2 when there are fewer (this container has none; the parent never touches the GPU).  ADVICE r05:
    under a launcher `--gpus` defaults to the launcher's WORLD_SIZE."""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    import torch
    if torch.cuda.device_count() < 2:
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "QILQR_BENCH_ONE_DEVICE_TEST")}
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
        assert out.returncode == 2 and "nothing was started" in out.stderr and "--gpus 2" in out.stderr and out.stdout.strip() == "", out.stderr[-500:]
    old = {k: os.environ.get(k) for k in ("RANK", "WORLD_SIZE")}
    try:
        os.environ["WORLD_SIZE"], os.environ["RANK"] = "3", "1"
        a = types.SimpleNamespace(gpus=None)
        assert bench.launch_ranks_if_needed(a) is None and a.gpus == 3
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.gpu
def test_config3_strong_scaling_code_path_on_one_gpu():
    """bench.py --config 3 (BASELINE.json configs[3]: ONE batch cut into contiguous shards, strong scaling) with two
    ranks on GPU 0 over gloo, at a reduced total batch: the value counts the whole batch once per step, the gather
    is timed on its own too."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, QILQR_BENCH_ONE_DEVICE_TEST="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
                          "--gpus", "2", "--steps", "2", "--warmup", "1", "--config", "3", "--batch", "2050"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["scaling"] == "strong"
    assert j["config"]["batch_total"] == 2050 and j["config"]["batch_per_gpu"] == 1025
    assert abs(j["value"] - 2050 * 1e3 / j["ms_per_step"]) / j["value"] < 1e-6
    assert "configs[3]" in j["config"]["workload"] and j["gather_ms"] > 0
    assert j["status_counts"][2] == 0 and j["status_counts"][3] == 0


@pytest.mark.gpu
def test_real_nccl_backend_at_world_size_one():
    """The N > 1 line of bench.py runs over torch's RCCL (backend "nccl"), which no test could execute on a one-GPU box
    (the two-rank tests above swap in gloo).  --rehearse-nccl runs the N = 1 workload with init_process_group("nccl") at world
    size 1, launched the way the driver launches N > 1 (torch.distributed.run, before anything touches the GPU): communicator
    creation by the first-call all-reduce, every step's results through gather_to_root's batched ncclSend / ncclRecv pair
    addressed to rank 0 itself, barriers, HSA_ENABLE_IPC_MODE_LEGACY=0, and torch's HIP runtime beside the solver library's in
    one process.  bench.py itself asserts that the rows that came back are the rows the solver wrote."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                          "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
                          "--gpus", "1", "--steps", "3", "--warmup", "1", "--rehearse-nccl", "--no-serving", "--no-large-batch",
                          "--no-host-to-host", "--no-single-solve", "--no-reference-faithful", "--no-cpu-baseline"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["n_gpus"] == 1 and j["rehearse_nccl"]["backend"] == "nccl" and j["value"] > 10000
