"""bench.py: the default workload IS the metric's configuration (BASELINE.json: N_clip x N_frame = 2 x 2, 224 px, L_txt = 32), and the
N > 1 plan runs end to end.  The second test needs a GPU: it launches `--gpus 2` with both ranks on GPU 0 and gloo collectives
(the bench's own dry-run switches) -- a control-flow check of the three-graph replay plan, the bucketed exchange, the bf16-direct
optimizer path, the cross-rank parameter check and the sharded inference + row gather; never a measurement."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_workload_is_the_metric_configuration(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert (a.mode, a.gpus, a.videos, a.n_clips, a.frames, a.size, a.txt_len, a.repeat, a.pool) == ("train", 1, 16, 2, 2, 224, 32, 2, "lse")
    assert a.steps > 0 and a.warmup >= 0
    monkeypatch.setattr(sys, "argv", ["bench.py", "--mode", "infer16"])
    b = bench.parse()
    assert (b.n_clips, b.repeat, b.videos) == (16, 64, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--mode", "tgif"])
    c = bench.parse()
    assert (c.head, c.n_clips, c.repeat, c.txt_len) == ("multiple_choice", 2, 5, 25)


def test_full_is_off_by_default_and_dump_outputs_writes_float_arrays(monkeypatch, tmp_path):
    """A plain run measures only the headline figure (`--full` adds the rest); `--dump-outputs DIR` writes the last timed step's loss,
    a fixed seeded sample of the updated parameters and (infer16) the scores as float32 / float64 .npy files."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from types import SimpleNamespace
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", str(tmp_path)])
    a = bench.parse()
    assert a.full and a.dump_outputs == str(tmp_path)
    master = torch.randn(1000)
    bench.dump_outputs(str(tmp_path / "small"), loss=torch.tensor(0.25), bank=SimpleNamespace(master=master), scores=[0.5, 0.125])
    assert np.load(tmp_path / "small" / "loss.npy").tolist() == [0.25]
    assert np.array_equal(np.load(tmp_path / "small" / "params.npy"), master.numpy())
    sc = np.load(tmp_path / "small" / "scores.npy")
    assert sc.dtype == np.float64 and sc.tolist() == [0.5, 0.125]
    monkeypatch.setattr(bench, "DUMP_PARAM_SAMPLE", 64)                     # larger than the sample: the same seeded positions every time
    for d in ("big0", "big1"):
        bench.dump_outputs(str(tmp_path / d), bank=SimpleNamespace(master=master))
    p0, p1 = np.load(tmp_path / "big0" / "params.npy"), np.load(tmp_path / "big1" / "params.npy")
    assert p0.dtype == np.float32 and 0 < p0.size <= 64 and np.array_equal(p0, p1)
    assert np.isin(p0, master.numpy()).all() and not (tmp_path / "big0" / "loss.npy").exists()


def test_supervisor_retries_with_the_next_plan_and_honours_the_done_marker(monkeypatch, tmp_path):
    """bench.py's N > 1 supervisor: a failed attempt is retried with the next, more conservative plan; a hung one is
    killed at the deadline; an attempt that completed its timed region and JSON line (done marker) but died in teardown counts as done."""
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setenv("TMPDIR", str(tmp_path))
    from clipbert_amd.bench import launch as bench_launch                                   # (the supervisor lives in clipbert_amd/bench/launch.py since round 5; bench re-exports it)
    monkeypatch.setattr(bench_launch, "ATTEMPT_TIMEOUT_S", 3.0)
    log = tmp_path / "log.txt"

    def job(script_for_attempt):
        def make(attempt):
            env = dict(os.environ, CB_ATT=str(attempt), CB_LOG=str(log), CB_PLAN=bench.ATTEMPTS[attempt].get("CB_BENCH_PLAN", "captured"))
            return [sys.executable, "-c", script_for_attempt[attempt]], env
        return make
    note = "import os; open(os.environ['CB_LOG'], 'a').write(os.environ['CB_ATT'] + ':' + os.environ['CB_PLAN'] + '\\n');"
    # attempt 0 exits 3, attempt 1 succeeds: two attempts ran, the second under the split plan
    assert bench._run_attempts(job([note + "raise SystemExit(3)", note + "pass", note + "pass"]), 3, 0, "jobA") == 0
    assert log.read_text().split() == ["0:captured", "1:split"]
    # attempt 0 hangs (killed at the deadline), attempt 1 too, attempt 2 succeeds
    log.write_text("")
    hang = note + "import time; time.sleep(60)"
    assert bench._run_attempts(job([hang, hang, note + "pass"]), 3, 0, "jobB") == 0
    assert log.read_text().split() == ["0:captured", "1:split", "2:split"]
    # every attempt fails: the exit code is not 0
    assert bench._run_attempts(job(["raise SystemExit(2)"] * 3), 3, 0, "jobC") != 0
    # done marker written, then a crash in teardown: success, no retry
    log.write_text("")
    marker = bench._marker("jobD", 0, "r5.done")
    crash_after_done = note + f"open({marker!r}, 'w').write('x'); os._exit(11)"
    assert bench._run_attempts(job([crash_after_done, note + "pass"]), 2, 5, "jobD") == 0
    assert log.read_text().split() == ["0:captured"]
    # done marker written, then the teardown HANGS: the attempt counts as done after a grace period, long before the deadline
    log.write_text("")
    marker = bench._marker("jobD2", 0, "r2.done")
    hang_after_done = note + f"open({marker!r}, 'w').write('x'); import time; time.sleep(600)"
    monkeypatch.setattr(bench_launch, "ATTEMPT_TIMEOUT_S", 300.0)
    t_start = __import__("time").perf_counter()
    assert bench._run_attempts(job([hang_after_done, note + "pass"]), 2, 2, "jobD2") == 0
    assert __import__("time").perf_counter() - t_start < 60 and log.read_text().split() == ["0:captured"]
    # another rank's failure marker ends this rank's (hung) attempt early and both move on together
    log.write_text("")
    open(bench._marker("jobE", 0, "failed"), "w").write("x")
    import time
    t0 = time.perf_counter()
    monkeypatch.setattr(bench_launch, "ATTEMPT_TIMEOUT_S", 60.0)
    assert bench._run_attempts(job([hang, note + "pass"]), 2, 1, "jobE") == 0
    assert time.perf_counter() - t0 < 20 and log.read_text().split() == ["0:captured", "1:split"]


def test_supervise_is_a_no_op_for_one_gpu_and_for_workers(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    assert bench.supervise(bench.parse()) is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    monkeypatch.setenv("CB_BENCH_WORKER", "1")
    assert bench.supervise(bench.parse()) is None


@pytest.mark.parametrize("launcher", ["none", "torchrun"])
@pytest.mark.parametrize("stub", ["ok", "fail0:1", "hang0:0"])
def test_supervised_launch_end_to_end_with_stub_workers(launcher, stub, tmp_path):
    """The whole N > 1 launch path of bench.py on CPU, with stub workers in place of the measured ones (bench._stub_worker): no launcher
    (bench starts its own ranks) and under `torch.distributed.run` (every rank process supervises one worker).  Attempt 0 succeeding;
    one rank failing on attempt 0 (the others hang in the collective until the failure marker reaches their supervisors, then ALL ranks
    retry together, rendezvousing through a fresh store on the derived port); one rank hanging until the deadline.  Exactly one JSON
    line comes out, from the attempt that finished."""
    env = dict(os.environ, CB_BENCH_TEST_STUB=stub, TMPDIR=str(tmp_path), CB_BENCH_ATTEMPT_TIMEOUT="12" if stub.startswith("hang") else "120")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "CB_BENCH_WORKER", "CB_BENCH_PLAN", "CB_COMM", "TORCHELASTIC_USE_AGENT_STORE"):
        env.pop(k, None)
    bench_py = os.path.join(ROOT, "bench.py")
    if launcher == "none":
        cmd = [sys.executable, bench_py, "--gpus", "2"]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
               str(_free_port()), bench_py, "--gpus", "2"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = lines[0]
    assert out["stub"] and out["n_gpus"] == 2
    if stub == "ok":
        assert out["attempt"] == 0 and out["plan_env"] == ""
    else:
        assert out["attempt"] in (1, 2) and out["plan_env"] == "split", out      # the next rung of the ladder, on every rank (2: its port was taken)
        assert "retrying with" in r.stderr


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["train", "infer16"])
def test_two_rank_dry_run_on_one_gpu(mode):
    # (gloo moves the 297 MB of a step's gradients through the host: 8-22 s per step on the GPU boxes; CB_BENCH_ATTEMPT_TIMEOUT keeps a
    # retry after a hung attempt inside this test's own limit)
    env = dict(os.environ, CB_BENCH_SHARE_GPU="1", CB_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1", CB_BENCH_ATTEMPT_TIMEOUT="330")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
           str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--mode", mode, "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]                     # rank 0 prints ONE JSON line
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["value"] > 0 and out["scaling"] == "weak"
    assert out["config"]["parallelism"] == "dp2" and out["config"]["n_clips"] == (2 if mode == "train" else 16)
    if mode == "train":
        assert out["config"]["dp_self_check"].startswith("ok"), out["config"]["dp_self_check"]
        assert out["config"]["n_graphs"] in (1, 2, 3, 4) and out["config"]["hip_graph"] is True      # machine fields only: never prose
    else:
        assert out["config"]["rows_gathered"] == 2 * 2 * 64       # 2 ranks x 2 timed steps x 64 captions


@pytest.mark.gpu
def test_bare_gpus_2_launches_its_own_ranks():
    """`python bench.py --gpus 2` with NO launcher starts its own two ranks (here both on GPU 0 with gloo collectives)
    and prints rank 0's single JSON line."""
    env = dict(os.environ, CB_BENCH_SHARE_GPU="1", CB_BENCH_BACKEND="gloo", CB_BENCH_ATTEMPT_TIMEOUT="330")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "CB_BENCH_WORKER"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--full"], env=env, capture_output=True,
                       text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["config"]["dp_self_check"].startswith("ok")
    assert out["config"]["attempt"] in (0, 1) and "exposed_comm" in out["config"]


def _multi_gpu_bench(extra_env, n=2):
    env = dict(os.environ, **extra_env)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "CB_BENCH_WORKER"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "3", "--warmup", "1", "--full"], env=env, capture_output=True,
                       text=True, timeout=1500, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])


def _n_gpus():
    import torch
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


@pytest.mark.gpu
@pytest.mark.parametrize("plan", ["captured", "split", "owner_only", "torch_carrier"])
def test_real_rccl_ranks_when_the_box_has_two_gpus(plan):
    """on a box with >= 2 GPUs the data-parallel plans run over real RCCL ranks -- the library's own carrier
    (cb_allreduce_bucket) captured in one graph, the four-graph plan, the owner-only RS -> AdamW -> AG update, torch.distributed as the
    carrier -- and every one of them ends with bit-identical parameters on all ranks.  Skipped (not failed) on 1-GPU boxes."""
    if _n_gpus() < 2:
        pytest.skip("needs >= 2 GPUs (the build boxes have one)")
    env = {"captured": {"CB_BENCH_PLAN": "captured"}, "split": {"CB_BENCH_PLAN": "split"}, "owner_only": {"CB_BENCH_SHARD": "1", "CB_BENCH_PLAN": "captured"},
           "torch_carrier": {"CB_BENCH_PLAN": "split", "CB_COMM": "torch"}}[plan]
    out = _multi_gpu_bench(env, n=min(_n_gpus(), 8))
    cfg = out["config"]
    assert out["n_gpus"] >= 2 and out["value"] > 0
    assert cfg["dp_self_check"].startswith("ok"), cfg["dp_self_check"]
    assert cfg["grad_exchange"].startswith("torch" if plan == "torch_carrier" else "native"), cfg["grad_exchange"]
    assert cfg["n_graphs"] == (1 if plan in ("captured", "owner_only") else 4)
    if plan == "owner_only":
        assert cfg["update"].startswith("owner-only")
    assert 0.0 < cfg["final_loss"] < 5.0


@pytest.mark.gpu
def test_loopback_plan_captures_the_collectives_of_the_full_step():
    """the library's own RCCL entry point (cb_allreduce_bucket) inside the hipGraph of the FULL training step --
    bench.py's data-parallel plan on one GPU with a world-size-1 communicator (CB_BENCH_LOOPBACK=1): one graph, no eager collective."""
    env = dict(os.environ, CB_BENCH_LOOPBACK="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-roofline"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    cfg = out["config"]
    assert cfg["n_graphs"] == 1 and cfg["hip_graph"] is True and "LOOPBACK" in cfg["parallelism"]
    assert cfg["grad_exchange"].startswith("native")
    assert out["value"] > 0 and 0.0 < cfg["final_loss"] < 5.0


@pytest.mark.gpu
def test_loopback_owner_only_update_is_captured_and_trains():
    """The other half of VERDICT r2 item 7: cb_reduce_scatter_bucket -> AdamW on the owned pieces -> cb_allgather_bucket inside the ONE
    hipGraph of the step (world-size-1 communicator; the 2-rank arithmetic is tests/test_dp_gloo.py::test_dp2_owner_only_update_equals_dp1)."""
    env = dict(os.environ, CB_BENCH_LOOPBACK="1", CB_BENCH_SHARD="1")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--no-roofline"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    cfg = out["config"]
    assert cfg["n_graphs"] == 1 and cfg["update"].startswith("owner-only") and "cb_reduce_scatter_bucket" in cfg["grad_exchange"]
    assert out["value"] > 0 and 0.0 < cfg["final_loss"] < 5.0


@pytest.mark.gpu
def test_plain_run_times_the_given_steps_and_dumps_the_last_step(tmp_path):
    """`bench.py --gpus 1 --steps N --warmup W --dump-outputs DIR`: exactly the headline line (no roofline / CPU baseline without
    `--full`), `steps` and `ms_per_step` of the N timed steps, and the last step's outputs as finite float arrays within 64 MB."""
    import numpy as np
    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert (out["unit"], out["higher_is_better"], out["dtype"]) == ("clips/s", True, "bf16")
    assert "roofline" not in out and "cpu_baseline" not in out
    files = sorted(p.name for p in out_dir.iterdir())
    assert files == ["loss.npy", "params.npy"], files
    assert sum(p.stat().st_size for p in out_dir.iterdir()) <= 64 << 20
    for name in files:
        arr = np.load(out_dir / name)
        assert arr.dtype in (np.float32, np.float64) and arr.size > 0 and np.isfinite(arr).all(), name
