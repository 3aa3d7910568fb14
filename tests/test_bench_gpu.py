"""bench.py end to end on the GPU box: the one-GPU line, and the N = 2 flow (parent starts its own ranks, barriers, MAX over
ranks, weak value + strong leg + comm figures, ONE JSON line from rank 0) with both ranks sharing cuda:0 over gloo
(CS_BENCH_SHARE_GPU=1: the pool has one GPU per box and RCCL cannot put two ranks on one device)."""
import json
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = ["--steps", "5", "--warmup", "2", "--min-seconds", "0.05", "--rows", "65536", "--cpu-budget", "0", "--no-extras"]


def run_raw(args, env_extra=None):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT", "TORCHELASTIC_RUN_ID")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], capture_output=True, text=True, env=env, timeout=900)


def run(args, env_extra=None):
    r = run_raw(args, env_extra)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_one_gpu_line():
    d = run(FAST)
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["strong"] is None and d["comm"] is None
    assert d["value"] == pytest.approx(d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3), rel=1e-3)
    assert d["timing"]["blocks"] >= 1 and d["timing"]["steps_per_block"] == 5
    r = d["roofline"]
    assert r["bound"] == "mfma" and 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic"] is None or r["traffic_source"].startswith("profiles/")
    assert d["heldout"]["mse"] > 0 and d["predict"]["columns_per_s"] > 0 and d["predict"]["rows_per_call"] == 65536
    # round 3: the per-kernel figures add up to the step (never above it), sysfs load beside the clocks, the cooperative
    # chain's time-out counter, and no output whose R2 is negative because a ReLU head died (synthetic_init)
    assert sum(k["ms_per_step"] for k in d["kernels"].values()) <= d["ms_per_step"] * 1.001
    assert 0 < d["kernels_note"]["scaled_by"] <= 1.0
    assert d["coop_timeouts"] == 0 and "gpu_busy_percent" not in d["timing"]      # round 4: the dead sysfs field is gone
    assert "ReLU-head bias" in d["config"]["init"]


def test_one_gpu_line_with_the_cpu_legs():
    """The acceptance leg (engine against the fp32 CPU restatement after the same steps on the same batches) and the
    published-model side figure with its own CPU baseline."""
    d = run(["--steps", "5", "--warmup", "2", "--min-seconds", "0.05", "--rows", "65536", "--cpu-budget", "3", "--no-profile", "--extras", "pub_mlp"])
    a = d["heldout"]["against_cpu_restatement"]
    assert "error" not in a, a
    # round 6: a STATISTIC over six data orders, three sides.  ASSERTED: the engine against the CPU restatement run in the engine's own
    # arithmetic (bf16 operands emulated) - per variable and over all outputs the mean paired difference within 2 % + two standard
    # errors, the engine's scatter within 2.5 x the restatement's.  REPORTED with standard errors: what bf16 costs against float32.
    c = a["check"]
    assert c["sides"] == ["engine_bf16", "cpu_bf16"]
    assert c["passed"] and c["per_variable_passed"] and c["scatter_passed"] and c["all_outputs_passed"], c
    assert c["orders"] >= 6 and a["engine_vs_fp32"]["orders"] >= 3
    assert set(c) >= {"engine_vs_cpu", "cpu_vs_cpu_other_order", "engine_vs_engine_other_order", "allowed", "margin", "all_outputs", "order_to_order_sd"}
    assert set(c["engine_vs_cpu"]["se"]) == set(c["allowed"])
    assert all(c["engine_vs_cpu"]["of_the_order_means"][v] <= c["allowed"][v] for v in c["allowed"])
    assert all(abs(c["allowed"][v] - (0.02 + 2 * c["engine_vs_cpu"]["se"][v])) < 2e-4 for v in c["allowed"])
    assert c["all_outputs"]["rel_diff_of_the_order_means"] <= c["all_outputs"]["allowed"]
    for k in ("bf16_vs_fp32", "engine_vs_fp32"):
        assert a[k]["sides"][1] == "cpu_fp32" and set(a[k]["engine_vs_cpu"]["se"]) == set(c["allowed"]) and "all_outputs" in a[k]
    # the cost of bf16 operands after equal steps stays a few per cent (information in the line; a regression of the arithmetic - e.g.
    # a missing float32 master copy - would show here first): all outputs within 6 %, no variable beyond 12 %
    assert a["engine_vs_fp32"]["all_outputs"]["rel_diff_of_the_order_means"] <= 0.06
    assert max(a["engine_vs_fp32"]["engine_vs_cpu"]["of_the_order_means"].values()) <= 0.12
    assert a["min_R2"]["engine_bf16"] > 0.5 and a["min_R2"]["cpu_fp32"] > 0.5       # both sides learned every variable
    p = d["pub_mlp"]
    assert "error" not in p, p
    assert p["columns_per_s"] > 0 and p["cpu_baseline"]["value"] > 0 and p["cpu_baseline"]["kind"] == "port"
    assert d["cpu_baseline"]["value"] > 0


def test_dump_outputs_of_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: without --min-seconds the timed region is one block of exactly --steps steps, and what its last step
    computed (loss sums, weights and Adam moments in Keras order, float32, at most 64 MB) lands under DIR.  The inputs are seeded:
    a second run with the same arguments computes the same arrays."""
    import numpy as np
    args = ["--steps", "5", "--warmup", "2", "--rows", "65536", "--cpu-budget", "0", "--no-extras", "--no-profile"]
    dumps = []
    for k in range(2):
        out = tmp_path / f"run{k}"
        d = run([*args, "--dump-outputs", str(out)])
        assert d["steps"] == 5 and d["timing"]["blocks"] == 1 and d["timing"]["steps_per_block"] == 5 and d["ms_per_step"] > 0
        files = sorted(out.glob("*.npy"))
        assert sum(f.stat().st_size for f in files) <= 64 << 20
        dumps.append({f.stem: np.load(f) for f in files})
    a, b = dumps
    assert sorted(a) == sorted(b) and len(a) == 1 + 3 * 16
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["loss"].shape == (2,) and (a["loss"] > 0).all()
    assert a["weight_00"].shape == (124, 512) and a["weight_15"].shape == (8,) and (a["adam_v_00"] > 0).any()
    for name in a:
        np.testing.assert_allclose(a[name], b[name], rtol=1e-5, atol=1e-9, err_msg=name)


def test_two_ranks_start_themselves_and_report_weak_strong_and_comm():
    d = run(["--gpus", "2", *FAST, "--no-profile", "--batch", "2048", "--weak-large-batch", "8192", "--time-oneshot"], {"CS_BENCH_SHARE_GPU": "1"})
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2" and d["config"]["global_batch"] == 4096
    assert d["value"] == pytest.approx(4096 / (d["ms_per_step"] * 1e-3), rel=1e-3)          # whole-job columns / max-over-ranks time
    s = d["strong"]
    assert s["scaling"] == "strong" and s["global_batch"] == 8192 and s["per_gpu_batch"] == 4096 and s["value"] > 0
    # round 3: the strong leg is set beside ONE GPU at the same global batch and says whether it scales
    assert s["one_gpu_same_global_batch"]["value"] > 0 and s["compute_only_ms_per_step"] > 0
    assert s["predicted_ms_per_step"] >= s["compute_only_ms_per_step"]
    assert s["scales"] == (s["value"] > s["one_gpu_same_global_batch"]["value"]) and isinstance(s["verdict"], str)
    assert s["speedup_vs_one_gpu"] == pytest.approx(s["value"] / s["one_gpu_same_global_batch"]["value"], rel=1e-2)
    w = d["weak_large"]
    assert w["scaling"] == "weak" and w["per_gpu_batch"] == 8192 and w["global_batch"] == 16384 and w["value"] > 0
    c = d["comm"]
    assert c["nranks"] == 2 and c["bytes"] == 4787200 and c["allreduce_us_per_step"] > 0
    # the one-shot all-reduce over peer-mapped buffers is timed beside the collective in use (two processes on one device here)
    assert c["oneshot_ipc_error"] is None and c["allreduce_us_oneshot_ipc"] > 0


def test_one_gpu_line_carries_the_batch_sweep():
    """Round 4: SURVEY 8(d) config (2) names B in {1024, 8192, 65536}; the other two sizes ride in the driver's line (`sweep`),
    measured after the headline's timed region on models of their own."""
    d = run(["--steps", "5", "--warmup", "2", "--min-seconds", "0.05", "--rows", "65536", "--cpu-budget", "0", "--no-profile", "--extras", "sweep"])
    sw = d["sweep"]
    assert set(sw) == {"1024", "65536"}
    for b, p in sw.items():
        assert "error" not in p, p
        assert p["per_gpu_batch"] == int(b) and p["blocks"] == 10 and p["steps_per_block"] == 5
        assert p["value"] == pytest.approx(int(b) / (p["ms_per_step"] * 1e-3), rel=1e-3)
        assert 0 < p["whole_step_frac"] < 1 and 0 < p["dominant_frac"] < 1 and p["dominant_kernel"].startswith("k_")
        assert p["dominant_us"] <= p["ms_per_step"] * 1e3 * 1.001 and p["coop_timeouts"] == 0
    assert sw["1024"]["cooperative_chain"] is True and sw["65536"]["cooperative_chain"] is False
    assert sw["65536"]["value"] > sw["1024"]["value"]


N2 = ["--gpus", "2", *FAST, "--no-profile", "--batch", "2048", "--weak-large-batch", "0"]


def test_two_ranks_strong_leg_runs_plain_first_then_on_a_cooperative_model():
    """Round 4 (first contact with N > 1): the strong leg runs WITHOUT the cooperative chain first and on a second model with it
    after that (here, two ranks on one device, that model stays plain - the flow is what is tested), both reported."""
    d = run([*N2, "--strong-global-batch", "4096"], {"CS_BENCH_SHARE_GPU": "1"})
    s = d["strong"]
    assert s["per_gpu_batch"] == 2048 and s["cooperative_chain"] is False and s["value"] > 0
    c = s["with_cooperative_chain"]
    assert "error" not in c, c
    assert c["per_gpu_batch"] == 2048 and c["value"] > 0 and c["one_gpu_same_global_batch"]["value"] > 0
    assert "rccl_comm_matches_nranks" in d["comm"]          # None here (gloo on one device); a boolean with the engine's RCCL communicator


def test_two_ranks_a_failed_health_check_in_the_strong_leg_stays_inside_the_leg():
    """A rank whose check fails between two blocks of the cooperative strong leg (what a timed-out cooperative launch looks like):
    every rank leaves the leg together, the leg reports the error, the line and its weak value survive, exit code 0."""
    d = run([*N2, "--strong-global-batch", "4096"], {"CS_BENCH_SHARE_GPU": "1", "CS_BENCH_INJECT_FAIL": "1:strong_coop_check"})
    assert d["value"] > 0 and d["strong"]["value"] > 0
    assert "rank 1 failed its health check" in d["strong"]["with_cooperative_chain"]["error"]      # rank 0's view; rank 1 saw the exception itself


def test_two_ranks_a_rank_that_dies_ends_in_one_error_line_from_rank_zero():
    """A rank that fails before the JSON line (here: rank 1 at start-up, while rank 0 waits in the rendezvous): rank 0 prints ONE
    line with "error" - from its watcher thread, it is blocked itself - and the command exits non-zero."""
    r = run_raw(N2, {"CS_BENCH_SHARE_GPU": "1", "CS_BENCH_INJECT_FAIL": "1:start"})
    assert r.returncode != 0
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads(lines[-1])
    assert d["value"] is None and d["n_gpus"] == 2 and d["error"]
    assert "injected failure on rank 1" in d["failed_ranks"]["1"]
