#!/usr/bin/env python3
"""bench.py - training columns/sec of the low-res MLP (BASELINE.json metric) on N MI355X.

A "step" is one optimiser step of the cfg-MLP (124 -> 5x512 -> 128 -> [120 || 8], LeakyReLU 0.15,
Adam eps=1e-7, bf16 MFMA with fp32 accumulate / fp32 master weights) on one batch of synthetic
low-res-shaped columns gathered by a random permutation from an HBM-resident split:
gather+normalise-cast -> 7 Dense forward -> fused MSE/dz -> 7 wgrad + 6 dgrad -> (N>1: ONE RCCL
all-reduce of the flat fp32 gradient) -> fused optimiser + bf16 re-cast.  Nothing is skipped.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--batch PER_GPU_BATCH] [--dump-outputs DIR]
  The timed region is exactly K steps after W untimed ones (`--min-seconds S` repeats the K-step block until S seconds are timed);
  `ms_per_step` in the line is what one timed step took.  --dump-outputs writes what the last timed step computed (dump_outputs).
  N>1: one rank per GPU.  Either launched by `python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N`
  (RANK / LOCAL_RANK / WORLD_SIZE in the environment) or plainly as `python bench.py --gpus N`: the parent then touches no
  GPU and starts the N ranks itself as a child process group (torch.distributed.run on 127.0.0.1), passing stdout through.
  `value` is weak scaling (per-GPU batch fixed, global batch = N*batch); the line also carries `strong`: BASELINE
  configs[3], global batch 8192 dealt over the N ranks (1024 per GPU at N = 8).

Prints ONE JSON line on rank 0 (see DESIGN.md section "Measurement").
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

UNITS = (512, 512, 512, 512, 512)
# algorithmic FLOP per column of each kernel kind; chain_* are the fused-layer forms
FLOPS_PER_COL = {"gemm_fwd": 2 * 1_193_984, "gemm_dgrad": 2 * 1_130_496, "wgrad": 2 * 1_193_984,
                 "chain_fwd": 2 * 1_193_984, "chain_bwd": 2 * 1_130_496, "chain_fb": 2 * (1_193_984 + 1_130_496)}
KERNEL_NAMES = {"gemm_fwd": "k_gemm_nt<EPI_HIDDEN|EPI_OUT>", "gemm_dgrad": "k_gemm_nt<EPI_DGRAD>", "wgrad": "k_wgrad",
                "chain_fwd": "k_chain<BM,false>", "chain_bwd": "k_chain<BM,true>", "chain_fb": "k_chain_fb<BM>"}
TRAIN_FLOPS_PER_COL = 7_036_928
HBM_BYTES_PER_COL = 1008                    # 496 B x + 512 B y (fp32 storage), SURVEY 8(d)
PEAK_BF16_TFLOPS = 2500.0                   # dense MFMA peak, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0


PMC_FILES = ("r06_pmc_hbm_traffic.json", "r05_pmc_hbm_traffic.json", "r04_pmc_hbm_traffic.json", "r03_pmc_hbm_traffic.json", "r02_pmc_hbm_traffic.json", "r01_pmc_hbm_traffic.json")     # newest first


def pmc_traffic(kernel, batch):
    """(HBM bytes per launch of `kernel`, source file) from the committed PMC passes (profiles/rNN_pmc_hbm_traffic.json:
    separate `rocprofv3 --pmc FETCH_SIZE` / `WRITE_SIZE` runs of `bench.py --train-only`, gfx950 x2 read correction;
    tools/gpu_diag.sh + tools/pmc_traffic_json.py) - counters cannot be read from inside the timed process, so the figure
    is NOT measured in this run and carries its source.  (None, None) when no pass matches this batch."""
    for name in PMC_FILES:
        try:
            with open(os.path.join(REPO, "profiles", name)) as f:
                return json.load(f)[str(batch)][kernel]["traffic_bytes"], "profiles/" + name
        except (OSError, KeyError, ValueError):
            continue
    return None, None


class ClockSampler:
    """Shader clock (MHz) of the GPU while the timed region runs, read from sysfs (hwmon freq1_input, else the starred level of
    pp_dpm_sclk) by a host thread every 20 ms - nothing is launched on the GPU.  None where sysfs is not readable.
    (Round 3 also sampled `gpu_busy_percent`: it read 0.0 in all 51 samples of the driver's run - the counter is a slow average
    that a 1 s timed region never moves - and was dropped.)"""

    def __init__(self, index=0):
        import glob
        self.path = None
        cards = sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk"))
        # The box's sysfs lists every GPU of the host, the process sees only its own: pick the card by PCI address (card<index>
        # read a neighbour's clock on round 4's boxes - 96-158 MHz beside a busy GPU), fall back to the index.
        want = None
        try:
            import torch
            pr = torch.cuda.get_device_properties(index)
            want = "%04x:%02x:%02x." % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id)
        except Exception:
            pass
        pick = [c for c in cards if want and os.path.basename(os.path.realpath(os.path.dirname(c))).startswith(want)]
        self.matched_by = "pci address" if pick else "card index"
        if not pick and index < len(cards):
            pick = [cards[index]]
        if pick:
            self.path = pick[0]
            hw = sorted(glob.glob(os.path.join(os.path.dirname(pick[0]), "hwmon", "hwmon*", "freq1_input")))
            if hw:
                self.path = hw[0]                # current shader clock in Hz (pp_dpm_sclk's starred level is 94 MHz on some boxes of the pool)
        self.samples, self._stop, self._thr = [], False, None

    def read(self):
        try:
            if self.path.endswith("freq1_input"):
                return float(open(self.path).read()) / 1e6
            for line in open(self.path):
                if "*" in line:
                    return float(line.split(":")[1].strip().split("M")[0])
        except Exception:
            return None
        return None

    def __enter__(self):
        import threading
        if self.path:
            def loop():
                while not self._stop:
                    v = self.read()
                    if v is not None:
                        self.samples.append(v)
                    time.sleep(0.02)
            self._thr = threading.Thread(target=loop, daemon=True)
            self._thr.start()
        return self

    def __exit__(self, *exc):
        self._stop = True
        if self._thr:
            self._thr.join(timeout=1.0)

    def summary(self):
        if not self.samples:
            return None
        s = sorted(self.samples)
        return {"min": s[0], "median": s[len(s) // 2], "max": s[-1], "samples": len(s), "source": self.path, "card_matched_by": self.matched_by}


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as children through torch.distributed.run (this
    process makes no GPU call and is never replaced by exec) and return their exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__), *argv]
    return subprocess.run(cmd, env=env).returncode


def synth_on_device(torch, n, seed, device, signal=(1.0, 0.05)):
    """Low-res-shaped synthetic columns (SURVEY.md 8d recipe), generated on the GPU.  `signal` = (gain inside the tanh, target
    amplitude): (1, 0.05) is the recipe (signal std 0.0075 under noise 0.01: R2 <= ~0.36 attainable); the acceptance leg uses
    (3, 0.3) as tests/test_mlp_gpu.py does, so that a few hundred steps reach R2 ~ 0.9 and a comparison of R2 means something."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    x = torch.empty((n, 124), dtype=torch.float32, device=device)
    x[:, :120] = (torch.randn((n, 120), generator=g, device=device) * 0.15).clamp_(-1, 1)
    x[:, 120:] = torch.rand((n, 4), generator=g, device=device) - 0.5
    night = torch.rand(n, generator=g, device=device) < 0.5
    x[night, 121] = 0
    ga = torch.Generator(device=device)
    ga.manual_seed(20230614)
    a = torch.randn((124, 128), generator=ga, device=device) / (124 ** 0.5)
    y = torch.tanh(signal[0] * (x @ a)) * signal[1] + torch.randn((n, 128), generator=g, device=device) * 0.01
    y[:, 120:] = y[:, 120:].clamp_(min=0)
    y[:, 60:72] = 0
    return x.contiguous(), y.contiguous()


def side_bench(fn):
    try:
        return fn()
    except Exception as e:                       # a side figure must never take the headline line down
        return {"error": f"{type(e).__name__}: {e}"}


RELU_HEAD_BIAS = 0.02       # synthetic recipe only, see synthetic_init


def synthetic_init(seed=0, units=UNITS):
    """Initial weights of the synthetic runs: Keras' Dense defaults (glorot_uniform kernels, zero biases) EXCEPT the bias of the
    8-wide ReLU head, which starts at +0.02 (`bias_initializer=Constant(0.02)`, a legal Keras setting).  Why: the recipe's
    ReLU-head targets are max(z, 0) with mean 0.005 and std 0.007; with a zero bias the first Adam steps at lr 1e-3 push two
    of the eight heads (cam_out_FLWDS, cam_out_SOLLD with seed 0) below zero for every row - dead units in the engine AND in
    the fp32 CPU restatement (measured: alive fraction 0.96 / 0.85 at step 0, 0.00 from step 5 on, at lr 1e-4 too) - which put
    R2 = -0.47 and a constant MAE into rounds 1-2's `heldout`.  With +0.02 all eight stay alive (CPU restatement, 160 steps)."""
    from climsim_amd.mlp import glorot_uniform_weights
    ws = glorot_uniform_weights(124, units, 120, 8, seed)
    ws[-1][:] = RELU_HEAD_BIAS
    return ws


_METRICS = None


def device_metrics():
    """The reference's evaluation pipeline (pressure-thickness, area and energy-unit weighting; data_utils.py:1112-1362,
    1432-1497) on the device (climsim_amd.metrics).  Grid and normalisation constants: the committed low-res bundles under tests/golden/."""
    global _METRICS
    if _METRICS is None:
        from climsim_amd.assets import load_grid_info, load_npz_assets
        from climsim_amd.data_utils import data_utils
        from climsim_amd.metrics import GpuMetrics
        gold = os.path.join(REPO, "tests", "golden")
        grid = load_grid_info(os.path.join(gold, "grid_lowres.npz"))
        sets = [load_npz_assets(os.path.join(gold, "norm_lowres.npz"), k) for k in ("input_mean", "input_max", "input_min", "output_scale")]
        du = data_utils(grid, *sets)
        du.set_to_v1_vars()
        _METRICS = GpuMetrics(du)
    return _METRICS


def per_variable_tables(pred, yv, xv):
    import math
    df_var, _ = device_metrics().metrics_tables(pred, yv, xv)

    def num(x, nd):                                      # strict JSON: no inf/nan (zero-variance levels give R2 = -inf)
        x = float(x)
        return round(x, nd) if math.isfinite(x) else None
    return {"MAE": {v: num(df_var.loc[v, "MAE"], 6) for v in df_var.index}, "R2": {v: num(df_var.loc[v, "R2"], 4) for v in df_var.index}}


def heldout_per_variable(model, xv, yv):
    """Per-variable MAE / R2 of the just-trained model on the held-out split, through the evaluation pipeline of the reference."""
    n = (xv.shape[0] // 384) * 384                       # whole "time steps" of the 384-column grid
    pred = model.predict(xv[:n], as_numpy=False)
    return {"rows": n, **per_variable_tables(pred, yv[:n], xv[:n]),
            "note": "energy-weighted units (W/m2) as in the reference's evaluation; R2 is null where a level has zero target variance"}


def acceptance_check(tables, overall=None, sides=("engine_bf16", "cpu_fp32")):
    """One paired comparison of the acceptance leg, separated from the runs so that it can be driven on made-up tables
    (tests/test_bench_contract_cpu.py).  `tables[side][order]` = {variable: MAE}; order o of both sides saw the same batches in the same
    sequence, so the orders are PAIRS.  Per variable the paired differences d_o = a_o - b_o give delta = mean(d_o) and its standard
    error se = std(d_o, ddof=1) / sqrt(n); held to |delta| <= 2 % (bf16 after equal steps) + 2 se, both relative to
    side b's mean.  Side a's own run-to-run scatter enters through se only TOGETHER with b's (round-5 advisor finding: it must not
    widen its own bar) and is bounded separately: its order-to-order standard deviation may not exceed 2.5 x b's.
    `overall[side][order]` (optional) = MAE over all 128 outputs, held to the same rule (round 6 measured it over six orders: 1.7 -
    2.6 % +- 1.0 - 1.3 % between bf16 operands and float32 - round 5's 0.1 % was one lucky pair, a flat 2 % bar is a coin flip)."""
    import math
    a_, b_ = sides
    names = list(tables[b_][0])
    n = len(tables[b_])
    assert n >= 2 and len(tables[a_]) == n, "the check needs the same >= 2 data orders on both sides"

    def mean(xs):
        return sum(xs) / len(xs)

    def sd(xs):
        m = mean(xs)
        return math.sqrt(sum((x - m) ** 2 for x in xs) / (len(xs) - 1))
    mu = {s_: {v: mean([t[v] for t in tables[s_]]) for v in names} for s_ in sides}
    ref = {v: max(abs(mu[b_][v]), 1e-30) for v in names}
    sig = {s_: {v: sd([t[v] for t in tables[s_]]) / ref[v] for v in names} for s_ in sides}
    d = {v: [e[v] - c[v] for e, c in zip(tables[a_], tables[b_])] for v in names}
    signed = {v: mean(d[v]) / ref[v] for v in names}
    delta = {v: abs(signed[v]) for v in names}
    se = {v: sd(d[v]) / math.sqrt(n) / ref[v] for v in names}
    allowed = {v: 0.02 + 2.0 * se[v] for v in names}
    same_order = {v: max(abs(x) for x in d[v]) / ref[v] for v in names}

    def pair_spread(ts, v):
        return max(abs(ts[i][v] - ts[j][v]) / max(abs(ts[j][v]), 1e-30) for i in range(len(ts)) for j in range(len(ts)) if i != j)
    spread = {s_: {v: pair_spread(tables[s_], v) for v in names} for s_ in sides}
    worst = max(names, key=lambda v: delta[v] - allowed[v])
    # side a may not be more erratic than side b (floor: 0.5 % - two runs that agree to rounding have no scatter to compare)
    scatter_ok = {v: sig[a_][v] <= 2.5 * max(sig[b_][v], 0.005) for v in names}
    r4 = lambda t: {v: round(x, 4) for v, x in t.items()}          # noqa: E731
    out = {"orders": n, "sides": [a_, b_],
           "engine_vs_cpu": {"of_the_order_means": r4(delta), "signed": r4(signed), "se": r4(se), "same_order_worst": r4(same_order)},
           "order_to_order_sd": {a_: r4(sig[a_]), b_: r4(sig[b_])},
           "cpu_vs_cpu_other_order": r4(spread[b_]), "engine_vs_engine_other_order": r4(spread[a_]),
           "allowed": r4(allowed), "tolerance": "per variable and for the all-output MAE: |mean paired difference| <= 0.02 + 2 se, relative to the second side's mean; "
                                                "first side's order-to-order sd <= 2.5 x the second's",
           "worst_variable": worst, "margin": round(allowed[worst] - delta[worst], 4),
           "per_variable_passed": bool(all(delta[v] <= allowed[v] for v in names)),
           "scatter_passed": bool(all(scatter_ok.values()))}
    if overall is not None:
        do = [e - c for e, c in zip(overall[a_], overall[b_])]
        mo = max(abs(mean(overall[b_])), 1e-30)
        se_o = sd(do) / math.sqrt(n) / mo
        out["all_outputs"] = {"rel_diff_of_the_order_means": round(abs(mean(do)) / mo, 5), "signed": round(mean(do) / mo, 5), "se": round(se_o, 5),
                              "allowed": round(0.02 + 2.0 * se_o, 5)}
        out["all_outputs_passed"] = bool(abs(mean(do)) / mo <= 0.02 + 2.0 * se_o)
    out["passed"] = bool(out["per_variable_passed"] and out["scatter_passed"] and out.get("all_outputs_passed", True))
    return out


def acceptance_order(torch, nbat, o):
    """Batch sequence of data order `o` (the same in the engine's process and in the CPU workers)."""
    return list(range(nbat)) if o == 0 else torch.randperm(nbat, generator=torch.Generator().manual_seed(100 + o)).tolist()


def acceptance_cpu_worker(work):
    """`python bench.py --acceptance-cpu-worker DIR`: the CPU sides of the acceptance leg in a process of their own (no GPU call): trains
    the restatement on the batches of DIR - `cpu_bf16` for every data order, `cpu_fp32` for the first `orders_fp32` - and writes the held-out
    predictions."""
    import numpy as np
    import torch
    from oracle.mlp_oracle import MLPConfig
    from oracle.mlp_torch_cpu import TorchMLP
    meta = json.load(open(os.path.join(work, "meta.json")))
    torch.set_num_threads(int(meta["threads"]))
    xc = torch.from_numpy(np.load(os.path.join(work, "x.npy")))
    yc = torch.from_numpy(np.load(os.path.join(work, "y.npy")))
    xs = torch.from_numpy(np.load(os.path.join(work, "xs.npy")))
    steps, bs, nbat = meta["steps"], meta["bs"], meta["steps"]
    for side, n_orders in (("cpu_bf16", meta["orders"]), ("cpu_fp32", meta["orders_fp32"])):
        out = []
        for o in range(n_orders):
            model = TorchMLP(synthetic_init(0, tuple(meta["units"])), MLPConfig(hidden=tuple(meta["units"])), bf16=(side == "cpu_bf16"))
            seq = acceptance_order(torch, nbat, o)
            for it in range(steps):
                lo = seq[it % nbat] * bs
                model.train_step(xc[lo:lo + bs], yc[lo:lo + bs], meta["lr0"] if it < steps * meta["high_share"] else meta["lr0"] * 0.1)
            with torch.no_grad():
                out.append(model.forward(xs).numpy().copy())
        np.save(os.path.join(work, f"pred_{side}.npy.tmp.npy"), np.stack(out))
        os.replace(os.path.join(work, f"pred_{side}.npy.tmp.npy"), os.path.join(work, f"pred_{side}.npy"))


def acceptance_vs_cpu(torch, device, steps=800, bs=1024, lr0=1e-3, high_share=0.5, orders=6, orders_fp32=3):
    """SURVEY 8(d) "MAE acceptance", synthetic form, inside the bench line.  The cfg-MLP is trained for the SAME `steps` steps on the SAME
    batches (Adam, lr 1e-3, 1e-4 for the second half) from synthetic_init(0) by THREE implementations, `orders` times with the batches
    in another order each time (same rows, same init), and scored on the same held-out rows through the reference's evaluation weighting:
      engine_bf16   the HIP engine (bf16 MFMA operands, float32 accumulate / master weights / Adam),
      cpu_bf16      the torch-CPU restatement of the reference step with the ENGINE'S ARITHMETIC emulated (oracle/mlp_torch_cpu.py,
                    bf16=True: the rounding points of oracle/mlp_oracle.py, which the parity tests hold the kernels to step by step),
      cpu_fp32      the same restatement in float32 - the reference's own arithmetic.
    Two training runs of a 5 x 512 model differ by several per cent on single outputs from the data order alone, in ANY implementation
    (order-to-order sd 2 - 10 %), so every comparison is a paired statistic over the orders (acceptance_check: 2 % + 2 standard errors).
    ASSERTED (`check`, tests/test_bench_gpu.py): engine_bf16 against cpu_bf16 - the engine does what its arithmetic says, end to end.
    REPORTED beside it (`bf16_vs_fp32`, `engine_vs_fp32`, three orders): how bf16 operands differ from float32 after equal steps - round 6
    measured (six orders of 1200 steps) the engine's MAE 2.5 - 6 % BELOW float32's per variable, 2.6 % +- 1.0 % over all outputs, the CPU
    emulation 1.1 % +- 0.4 % below: a one-sided shift of the arithmetic (the emulation on the CPU shows it too) of the size of SURVEY's
    2 % line, printed with its standard error instead of being hidden in a wide bar."""
    import shutil
    import subprocess
    import tempfile
    import numpy as np
    from climsim_amd.mlp import MLPEmulator
    steps, lr0, high_share = int(os.environ.get("CS_ACC_STEPS", steps)), float(os.environ.get("CS_ACC_LR", lr0)), float(os.environ.get("CS_ACC_HIGH", high_share))
    orders = int(os.environ.get("CS_ACC_ORDERS", orders))
    nbat = steps                                         # every batch is fresh: no row is seen twice (32 recycled batches overfit the noise: R2 < 0 on both sides)
    x, y = synth_on_device(torch, nbat * bs, 4242, device, signal=(3.0, 0.3))
    xs, ys = synth_on_device(torch, 12 * 384, 4243, device, signal=(3.0, 0.3))
    t0 = time.perf_counter()
    names = ("engine_bf16", "cpu_bf16", "cpu_fp32")
    # the CPU sides are a CHILD PROCESS (acceptance_cpu_worker: no GPU call, its own thread pool) that trains while this process drives
    # the engine; the batches travel through files in shared memory.  Its time is the leg's time: a GPU box grants this job ~16 cores
    # (cpu_baseline: 16 of 256 threads are the fastest), on which one float32 step of batch 1024 takes ~10 ms and the bf16 emulation ~12 -
    # hence 800 steps, the emulation (the asserted side) for all six orders and float32 (information) for three: ~100 s.
    #   (Tried: both CPU models on two threads of this process, and two child processes side by side - 310 / 318 s for 2 x 6 x 1200 steps.)
    orders_fp32 = min(int(os.environ.get("CS_ACC_ORDERS_FP32", orders_fp32)), orders)
    need = (x.numel() + y.numel() + xs.numel()) * 4 + (64 << 20)
    shm = None                                           # shared memory if it has room for the batches (a container's default /dev/shm is 64 MB), else the temp dir
    for cand in ("/dev/shm", tempfile.gettempdir()):
        try:
            if os.path.isdir(cand) and os.access(cand, os.W_OK) and shutil.disk_usage(cand).free > need:
                shm = cand
                break
        except OSError:
            pass
    work = tempfile.mkdtemp(prefix="cs_acc_", dir=shm)
    children = {}
    try:
        np.save(os.path.join(work, "x.npy"), x.cpu().numpy())
        np.save(os.path.join(work, "y.npy"), y.cpu().numpy())
        np.save(os.path.join(work, "xs.npy"), xs.cpu().numpy())
        threads = max(1, min(16, os.cpu_count() or 1))
        with open(os.path.join(work, "meta.json"), "w") as f:
            json.dump({"steps": steps, "bs": bs, "orders": orders, "orders_fp32": orders_fp32, "lr0": lr0, "high_share": high_share, "units": list(UNITS),
                       "threads": threads}, f)
        env = dict(os.environ, OMP_NUM_THREADS=str(threads), MKL_NUM_THREADS=str(threads))
        children["cpu"] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--acceptance-cpu-worker", work], env=env,
                                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        preds = {k: [] for k in names}
        for o in range(orders):
            m = MLPEmulator(units=UNITS, activation="leakyrelu", optimizer="Adam", max_batch=12 * 384, seed=None, device=device.index)
            m.set_weights(synthetic_init(0))
            seq = acceptance_order(torch, nbat, o)
            for it in range(steps):
                lo = seq[it % nbat] * bs
                m.train_on_batch(x[lo:lo + bs], y[lo:lo + bs], lr0 if it < steps * high_share else lr0 * 0.1)
            preds["engine_bf16"].append(m.predict(xs, as_numpy=False).clone())
            m.close()
        pr = children["cpu"]
        try:
            _, err = pr.communicate(timeout=900)
        except subprocess.TimeoutExpired:
            pr.kill()
            raise RuntimeError("the CPU worker of the acceptance leg did not finish in 900 s")
        if pr.returncode != 0:
            raise RuntimeError(f"the CPU worker of the acceptance leg failed: {err.decode(errors='replace')[-400:]}")
        for side in ("cpu_bf16", "cpu_fp32"):
            arr = np.load(os.path.join(work, f"pred_{side}.npy"))
            preds[side] = [torch.from_numpy(arr[o]).to(device).contiguous() for o in range(arr.shape[0])]
    finally:
        for pr in children.values():
            if pr.poll() is None:
                pr.kill()
        shutil.rmtree(work, ignore_errors=True)
    tables = {k: [] for k in names}
    overall = {k: [] for k in names}
    first = {}
    for o in range(orders):
        for name in names:
            if o >= len(preds[name]):
                continue
            pr = preds[name][o]
            e = (pr - ys).double()
            t = per_variable_tables(pr, ys, xs)
            tables[name].append(t["MAE"])
            overall[name].append(float(e.abs().mean()))
            if o == 0:
                first[name] = {"mse": float((e * e).mean()), "mae": float(e.abs().mean()), **t}
    nf = len(tables["cpu_fp32"])                         # the float32 side ran the first `orders_fp32` orders: paired with the same orders of the others
    out = {"task": f"cfg-MLP from synthetic_init(0), {steps} steps of batch {bs} (fresh rows every step, the same batches in the same order on every side), lr 1e-3 then 1e-4 for the second half; "
                   f"targets tanh(3 xA) * 0.3 + noise (the recipe with a stronger signal, as the acceptance test); held-out {12 * 384} rows; {orders} data orders (float32 side: the first {nf})",
           "seconds": round(time.perf_counter() - t0, 1), **first}
    out["check"] = acceptance_check(tables, overall, ("engine_bf16", "cpu_bf16"))
    t3 = {k: v[:nf] for k, v in tables.items()}
    o3 = {k: v[:nf] for k, v in overall.items()}
    out["bf16_vs_fp32"] = acceptance_check(t3, o3, ("cpu_bf16", "cpu_fp32"))
    out["engine_vs_fp32"] = acceptance_check(t3, o3, ("engine_bf16", "cpu_fp32"))
    for k in ("bf16_vs_fp32", "engine_vs_fp32"):
        out[k] = {kk: out[k][kk] for kk in ("orders", "sides", "engine_vs_cpu", "allowed", "all_outputs", "per_variable_passed", "all_outputs_passed", "worst_variable", "margin")}
        out[k]["note"] = "information: what bf16 operands cost against float32 after equal steps, with its standard error; SURVEY 8(d) drew the line at 2 %"
    out["max_rel_diff_MAE"] = max(out["engine_vs_fp32"]["engine_vs_cpu"]["of_the_order_means"].values())
    out["rel_diff_mae_all_outputs"] = round(abs(first["engine_bf16"]["mae"] - first["cpu_fp32"]["mae"]) / first["cpu_fp32"]["mae"], 5)
    r2 = [(first["engine_bf16"]["R2"][v], first["cpu_fp32"]["R2"][v]) for v in first["cpu_fp32"]["R2"]]
    out["min_R2"] = {"engine_bf16": min(a for a, b in r2 if a is not None), "cpu_fp32": min(b for a, b in r2 if b is not None)}
    return out


PUB_UNITS = (768, 640, 512, 640, 640)       # published lot-147 / trial_0027 (step1_results.csv:170)
PUB_TRAIN_FLOPS_PER_COL = 10_309_632


def pub_mlp_side_bench(torch, device, cpu_budget, batch=3072, steps=200):
    """SURVEY 8(d) config (1) names the published model beside the cfg-MLP: training columns/s of 768-640-512-640-640, RAdam,
    at its published batch 3072 on the GPU, and the torch-CPU restatement of the same model at batch 1024 (its own cpu_baseline)."""
    from climsim_amd.mlp import MLPEmulator
    m = MLPEmulator(units=PUB_UNITS, activation="leakyrelu", optimizer="RAdam", max_batch=batch, seed=None, device=device.index)
    m.set_weights(synthetic_init(0, PUB_UNITS))
    x, y = synth_on_device(torch, 16 * batch, 99, device)
    loss = torch.zeros(2, dtype=torch.float32, device=device)
    for i in range(20):
        m.train_on_batch(x[(i % 16) * batch:(i % 16 + 1) * batch], y[(i % 16) * batch:(i % 16 + 1) * batch], 2.5e-4, loss=loss)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        m.train_on_batch(x[(i % 16) * batch:(i % 16 + 1) * batch], y[(i % 16) * batch:(i % 16 + 1) * batch], 2.5e-4, loss=loss)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    m.close()
    out = {"workload": "published MLP 124->768-640-512-640-640->128->(120||8), LeakyReLU, RAdam lr 2.5e-4, batch 3072 (step1_results.csv:170, step2_retrain.py)",
           "columns_per_s": round(batch / dt, 1), "ms_per_step": round(dt * 1e3, 4),
           "tflops_algorithmic": round(PUB_TRAIN_FLOPS_PER_COL * batch / dt / 1e12, 1),
           "frac_of_bf16_peak": round(PUB_TRAIN_FLOPS_PER_COL * batch / dt / 1e12 / PEAK_BF16_TFLOPS, 4)}
    if cpu_budget > 0:
        from oracle.mlp_oracle import MLPConfig, glorot_init, synth_columns
        from oracle.mlp_torch_cpu import time_cpu_baseline
        cfg = MLPConfig(hidden=PUB_UNITS)
        xc, yc = synth_columns(8192, seed=2)
        cpu = time_cpu_baseline(glorot_init(cfg, 0), cfg, xc, yc, batch=1024, budget_s=cpu_budget)
        cpu["value"] = round(cpu["value"], 1)
        cpu["sample"] += " (Adam in place of RAdam: same cost per step)"
        out["cpu_baseline"] = cpu
    return out


def cnn_side_bench(batch=512, steps=30):
    """Level-axis CNN (depth 12, width 406; hpo_train.py): training step and prediction, columns/s."""
    import torch
    from climsim_amd.cnn import CNNEmulator
    m = CNNEmulator(depth=12, channel_width=406, max_batch=batch, trainable=True, init_seed=0, seed=1)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = (torch.rand((batch, 124), device="cuda", generator=g) - 0.5).contiguous()
    y = (torch.rand((batch, 128), device="cuda", generator=g) * 0.1).contiguous()

    def timed(fn, reps):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    dt = timed(lambda: m.train_on_batch(x, y, 1e-4, x3d=0, y3d=0), steps)
    dp = timed(lambda: m.predict(x, as_numpy=False), steps)
    out = {"workload": "CNN depth 12 width 406, batch 512, dropout 0.175, mae_adjusted, Adam", "train_columns_per_s": round(batch / dt, 1),
           "ms_per_step": round(dt * 1e3, 3), "train_tflops_algorithmic": round(3 * 1.584e9 * batch / dt / 1e12, 1),
           "frac_of_bf16_peak": round(3 * 1.584e9 * batch / dt / 1e12 / PEAK_BF16_TFLOPS, 4),
           "predict_columns_per_s": round(batch / dp, 1)}
    m.close()
    return out


def stream_side_bench():
    """BASELINE config 5 on one GPU: cfg-MLP trained from raw high-res-shaped fields through the device loader (bench_stream.py)."""
    import bench_stream
    r = bench_stream.run(4, 8, 8192)
    return {k: r[k] for k in ("workload", "value", "unit", "train_only_columns_per_s", "loader_only_columns_per_s", "serial_sum_columns_per_s",
                              "ratio_to_train_only", "ratio_to_serial_sum")}


def loader_side_bench(steps=16, ncol=21600):
    """Device loader on high-res-shaped timesteps (float64 raw fields in HBM -> normalised float32 rows)."""
    import types
    import numpy as np
    import torch
    from climsim_amd.loader import GpuColumnLoader
    vin = ["state_t", "state_q0001", "state_ps", "pbuf_SOLIN", "pbuf_LHFLX", "pbuf_SHFLX"]
    vout = ["ptend_t", "ptend_q0001", "cam_out_NETSW", "cam_out_FLWDS", "cam_out_PRECSC", "cam_out_PRECC", "cam_out_SOLS", "cam_out_SOLL",
            "cam_out_SOLSD", "cam_out_SOLLD"]
    lens = {v: 60 if v in ("state_t", "state_q0001", "ptend_t", "ptend_q0001") else 1 for v in vin + vout}
    rng = np.random.default_rng(0)
    du = types.SimpleNamespace(input_vars=vin, target_vars=vout, var_lens=lens, normalize=True, input_abbrev="mli", output_abbrev="mlo",
                               save_norm=lambda: (rng.normal(0, 1, 124), rng.uniform(0.5, 2, 124), rng.uniform(0.5, 2, 128)))
    ld = GpuColumnLoader(du)
    a = torch.rand((steps, 124, ncol), device="cuda", dtype=torch.float64)
    b = torch.rand((steps, 128, ncol), device="cuda", dtype=torch.float64)
    for _ in range(3):
        ld.stack_raw(a, b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        ld.stack_raw(a, b)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 10
    cols = steps * ncol
    gbs = cols * 3024 / dt / 1e9
    return {"workload": f"{steps} timesteps x {ncol} columns, float64 sources", "columns_per_s": round(cols / dt, 1),
            "roofline": {"bound": "hbm", "achieved": round(gbs, 1), "peak": 8000.0, "unit": "GB/s", "frac": round(gbs / 8000.0, 3)}}


class LegFailed(RuntimeError):
    """A leg failed on SOME rank (agreed on with a MAX all-reduce in timed_blocks): every rank raises it together."""


def inject_failure(where, rank):
    """Test switch: CS_BENCH_INJECT_FAIL="<rank>:<where>" raises on that rank at that point (tests/test_bench_gpu.py)."""
    spec = os.environ.get("CS_BENCH_INJECT_FAIL", "")
    if spec and spec.split(":")[0] == str(rank) and spec.split(":")[1] == where:
        raise RuntimeError(f"injected failure on rank {rank} at '{where}' (CS_BENCH_INJECT_FAIL)")


class FailureReporter:
    """N > 1: a failure of ANY rank before the JSON line must still end in ONE line from rank 0 (with "error") and a non-zero
    exit - no re-exec, no second attempt in this process tree.  A failing rank r > 0 leaves its message in a run-private
    directory and exits 1; the launcher (torch.distributed.run) then sends SIGTERM to the other ranks.  Rank 0 may be blocked
    inside a collective or a stream synchronisation at that moment, where a Python-level signal handler never runs: it keeps a
    watcher THREAD on the interpreter's signal wake-up pipe (`signal.set_wakeup_fd`: written from the C-level handler), which
    prints the error line and ends the process.  Rank 0's own exceptions print the line directly.
    (online_testing/.../train_mlp_h5loader.py:195-207,470-473 relies on torchrun's teardown alone.)"""

    def __init__(self, rank, world):
        import tempfile
        self.rank, self.world, self.done = rank, world, False
        # one directory per launch: the ranks share their parent (the launcher), so its pid names the run and nothing stale is read
        self.dir = os.path.join(tempfile.gettempdir(), "cs_bench_%s_%d" % (os.environ.get("MASTER_PORT", "0"), os.getppid()))
        os.makedirs(self.dir, exist_ok=True)
        if rank == 0 and world > 1:
            import signal
            import threading
            r, w = os.pipe()
            os.set_blocking(w, False)
            signal.set_wakeup_fd(w, warn_on_full_buffer=False)
            signal.signal(signal.SIGTERM, lambda *_: None)         # keep the default action (die silently) from running
            threading.Thread(target=self._watch, args=(r, int(signal.SIGTERM)), daemon=True).start()

    def _watch(self, rfd, sigterm):
        while True:
            data = os.read(rfd, 16)
            if not data:
                return
            if sigterm in data and not self.done:
                time.sleep(0.3)                                    # the failing rank writes its message before it exits
                self.emit("terminated by the launcher (SIGTERM): another rank failed")
                os._exit(1)

    def peer_errors(self):
        out = {}
        try:
            for f in sorted(os.listdir(self.dir)):
                if f.startswith("rank") and f.endswith(".err"):
                    out[f[4:-4]] = open(os.path.join(self.dir, f)).read()[:600]
        except OSError:
            pass
        return out

    def emit(self, msg):
        line = json.dumps({"metric": "training columns/sec", "value": None, "unit": "columns/s", "n_gpus": self.world,
                           "error": msg[:600], "failed_ranks": self.peer_errors()})
        sys.stdout.write(line + "\n")
        sys.stdout.flush()

    def fail(self, exc):
        import traceback
        msg = f"{type(exc).__name__}: {exc}"
        if self.rank == 0:
            self.done = True
            self.emit(msg)
        else:
            try:
                with open(os.path.join(self.dir, f"rank{self.rank}.err"), "w") as f:
                    f.write(msg + "\n" + traceback.format_exc()[-400:])
            except OSError:
                pass
        traceback.print_exc()
        sys.stderr.flush()
        os._exit(1)                                                # no teardown collectives: the group is broken


def sweep_point(torch, device, b, steps, blocks=10, lr=1e-3):
    """One more batch size of SURVEY 8(d) config (2) (B in {1024, 8192, 65536}) in the driver's line: `blocks` blocks of `steps`
    steps (median), AFTER the headline's timed region and on a model of its own, plus the per-kernel event pass for the dominant kernel."""
    import ctypes
    from climsim_amd import _lib
    from climsim_amd.mlp import MLPEmulator
    m = MLPEmulator(units=UNITS, activation="leakyrelu", optimizer="Adam", max_batch=b, seed=None, device=device.index,
                    cooperative=b <= 2048)                       # one process on this GPU: small batches take the cooperative chain
    m.set_weights(synthetic_init(0))
    rows = max(4 * b, 1 << 18)
    x, y = synth_on_device(torch, rows, 4321, device)
    g = torch.Generator(device=device)
    g.manual_seed(99)
    perm = torch.randperm(rows, device=device, generator=g)
    loss = torch.zeros(2, dtype=torch.float32, device=device)
    nb = rows // b

    def step(i):
        m.train_on_batch(x, y, lr, row_idx=perm[(i % nb) * b:(i % nb + 1) * b], loss=loss)
    for i in range(max(5, steps // 2)):
        step(i)
    secs = []
    for k in range(blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            step(k * steps + i)
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
        m.check()
    med = sorted(secs)[len(secs) // 2] / steps
    reps = 20
    with _lib.profile_session(ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)) as prof:
        for r in range(reps):
            step(r)
    ks = {k: v[0] / reps for k, v in prof.times.items() if v[1] > 0}            # ms per step, raw event durations
    scale = min(1.0, med * 1e3 / sum(ks.values())) if ks else 1.0
    dom = max((k for k in FLOPS_PER_COL if k in ks), key=lambda k: ks[k])
    dom_ms = ks[dom] * scale
    out = {"per_gpu_batch": b, "value": round(b / med, 1), "unit": "columns/s", "ms_per_step": round(med * 1e3, 4), "blocks": blocks,
           "steps_per_block": steps, "cooperative_chain": bool(b <= 2048),
           "whole_step_frac": round(TRAIN_FLOPS_PER_COL * b / med / 1e12 / PEAK_BF16_TFLOPS, 4),
           "dominant_kernel": KERNEL_NAMES[dom], "dominant_us": round(dom_ms * 1e3, 2),
           "dominant_frac": round(FLOPS_PER_COL[dom] * b / (dom_ms * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
           "kernels_us": {k: round(v * scale * 1e3, 2) for k, v in ks.items()}, "coop_timeouts": m.coop_timeouts}
    m.close()
    del x, y
    torch.cuda.empty_cache()
    return out


def agree_or_raise(torch, dist, device, err, msg):
    """Every rank learns whether ANY rank failed (MAX all-reduce of a flag) and all raise LegFailed together."""
    if dist:
        t = torch.tensor([1.0 if err else 0.0], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        err = float(t.item()) > 0
    if err:
        raise LegFailed(msg or "another rank failed in this leg")


def timed_blocks(torch, dist, device, step, steps, first_step, min_seconds, max_blocks=2000, after_block=None, warmup=0):
    """Blocks of EXACTLY `steps` steps, each bracketed by barrier + synchronize on both sides and reduced with MAX over the
    ranks, repeated until the blocks add up to `min_seconds` of step time (a 3 ms region says little about a GPU that has
    not reached its clocks).  Returns the per-block seconds.  `warmup` untimed steps run first.  A failure of `after_block`
    (the engine's health check between blocks: every rank is at the same point, outside any collective) on ANY rank travels
    with the block's time through the MAX all-reduce, so that every rank raises LegFailed together instead of one rank leaving
    the others inside the next barrier.  (A step that raises on one rank cannot be absorbed - the others are inside the step's
    collective - and ends the run: FailureReporter.)"""
    secs, it = [], first_step
    for i in range(warmup):
        step(i)
    while True:
        if dist:
            dist.barrier()
        torch.cuda.synchronize()
        err, msg = 0.0, ""
        t0 = time.perf_counter()
        for i in range(steps):
            step(it + i)
        torch.cuda.synchronize()
        if dist:
            dist.barrier()
        el = time.perf_counter() - t0
        if after_block:
            try:
                after_block()                    # outside the timed interval: e.g. the cooperative chain's time-out counter
            except Exception as e:               # noqa: BLE001
                err, msg = 1.0, f"{type(e).__name__}: {e}"
        if dist:
            t = torch.tensor([el, err * (dist.get_rank() + 1)], dtype=torch.float64, device=device)      # (which rank: the highest that failed)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el, err = float(t[0].item()), float(t[1].item())
        if err:
            raise LegFailed(msg or "rank %d failed its health check in this leg" % (int(err) - 1))
        secs.append(el)
        it += steps
        # every rank sees the same (MAX-reduced) times, so all take the same decision
        if sum(secs) >= min_seconds or len(secs) >= max_blocks:
            return secs


def block_stats(secs, steps, cols_per_step):
    s = sorted(secs)
    med = s[len(s) // 2]
    return {"blocks": len(s), "steps_per_block": steps, "timed_seconds": round(sum(s), 4),
            "ms_per_step": {"min": round(s[0] / steps * 1e3, 4), "median": round(med / steps * 1e3, 4), "max": round(s[-1] / steps * 1e3, 4)},
            "columns_per_s": {"best": round(cols_per_step * steps / s[0], 1), "median": round(cols_per_step * steps / med, 1),
                              "worst": round(cols_per_step * steps / s[-1], 1)}}, med


def dump_outputs(out_dir, model, loss):
    """What the timed path hands its caller after its last step, as `out_dir/<name>.npy` (float32, ~14 MB for the cfg-MLP):
    `loss` = that step's [sum of squared errors, sum of absolute errors] over its batch (the device tensor train_on_batch returns),
    `weight_NN` = the model's arrays in Keras order (kernel (in, out), bias, ...), `adam_m_NN` / `adam_v_NN` = the optimiser's
    moments in the same order.  Data, initial weights and batch order are seeded, so two builds run with the same arguments can
    be compared array for array.  Returns the names written."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {"loss": loss.detach().cpu().numpy()}
    arrays.update({"weight_%02d" % i: w for i, w in enumerate(model.get_weights())})
    m, v, _ = model.get_optimizer_state()
    arrays.update({"adam_m_%02d" % i: a for i, a in enumerate(m)})
    arrays.update({"adam_v_%02d" % i: a for i, a in enumerate(v)})
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))
    return sorted(arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8192, help="per-GPU batch (columns per rank per step)")
    ap.add_argument("--rows", type=int, default=1 << 20, help="HBM-resident synthetic rows per GPU")
    ap.add_argument("--min-seconds", type=float, default=0.0, help="repeat the --steps block until this much step time is measured "
                    "(default 0: one block, so that the timed region is exactly --steps steps)")
    ap.add_argument("--strong-global-batch", type=int, default=8192, help="N>1: global batch of the strong-scaling leg (BASELINE configs[3]); 0 = skip")
    ap.add_argument("--weak-large-batch", type=int, default=65536, help="N>1: per-GPU batch of a second weak-scaling leg (0 = skip)")
    ap.add_argument("--grad-payload", choices=("fp32", "bf16"), default="fp32", help="N>1: what the gradient all-reduce sends (fp32 = the reference's DDP; "
                    "bf16 = half the bytes, cs_dp_allreduce_bf16); both are timed and reported in `comm` either way")
    ap.add_argument("--collective", choices=("rccl", "oneshot"), default="rccl", help="N>1: the gradient all-reduce of the timed steps: RCCL (default) or "
                    "the one-kernel all-reduce over peer-mapped buffers (cs_dp_ipc_*); the other one is timed on its own and reported in `comm`")
    ap.add_argument("--time-oneshot", action="store_true", help="N>1 with --collective rccl: also time the one-shot all-reduce on its own (`comm.allreduce_us_oneshot_ipc`). "
                    "Off by default: that path has only run with two processes on ONE device, and a fault in it must not take a scaling run down")
    ap.add_argument("--cpu-budget", type=float, default=15.0, help="seconds of CPU-baseline timing (0 = skip)")
    ap.add_argument("--no-profile", action="store_true", help="skip the per-kernel HIP-event pass")
    ap.add_argument("--no-extras", action="store_true", help="skip the side figures")
    ap.add_argument("--extras", default="pub_mlp,cnn,loader,stream,sweep", help="which side figures to take (comma-separated)")
    ap.add_argument("--train-only", action="store_true", help="counter runs: nothing but the training steps (no held-out "
                    "evaluation, no prediction pass), so that per-kernel averages are averages over training launches")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed "
                    "(its loss sums, the model's weights and Adam moments) to DIR/<name>.npy, float32 (see dump_outputs)")
    args = ap.parse_args()

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: what RCCL needs between the ranks of this pool's hosts
    if args.collective == "oneshot" or args.time_oneshot:
        os.environ.setdefault("CS_DP_IPC_MULTI_DEVICE", "1")     # the flags ARE the caller's consent to a path that has not run over xGMI yet
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus > 1 and "RANK" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus, sys.argv[1:]))   # parent: no GPU call, children do the work
    rank = int(os.environ.get("RANK", "0"))
    reporter = FailureReporter(rank, world) if world > 1 else None
    try:
        run(args, world, rank)
    except SystemExit:
        raise
    except BaseException as e:               # noqa: BLE001 - N > 1: rank 0 must still print ONE line (with "error") and exit non-zero
        if reporter is None:
            raise
        reporter.fail(e)
    if reporter is not None:
        reporter.done = True


def run(args, world, rank):
    import torch
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    args.gpus = world
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback for the engine)")
    inject_failure("start", rank)
    # development / tests: every rank on cuda:0 with gloo collectives, so that the N > 1 flow of this file (barriers, MAX over
    # ranks, strong leg, comm figures, rank 0's line) can run on a one-GPU box; RCCL cannot put two ranks on one device
    share_gpu = os.environ.get("CS_BENCH_SHARE_GPU") == "1"
    if share_gpu:
        local_rank = 0
        os.environ["CS_DP_NATIVE"] = "0"
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    force_dist = os.environ.get("CS_BENCH_FORCE_DIST") == "1"     # development: run the N > 1 code path with a one-rank RCCL group
    multi = world > 1 or force_dist
    if multi:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if force_dist and world == 1:
            os.environ.setdefault("MASTER_PORT", "29517")
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=device)
        elif share_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=device)

    from climsim_amd import build
    if rank == 0:
        build.build()
    if dist:
        dist.barrier()
    from climsim_amd.mlp import MLPEmulator

    B = args.batch
    gb = args.strong_global_batch if multi else 0
    sb = gb // world if (gb and gb % world == 0 and gb // world >= 128) else 0       # per-GPU batch of the strong leg
    WL = args.weak_large_batch if (multi and args.weak_large_batch != B) else 0       # second weak leg: compute hides the collective's share
    model = MLPEmulator(units=UNITS, activation="leakyrelu", optimizer="Adam", max_batch=max(B, sb, gb if sb else 0, WL), seed=None, device=local_rank,
                        flags=int(os.environ.get("CS_FLAGS", "0")),   # engine flags: tuning experiments only
                        cooperative=not multi)                         # one process on the GPU: a --batch <= 2048 headline may take the cooperative
                                                                       # chain; under N > 1 the strong leg runs WITHOUT it first and with it second
    model.set_weights(synthetic_init(0))
    x, y = synth_on_device(torch, args.rows, 20230614 + rank, device)
    xv, yv = synth_on_device(torch, 65536, 777, device)
    model.gradient_tensor()
    loss = torch.zeros(2, dtype=torch.float32, device=device)
    lr = 1e-3
    gen = torch.Generator(device=device)
    gen.manual_seed(1234 + rank)
    perm = torch.randperm(args.rows, device=device, generator=gen)

    from climsim_amd.dp import DataParallel
    dp = DataParallel(model, dist if multi else None, grad_payload=args.grad_payload, collective=args.collective if multi else None)
    dp.broadcast_weights()

    def make_step(b, collective=True, one_call=False, mdl=None, dpx=None):
        # every rank owns its own HBM-resident shard of the split, so its local batch is a slice of
        # its own permutation (equivalent to the round-robin deal of a global permutation)
        mdl, dpx = mdl or model, dpx or dp
        nb = args.rows // b
        scale = 1.0 / (128.0 * b * (world if collective else 1))

        def step(i):
            idx = perm[(i % nb) * b:(i % nb + 1) * b]
            if multi and not one_call:
                mdl.loss_grads(x, y, row_idx=idx, loss=loss)
                if collective:
                    dpx.all_reduce_grads()                          # ONE RCCL all-reduce per step (cs_dp_allreduce, compute stream)
                mdl.apply_gradients(lr, scale)
            else:
                mdl.train_on_batch(x, y, lr, row_idx=idx, loss=loss)
        return step

    def timed(stepfn, cols_per_step, mdl=None, tag=None):
        def health():
            if tag:
                inject_failure(tag, rank)        # tests: a rank whose check fails between two blocks
            (mdl or model).check()               # e.g. a bounded wait of the cooperative chain that ran out on this rank
        secs_ = timed_blocks(torch, dist, device, stepfn, args.steps, args.warmup, args.min_seconds, after_block=health, warmup=args.warmup)
        st_, med_ = block_stats(secs_, args.steps, cols_per_step)
        return st_, med_

    from climsim_amd._lib import EngineError

    def agreed(fn):
        """A leg that must not take the line down: its outcome ({"error": ...} or its result) is the SAME on every rank.  Only
        failures that every rank sees together are absorbed here: LegFailed (health checks between blocks, agreed on in
        timed_blocks) and the EngineError of the native communicators' set-up (RcclComm / IpcComm raise on every rank or on none).
        Anything else - one rank alone - would leave the others inside a collective: it ends the run through FailureReporter."""
        try:
            return fn()
        except (LegFailed, EngineError) as e:
            return {"error": f"{type(e).__name__}: {e}"[:300]}

    step = make_step(B)
    for i in range(args.warmup):
        step(i)
    with ClockSampler(local_rank) as clk:
        secs = timed_blocks(torch, dist, device, step, args.steps, args.warmup, args.min_seconds, after_block=model.check)
    timing, med = block_stats(secs, args.steps, B * world)
    ms_per_step = med / args.steps * 1e3                            # the median block: EXACTLY --steps steps between barriers
    value = B * world * args.steps / med
    if args.dump_outputs and rank == 0:                             # before any other leg touches the model
        dump_outputs(args.dump_outputs, model, loss)
    held = None if args.train_only else model.evaluate(xv, yv)      # the model the timed region trained, before any other leg touches it
    per_var = None
    if rank == 0 and not args.train_only:
        per_var = side_bench(lambda: heldout_per_variable(model, xv, yv))

    # ---- N > 1: the collective on its own (HIP events on the compute stream around cs_dp_allreduce), the strong-scaling leg
    # (BASELINE configs[3]) set beside ONE GPU at the same global batch, and a second weak leg at a batch whose compute hides the collective
    comm = None
    strong = None
    weak_large = None
    if multi:
        def collective_us(payload, dpx=None):
            """median over 20 steps of the slowest rank's event pair around the collective (all ranks run the same sequence)"""
            dpx = dpx or dp
            keep, dpx.payload = dpx.payload, payload
            evs = []
            for i in range(20):
                idx = perm[i * B:(i + 1) * B]
                model.loss_grads(x, y, row_idx=idx, loss=loss)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dpx.all_reduce_grads()
                e1.record()
                model.apply_gradients(lr, 1.0 / (128.0 * B * world))
                evs.append((e0, e1))
            torch.cuda.synchronize()
            dpx.payload = keep
            ar = sorted(a.elapsed_time(b) * 1e3 for a, b in evs)
            t = torch.tensor([ar[len(ar) // 2]], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return round(float(t.item()), 1)

        n_grad = int(model.gradient_tensor().numel())
        us = {pl: collective_us(pl) for pl in (("fp32", "bf16") if dp.collective == "rccl" else ("fp32",))}
        us.setdefault("bf16", None)
        rccl_n, rccl_r = None, None
        if dp.native is not None and dp.collective == "rccl":
            try:
                rccl_n, rccl_r = dp.native.info()
            except Exception:                                        # an RCCL without ncclCommCount: report nothing rather than fail the run
                pass
        # the OTHER collective on its own, same 20 steps (the one-shot all-reduce rebinds the engine's gradient buffer to its
        # exchange buffer while it exists; RCCL's communicator works on whatever buffer the engine holds)
        other_us, other_err = None, None
        if dp.collective == "rccl" and args.time_oneshot:
            from climsim_amd._lib import EngineError
            try:
                dpo = DataParallel(model, dist, collective="oneshot")
                other_us = collective_us("fp32", dpo)
                other_err = ("%d waits timed out" % dpo.native.timeouts) if dpo.native.timeouts else None
                dpo.close()
            except EngineError as e:                                # raised on every rank or on none (IpcComm agrees on each step)
                other_err = str(e)[:200]
            dp.grad = model.gradient_tensor()
        comm = {"collective": ("one-kernel all-reduce over peer-mapped buffers (cs_dp_ipc_allreduce)" if dp.collective == "oneshot" else
                               "ncclAllReduce(sum) of the flat gradient, issued on the compute stream (cs_dp_allreduce%s)" % ("_bf16" if dp.payload == "bf16" else ""))
                if dp.native is not None else "torch.distributed.all_reduce", "nranks": dist.get_world_size(),
                "allreduce_us_oneshot_ipc": other_us if dp.collective == "rccl" else us["fp32"], "oneshot_ipc_error": other_err,
                "rccl_comm_count": rccl_n, "rccl_user_rank": rccl_r,       # ncclCommCount / ncclCommUserRank of the engine's own communicator (rank 0's view)
                "rccl_comm_matches_nranks": (rccl_n == dist.get_world_size()) if rccl_n is not None else None,
                "payload": dp.payload, "bytes": n_grad * (2 if dp.payload == "bf16" else 4), "allreduce_us_per_step": us[dp.payload],
                "allreduce_us_fp32_payload": us["fp32"], "allreduce_us_bf16_payload": us["bf16"],
                "note": "median over 20 steps of the slowest rank's event pair around the collective; includes the wait for the slowest "
                        "rank's gradients; the timed steps use `payload` (--grad-payload; bf16 adds a pack and an unpack kernel inside the pair)"}
        if sb:
            def strong_leg(mdl, dpx, coop):
                st, smed = timed(make_step(sb, mdl=mdl, dpx=dpx), gb, mdl, tag="strong_coop_check" if coop else "strong_check")
                # what the leg has to beat, measured by every rank on its own GPU with no collective: (a) the per-GPU share of the
                # work alone (what is left is the exposed collective), (b) ONE GPU taking the whole global batch (MAX over ranks)
                _, cmed = timed(make_step(sb, collective=False, mdl=mdl, dpx=dpx), sb, mdl)
                _, omed = timed(make_step(gb, collective=False, one_call=True, mdl=mdl, dpx=dpx), gb, mdl)
                v_strong, v_one = gb * args.steps / smed, gb * args.steps / omed
                return {"scaling": "strong", "global_batch": gb, "per_gpu_batch": sb, "value": round(v_strong, 1), "unit": "columns/s",
                        "cooperative_chain": bool(coop and sb <= 2048),
                        "ms_per_step": round(smed / args.steps * 1e3, 4), "timing": st,
                        "compute_only_ms_per_step": round(cmed / args.steps * 1e3, 4),
                        "predicted_ms_per_step": round(cmed / args.steps * 1e3 + us[dp.payload] * 1e-3, 4),
                        "one_gpu_same_global_batch": {"value": round(v_one, 1), "ms_per_step": round(omed / args.steps * 1e3, 4)},
                        "speedup_vs_one_gpu": round(v_strong / v_one, 3), "scales": bool(v_strong > v_one),
                        "verdict": ("%d GPUs beat one GPU at global batch %d" % (world, gb)) if v_strong > v_one else
                                   ("NOT scaling: one GPU at global batch %d is faster than %d GPUs at %d columns each - the step is "
                                    "compute + one exposed all-reduce, and at this per-GPU batch the collective outweighs the compute it saves" % (gb, world, sb)),
                        "config": "BASELINE configs[3]: MLP DDP, RCCL all-reduce over xGMI, global batch 8192"}
            # first WITHOUT the cooperative chain (plain launches only: nothing in it waits for another workgroup), then - where the
            # per-GPU batch is small enough for it - WITH it, on a model of its own; each leg's failure stays inside its object
            strong = agreed(lambda: strong_leg(model, dp, False))
            if sb <= 2048 and os.environ.get("CS_BENCH_STRONG_COOP", "1") != "0":
                def coop_leg():
                    # (two ranks sharing ONE device - the tests' stand-in for N > 1 - must not launch cooperatively: the leg's flow runs, plain)
                    m2, err = None, ""
                    try:
                        m2 = MLPEmulator(units=UNITS, activation="leakyrelu", optimizer="Adam", max_batch=max(sb, gb), seed=None, device=local_rank, cooperative=not share_gpu)
                        m2.set_weights(synthetic_init(0))
                        m2.gradient_tensor()
                    except EngineError as e:
                        err = str(e)
                    try:
                        agree_or_raise(torch, dist, device, bool(err), err)      # every rank has its model, or no rank goes on
                        dp2 = DataParallel(m2, dist, grad_payload=args.grad_payload, collective=args.collective)
                        try:
                            return strong_leg(m2, dp2, True)
                        finally:
                            torch.cuda.synchronize()
                            dp2.close()
                    finally:
                        if m2 is not None:
                            m2.close()
                strong_coop = agreed(coop_leg)
                if isinstance(strong, dict):
                    strong["with_cooperative_chain"] = strong_coop
        if WL:
            def weak_large_leg():
                wt, wmed = timed(make_step(WL), WL * world)
                _, wcmed = timed(make_step(WL, collective=False), WL)
                return {"scaling": "weak", "per_gpu_batch": WL, "global_batch": WL * world, "value": round(WL * world * args.steps / wmed, 1),
                        "unit": "columns/s", "ms_per_step": round(wmed / args.steps * 1e3, 4), "timing": wt,
                        "compute_only_ms_per_step": round(wcmed / args.steps * 1e3, 4),
                        "note": "second weak leg: at this per-GPU batch the step's compute is ~10x the collective"}
            weak_large = agreed(weak_large_leg)

    # ---- untimed: held-out error of the model that was just trained, per-kernel timing, CPU baseline
    if args.train_only:
        if rank == 0:
            print(json.dumps({"metric": "training columns/sec", "value": round(value, 1), "unit": "columns/s", "n_gpus": world,
                              "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "train_only": True}), flush=True)
        if dist:
            torch.cuda.synchronize()
            dp.close()
            dist.destroy_process_group()
        return
    # model.predict throughput (reference: 36.6k-46.7k columns/s on an A100, step3_inference.ipynb) - secondary figure
    # (round 4: calls of 65536 rows - prediction is not bound by max_batch, which sizes the training buffers; one warm-up pass, median of 3)
    n_pred = min(args.rows, 1_681_920)
    model.predict(x[:n_pred], as_numpy=False)
    tps = []
    for _ in range(3):
        torch.cuda.synchronize()
        tp = time.perf_counter()
        model.predict(x[:n_pred], as_numpy=False)
        torch.cuda.synchronize()
        tps.append(time.perf_counter() - tp)
    predict_cps = n_pred / sorted(tps)[1]
    predict_rows_per_call = model._forward_chunk(None)
    roofline, kernels, kernels_note = None, None, None
    if not args.no_profile and rank == 0:
        # per-kernel durations over 40 BACK-TO-BACK steps (no synchronisation between them: the regime of the timed region),
        # every launch carrying its own start / stop events - the dispatch packet's timestamps, what rocprofv3 reports
        import ctypes
        from climsim_amd import _lib
        reps = 40
        nb = args.rows // B
        for r in range(5):
            model.train_on_batch(x, y, lr, row_idx=perm[(r % nb) * B:(r % nb + 1) * B], loss=loss)
        with _lib.profile_session(ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)) as prof:
            for r in range(reps):
                model.train_on_batch(x, y, lr, row_idx=perm[(r % nb) * B:(r % nb + 1) * B], loss=loss)
        agg = {k: list(v) for k, v in prof.times.items()}
        kernels = {k: {"ms_per_step": v[0] / reps, "launches_per_step": v[1] / reps,
                       "avg_us_per_launch": (v[0] / max(v[1], 1)) * 1e3} for k, v in agg.items()}
        kernels = {k: v for k, v in kernels.items() if v["launches_per_step"] > 0}
        # The event pairs are the dispatch packets' begin / end stamps, and those OVERLAP at the kernel boundaries (a
        # dispatch is stamped "begun" while its predecessor drains): round 2's figures added up to 129.2 us for a 122.4 us
        # step, and rocprofv3's own kernel trace agreed with the step, not with the sum.  The per-kernel times below are
        # therefore scaled so that they add up to the measured step (never above it); the raw event sum is kept beside them.
        raw_sum = sum(v["ms_per_step"] for v in kernels.values())
        kscale = min(1.0, ms_per_step / raw_sum) if raw_sum > 0 else 1.0
        for v in kernels.values():
            v["event_ms_per_step"] = v["ms_per_step"]
            v["ms_per_step"] *= kscale
            v["avg_us_per_launch"] *= kscale
        kernels_note = {"event_sum_ms_per_step": round(raw_sum, 5), "scaled_by": round(kscale, 4),
                        "note": "per-kernel times = dispatch-event durations x scaled_by, so that they add up to ms_per_step when the raw events overlap"}
        dom = max((k for k in FLOPS_PER_COL if k in kernels), key=lambda k: kernels[k]["ms_per_step"])
        for k, f in FLOPS_PER_COL.items():
            if k in kernels:
                kernels[k]["tflops"] = f * B / (kernels[k]["ms_per_step"] * 1e-3) / 1e12
        achieved = kernels[dom]["tflops"]
        traffic, traffic_src = pmc_traffic(KERNEL_NAMES[dom], B)
        roofline = {"kernel": KERNEL_NAMES[dom],
                    # `bound`: which of the contract's two rooflines (hbm | mfma) `frac` is priced against - the kernel's arithmetic
                    # intensity on HBM bytes (~7,000 FLOP/B) puts it under the MFMA one.  `limited_by`: what the counters say holds it
                    # there: every workgroup streams all 4.65 MB of weights through its CU for 32 rows.
                    "bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
                    "limited_by": ("each CU's own request path: a 32-row tile pulls all 4.65 MB of weights through its CU (1.19 GB per launch, 26 FLOP per byte) at ~52 of the path's 64 B/clk, where the stream saturates once 64 KB per CU are in flight (a deeper queue changes nothing); halving the L2 traffic alone buys 4 % (profiles/r05_chain_probes.txt, r05_wring_depth.txt)"
                                   if dom == "chain_fb" and B == 8192 else "see DESIGN.md section 4"),
                    "avg_us_per_launch": round(kernels[dom]["avg_us_per_launch"], 2),
                    "launches_per_step": kernels[dom]["launches_per_step"],
                    "flops_per_launch": FLOPS_PER_COL[dom] * B / kernels[dom]["launches_per_step"],
                    "traffic": traffic, "traffic_source": traffic_src,
                    "whole_step": {"achieved": round(TRAIN_FLOPS_PER_COL * B / (ms_per_step * 1e-3) / 1e12, 2),
                                   "frac": round(TRAIN_FLOPS_PER_COL * B / (ms_per_step * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4),
                                   "hbm_algorithmic_GBs": round(HBM_BYTES_PER_COL * B / (ms_per_step * 1e-3) / 1e9, 1)}}
    cpu = None
    if rank == 0 and world == 1 and args.cpu_budget > 0:
        from oracle.mlp_oracle import MLPConfig, glorot_init, synth_columns
        from oracle.mlp_torch_cpu import time_cpu_baseline
        cfg = MLPConfig(hidden=UNITS)
        xc, yc = synth_columns(16384, seed=1)
        cpu = time_cpu_baseline(glorot_init(cfg, 0), cfg, xc, yc, batch=1024, budget_s=args.cpu_budget)
        cpu["value"] = round(cpu["value"], 1)
    acceptance = None
    if rank == 0 and world == 1 and args.cpu_budget > 0:
        acceptance = side_bench(lambda: acceptance_vs_cpu(torch, device))

    # ---- secondary figures of the other section-8 rows (untimed region, rank 0, single GPU): CNN step and device loader
    extras = {}
    n_params = model.count_params()
    coop_timeouts = model.coop_timeouts
    if rank == 0 and world == 1 and not args.no_extras:
        model.close()
        torch.cuda.empty_cache()
        want = set(args.extras.split(","))
        if "pub_mlp" in want:
            extras["pub_mlp"] = side_bench(lambda: pub_mlp_side_bench(torch, device, args.cpu_budget / 3))
        if "cnn" in want:
            extras["cnn"] = side_bench(cnn_side_bench)
        if "loader" in want:
            extras["loader"] = side_bench(loader_side_bench)
        if "stream" in want:
            extras["stream"] = side_bench(stream_side_bench)
        if "sweep" in want:
            # SURVEY 8(d) config (2) names B in {1024, 8192, 65536}: the other two sizes, after (and apart from) the headline's timed region
            extras["sweep"] = {str(b): side_bench(lambda b=b: sweep_point(torch, device, b, args.steps)) for b in (1024, 65536) if b != B}

    if rank == 0:
        out = {"metric": "training columns/sec", "value": round(value, 1), "unit": "columns/s",
               "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
               "config": {"workload": "cfg-MLP 124->5x512->128->(120||8) LeakyReLU(0.15), Adam(eps=1e-7) lr=1e-3, "
                                      "mse, synthetic low-res columns gathered from an HBM-resident split",
                          "init": "glorot_uniform kernels, zero biases, ReLU-head bias +%.2f (synthetic recipe only: keeps the 8 ReLU outputs alive, see synthetic_init)" % RELU_HEAD_BIAS,
                          "per_gpu_batch": B, "global_batch": B * world, "rows_resident_per_gpu": args.rows,
                          "parallelism": f"dp{world}", "params": n_params},
               "timing": {**timing, "value_from": "median block", "gpu_sclk_mhz": clk.summary()},
               "coop_timeouts": coop_timeouts,
               "comm": comm, "strong": strong, "weak_large": weak_large,
               "heldout": {"mse": held["mse"], "mae": held["mae"], "rows": 65536, "per_variable": per_var,
                           "against_cpu_restatement": acceptance},
               "predict": {"columns_per_s": round(predict_cps, 1), "rows": n_pred, "rows_per_call": predict_rows_per_call, "passes": "median of 3"},
               "roofline": roofline, "kernels": kernels, "kernels_note": kernels_note, "cpu_baseline": cpu, **extras}
        line = json.dumps(out, allow_nan=False)

    def flush_c_stdio():
        # RCCL writes a version banner through C stdio; on a pipe it would otherwise come out at exit, BEHIND the result
        import ctypes
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()

    if dist:
        torch.cuda.synchronize()
        dp.close()                       # the engine's own RCCL communicator goes first
        flush_c_stdio()                  # every rank empties its buffers before rank 0 prints
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        flush_c_stdio()
        print(line, flush=True)          # the JSON line is the last line of stdout


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--acceptance-cpu-worker":
        acceptance_cpu_worker(sys.argv[2])
        sys.exit(0)
    main()
