"""Training-step time of the float32 mode (CS_FLAG_FP32) beside the default bf16 engine: the cfg-MLP at batch 8192 and the published
768-640-512-640-640 model at 3072.  One JSON line per case and precision: step time from device events over back-to-back steps
(warm-up first, a synchronisation on both sides of the timed block), columns/s, the step's FLOP (oracle MLPConfig.train_flops) and
the share of the f32-input MFMA peak (157.3 TF) they represent, plus the per-kernel-kind times of a profiled block.
`python tools/fp32_step_time.py [--steps 200] [--warmup 20]`."""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from climsim_amd import _lib  # noqa: E402
from climsim_amd.mlp import MLPEmulator  # noqa: E402
from oracle.mlp_oracle import MLPConfig  # noqa: E402

F32_PEAK_TF = 157.3            # 256 CUs x 4 SIMDs x 64 FLOP/clk x 2.4 GHz
CASES = {"cfg_mlp_b8192": ((512,) * 5, 8192), "pub_mlp_b3072": ((768, 640, 512, 640, 640), 3072)}


def time_case(units, batch, precision, steps, warmup):
    m = MLPEmulator(units=units, activation="relu", optimizer="AdamTorch", epsilon=1e-8, max_batch=batch, seed=0, precision=precision)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(batch, 124, device="cuda", generator=g) * 0.2
    y = torch.randn(batch, 128, device="cuda", generator=g) * 0.05
    for _ in range(warmup):
        m.train_on_batch(x, y, 1e-4)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        m.train_on_batch(x, y, 1e-4)
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / steps
    with _lib.profile_session(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) as prof:
        for _ in range(20):
            m.train_on_batch(x, y, 1e-4)
    kinds = {k: round(v[0] / 20 * 1e3, 1) for k, v in prof.times.items() if v[1]}
    m.close()
    return ms, kinds


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args(argv)
    for name, (units, batch) in CASES.items():
        flop = MLPConfig(hidden=units).train_flops() * batch
        for precision in ("bf16", "fp32"):
            ms, kinds = time_case(units, batch, precision, args.steps, args.warmup)
            print(json.dumps({"case": name, "precision": precision, "batch": batch, "step_ms": round(ms, 4),
                              "columns_per_s": round(batch / (ms * 1e-3)), "gflop_per_step": round(flop / 1e9, 2),
                              "f32_peak_share": round(flop / (ms * 1e-3) / (F32_PEAK_TF * 1e12), 3), "kernel_us": kinds}), flush=True)


if __name__ == "__main__":
    main()
