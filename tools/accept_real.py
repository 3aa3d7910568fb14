#!/usr/bin/env python3
"""Real-data acceptance (SURVEY 8(d) "MAE acceptance"): train the PUBLISHED configuration on the ClimSim low-res splits, score the
held-out split through the reference's evaluation weighting and print per-variable MAE / R2 / RMSE beside the published numbers.

    python tools/accept_real.py --data DIR [--model mlp|cnn] [--epochs N] [--out DIR] [--limit-rows N]

DIR holds the files `climsim_utils.data_utils.save_as_npy` writes (data_utils.py:906-925): {train,val,scoring}_input.npy (N,124) float32
(normalised) and {train,val,scoring}_target.npy (N,128) float32 (scaled).  The data set is not in this repository and not on the
build's machines: the script has never seen the real files - what it does with arrays of that shape is covered by
tests/test_accept_real_cpu.py (table logic, file checks) and by the engine's own tests (fit / predict / device metrics).

  mlp: 124 -> 768-640-512-640-640 -> 128 -> (120 linear || 8 relu), LeakyReLU(0.15), RAdam, batch 3072 - lot-147 / trial_0027,
       baseline_models/MLP/HPO/step1_results.csv:170, retrained by step2_retrain.py.  Schedule AS THE REFERENCE'S CODE RUNS IT
       (SURVEY appendix B): tfa CyclicalLearningRate(2.5e-4, 2.5e-3, step_size = 2 * (26280 // 3072) = 16, triangular2) - the
       amplitude halves every 32 steps, so from ~300 steps on the rate IS 2.5e-4.  Default 30 epochs = the 12 of the search run
       + the 18 of the retraining (step2_retrain.py:253-285 warm-starts from the search's checkpoint); best epoch by val_loss.
  cnn: depth 12, width 406, kernel 3, dropout 0.175, mae_adjusted, Adam with the cyclical schedule of hpo_train.py:204-213 (whose
       step_size = 2 * (10091520 // 12) makes it a slow ramp), batch 512, 15 epochs (baseline_models/CNN/training/hpo_train.py).

Output: the table on stdout, `<out>/{MLP,CNN}_preds.npy` (N,128) float32 in the scaled output space (what the reference's
main_figure_generation.ipynb loads), `<out>/accept_<model>.json`.  Exit code 0 when every published MAE is matched within
--tolerance (default 1 %: SURVEY 8(d) / BASELINE north_star), 1 otherwise.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

VARS = ("ptend_t", "ptend_q0001", "cam_out_NETSW", "cam_out_FLWDS", "cam_out_PRECSC", "cam_out_PRECC", "cam_out_SOLS", "cam_out_SOLL",
        "cam_out_SOLSD", "cam_out_SOLLD")
# website/evaluating.md:17-54 (W/m2; "--" = not reported)
PUBLISHED = {
    "mlp": {"MAE": (2.683, 4.495, 13.36, 5.224, 2.684, 34.33, 7.97, 10.30, 4.533, 4.806),
            "R2": (0.589, None, 0.983, 0.924, None, -38.69, 0.961, 0.948, 0.956, 0.866),
            "RMSE": (4.421, 7.322, 26.71, 6.969, 4.734, 72.88, 17.40, 21.95, 9.420, 10.12)},
    "cnn": {"MAE": (2.585, 4.401, 18.85, 8.598, 3.364, 37.83, 10.83, 13.15, 5.817, 5.679),
            "R2": (0.627, None, 0.944, 0.828, None, 0.077, 0.927, 0.916, 0.927, 0.813),
            "RMSE": (4.369, 7.284, 36.91, 10.86, 6.001, 85.31, 22.92, 27.25, 12.13, 12.10)},
}
# the MLP's MAE to full precision as the reference's own test notebook holds it (tests/unit_tests.ipynb, cells at nb:1338-1554)
PUBLISHED_MLP_MAE_EXACT = (2.6827649418146033, 4.494751601035413, 13.360914708055326, 5.22446795168065, 2.6839145034091993,
                           34.33306491959438, 7.970805061077366, 10.299178191838227, 4.533140962900527, 4.8063065724325)
SPLIT_ROWS = {"train": 10_091_520, "val": 1_441_920, "scoring": 1_681_920}       # hpo_train.py:358; quickstart_example.ipynb


def load_split(data_dir: str, split: str, limit_rows: int | None = None):
    """(input, target) of one split as read-only memory maps; shapes and dtypes checked against the on-disk contract."""
    out = []
    for kind, width in (("input", 124), ("target", 128)):
        path = os.path.join(data_dir, f"{split}_{kind}.npy")
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} not found: expected the files data_utils.save_as_npy writes ({split}_input.npy, {split}_target.npy)")
        a = np.load(path, mmap_mode="r")
        if a.ndim != 2 or a.shape[1] != width:
            raise ValueError(f"{path}: shape {a.shape}, expected (N, {width})")
        if a.dtype != np.float32:
            raise ValueError(f"{path}: dtype {a.dtype}, expected float32 (data_utils.py:906-925 casts before saving)")
        out.append(a)
    if out[0].shape[0] != out[1].shape[0]:
        raise ValueError(f"{split}: {out[0].shape[0]} input rows but {out[1].shape[0]} target rows")
    n = out[0].shape[0]
    if n % 384:
        raise ValueError(f"{split}: {n} rows is not a whole number of 384-column time steps")
    if limit_rows:
        n = min(n, (limit_rows // 384) * 384)
    return out[0][:n], out[1][:n]


def comparison_rows(df_var, model: str):
    """[{variable, metric, ours, published, rel_diff}] for every (variable, metric) the published table reports."""
    rows = []
    pub = PUBLISHED[model]
    for i, v in enumerate(VARS):
        for metric in ("MAE", "R2", "RMSE"):
            ours = float(df_var.loc[v, metric])
            p = pub[metric][i]
            rel = None if p is None or not math.isfinite(ours) else abs(ours - p) / max(abs(p), 1e-30)
            rows.append({"variable": v, "metric": metric, "ours": ours if math.isfinite(ours) else None, "published": p, "rel_diff": rel})
    return rows


def verdict(rows, tolerance: float):
    """The acceptance bar: every published MAE within `tolerance` (relative).  R2 and RMSE are printed, not gated (R2 of PRECC is -38.69
    in the published table: a ratio of small numbers; the north star names MAE)."""
    mae = [r for r in rows if r["metric"] == "MAE" and r["published"] is not None]
    worst = max(mae, key=lambda r: r["rel_diff"] if r["rel_diff"] is not None else math.inf)
    ok = all(r["rel_diff"] is not None and r["rel_diff"] <= tolerance for r in mae)
    return {"passed": bool(ok), "tolerance": tolerance, "worst_variable": worst["variable"],
            "worst_rel_diff": worst["rel_diff"], "n_checked": len(mae)}


def format_table(rows, model: str) -> str:
    lines = [f"{'variable':<16}" + "".join(f"{m + ' ours':>12}{m + ' publ.':>12}{'diff %':>8}" for m in ("MAE", "R2", "RMSE"))]
    for v in VARS:
        cells = [f"{v:<16}"]
        for m in ("MAE", "R2", "RMSE"):
            r = next(x for x in rows if x["variable"] == v and x["metric"] == m)
            ours = "--" if r["ours"] is None else f"{r['ours']:.4g}"
            pub = "--" if r["published"] is None else f"{r['published']:.4g}"
            rel = "" if r["rel_diff"] is None else f"{100 * r['rel_diff']:.2f}"
            cells.append(f"{ours:>12}{pub:>12}{rel:>8}")
        lines.append("".join(cells))
    lines.append(f"(published: website/evaluating.md:17-54, column {model.upper()}; W/m2, energy-weighted as data_utils.output_weighting)")
    return "\n".join(lines)


def make_data_utils():
    """The reference's evaluation constants: the committed low-res grid and normalisation bundles (tests/golden/, extracted from the
    reference's own .nc assets by tests/golden/make_golden.py)."""
    from climsim_amd.assets import load_grid_info, load_npz_assets
    from climsim_amd.data_utils import data_utils
    gold = os.path.join(REPO, "tests", "golden")
    grid = load_grid_info(os.path.join(gold, "grid_lowres.npz"))
    sets = [load_npz_assets(os.path.join(gold, "norm_lowres.npz"), k) for k in ("input_mean", "input_max", "input_min", "output_scale")]
    du = data_utils(grid, *sets)
    du.set_to_v1_vars()
    return du


def train_and_score(args):
    import torch
    from climsim_amd import build
    build.build()
    from climsim_amd.metrics import GpuMetrics
    dev = torch.device("cuda", 0)
    xt, yt = load_split(args.data, "train", args.limit_rows)
    xv, yv = load_split(args.data, "val", args.limit_rows)
    xs, ys = load_split(args.data, "scoring", args.limit_rows)
    for name, a in (("train", xt), ("val", xv), ("scoring", xs)):
        if not args.limit_rows and a.shape[0] != SPLIT_ROWS[name]:
            print(f"note: {name} split has {a.shape[0]} rows, the published splits have {SPLIT_ROWS[name]}", file=sys.stderr)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731  (the train split is 10.2 GB: resident in HBM)
    xt_d, yt_d, xv_d, yv_d, xs_d, ys_d = (to_dev(a) for a in (xt, yt, xv, yv, xs, ys))
    os.makedirs(args.out, exist_ok=True)
    best = os.path.join(args.out, f"accept_{args.model}_best.npz")
    if args.model == "mlp":
        from climsim_amd.mlp import CyclicalLearningRate, MLPEmulator
        epochs = args.epochs or 30
        m = MLPEmulator(units=(768, 640, 512, 640, 640), activation="leakyrelu", optimizer="RAdam", max_batch=3072, seed=args.seed,
                        precision=getattr(args, "precision", "bf16"))
        hist = m.fit(xt_d, yt_d, batch_size=3072, epochs=epochs, validation_data=(xv_d, yv_d),
                     learning_rate=CyclicalLearningRate(2.5e-4, 2.5e-3, step_size=2 * (26280 // 3072)), seed=args.seed,
                     checkpoint_best=best, early_stopping_patience=8, csv_log=os.path.join(args.out, "accept_mlp_log.csv"), verbose=1)
        m.load_weights(best)
        preds = m.predict(xs_d, as_numpy=False)
    else:
        from climsim_amd.cnn import CNNEmulator
        epochs = args.epochs or 15
        m = CNNEmulator(depth=12, channel_width=406, max_batch=512, trainable=True, loss="mae", dropout=0.175, init_seed=args.seed, seed=args.seed)
        hist = m.fit(xt_d, yt_d, batch_size=512, epochs=epochs, validation_data=(xv_d, yv_d), seed=args.seed,
                     checkpoint=os.path.join(args.out, "accept_cnn_{epoch}.npz"), early_stopping_patience=10, verbose=1)
        monitor = hist.get("val_loss") or hist["loss"]
        m.load_weights(os.path.join(args.out, f"accept_cnn_{int(np.argmin(monitor)) + 1}.npz"))        # best epoch by val_loss
        preds = m.predict(xs_d, flat_output=True, as_numpy=False)
    np.save(os.path.join(args.out, f"{args.model.upper()}_preds.npy"), preds.cpu().numpy().astype(np.float32))
    df_var, _ = GpuMetrics(make_data_utils()).metrics_tables(preds, ys_d, xs_d)
    m.close()
    return df_var, hist


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--data", required=True, help="directory with {train,val,scoring}_{input,target}.npy")
    ap.add_argument("--model", choices=("mlp", "cnn"), default="mlp")
    ap.add_argument("--epochs", type=int, default=0, help="default: 30 (mlp), 15 (cnn)")
    ap.add_argument("--out", default="accept_out")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--tolerance", type=float, default=0.01, help="relative MAE tolerance of the verdict (1 %%)")
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16",
                    help="MLP arithmetic: bf16 operands (default) or the reference's float32 (CS_FLAG_FP32)")
    ap.add_argument("--limit-rows", type=int, default=0, help="development: use only the first N rows of every split")
    args = ap.parse_args(argv)
    df_var, hist = train_and_score(args)
    rows = comparison_rows(df_var, args.model)
    v = verdict(rows, args.tolerance)
    print(format_table(rows, args.model))
    print(f"verdict: {'PASS' if v['passed'] else 'FAIL'} - worst MAE difference {100 * (v['worst_rel_diff'] or float('nan')):.2f} % ({v['worst_variable']}), bar {100 * v['tolerance']:.1f} %")
    with open(os.path.join(args.out, f"accept_{args.model}.json"), "w") as f:
        json.dump({"model": args.model, "precision": args.precision, "rows": rows, "verdict": v, "history": {k: [float(x) for x in vals] for k, vals in hist.items()}}, f, indent=1)
    return 0 if v["passed"] else 1


if __name__ == "__main__":
    sys.exit(main())
