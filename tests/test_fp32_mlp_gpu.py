"""The float32 arithmetic mode (CS_FLAG_FP32, `precision="fp32"`, csrc/gemm_f32.h) against float32 references.

The bf16 engine can only be held to the reference's vectors at bf16-operand bars (2-25 %, tests/test_hot_mlp_gpu.py); in float32
mode the same vectors and the float32 oracles (`bf16=False`) hold it at accumulation-order bars:
  - reference vectors (tests/golden/hot_mlp_golden.npz): predictions 1e-5 of the largest, loss / mae 1e-5, gradient summaries and
    five-step movements at tests/test_hot_mlp_cpu.py's bars times 3 (a blocked MFMA chain sums in another order than numpy; the
    ReLU-kink rows already need LOOSE there),
  - Keras rules, online-MLP losses and pruning, ragged batches against oracle/mlp_oracle.py and oracle/online_mlp_oracle.py at
    bf16=False,
  - determinism (no atomics on the gradient path), the launches of a step, the modes the float32 path refuses, and the
    equal-steps acceptance of SURVEY 8(d) against oracle/mlp_torch_cpu.TorchMLP(bf16=False)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import mlp_oracle as O  # noqa: E402
from oracle import online_mlp_oracle as OO  # noqa: E402
from online_mlp_inputs import CASES, HOT_CASES, LR, batches, hot_batches, hot_init_state, hot_pred_rows, init_state  # noqa: E402
from test_hot_mlp_cpu import LOOSE, cfg_of, keras_list, state_dict, summary_errors  # noqa: E402

HOT = np.load(os.path.join(os.path.dirname(__file__), "golden", "hot_mlp_golden.npz"))
ONLINE = np.load(os.path.join(os.path.dirname(__file__), "golden", "online_mlp_golden.npz"))
WIDEN = 3.0


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from climsim_amd import build
    build.build()
    from climsim_amd import _lib, mlp
    return mlp, _lib


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / (np.linalg.norm(np.asarray(b, np.float64)) + 1e-30))


def make_hot(M, name, precision="fp32"):
    n_in, n_out, hidden, loss, nb = HOT_CASES[name]
    m = M[0].MLPEmulator(units=tuple(hidden[:-1]), activation="relu", optimizer="AdamTorch", epsilon=1e-8, max_batch=nb, seed=None,
                         precision=precision)
    m.set_weights(keras_list(hot_init_state(name), len(hidden)))
    return m


@pytest.mark.parametrize("name", list(HOT_CASES))
def test_reference_vectors_at_float32_bars(M, name):
    from conftest import record_margin
    n_in, n_out, hidden, loss, nb = HOT_CASES[name]
    m = make_hot(M, name)
    assert m.precision == "fp32"
    x, y = hot_batches(name)[0]
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    pred = m.predict(xd, as_numpy=False).cpu().numpy()
    rows, amax = hot_pred_rows(name), float(HOT[f"{name}/pred_absmax"])
    e_pred = float(np.abs(pred[rows] - HOT[f"{name}/pred_rows"]).max() / amax)
    record_margin(f"fp32_hot_{name}_pred_vs_reference_max", e_pred)
    assert e_pred <= 1e-5, e_pred
    sums = m.loss_grads(xd, yd).cpu().numpy().astype(np.float64) / (128 * nb)
    for i, key in enumerate(("loss", "mae")):
        e = abs(sums[i] - float(HOT[f"{name}/{key}"])) / float(HOT[f"{name}/{key}"])
        record_margin(f"fp32_hot_{name}_{key}_vs_reference_rel", e)
        assert e <= 1e-5, (key, e)
    g = state_dict(m.get_gradients(1.0 / (128 * nb)), len(hidden))
    for li in range(len(hidden) + 1):
        key = f"linears.{li}.0" if li < len(hidden) else "final_linear"
        errs = summary_errors(name, f"{name}/grad", key + ".weight", g[key + ".weight"])
        rb = HOT[f"{name}/grad/{key}.bias"]
        errs["bias"] = float(np.abs(g[key + ".bias"] - rb).max() / np.abs(rb).max())
        for f, e in errs.items():
            record_margin(f"fp32_hot_{name}_grad_{f}_vs_reference", e)
            assert e <= WIDEN * LOOSE[f], (key, f, e)
    # five steps of the reference's optimiser, one-call steps (row splits stored and added by the optimiser)
    m2 = make_hot(M, name)
    init = hot_init_state(name)
    losses = [float(m2.train_on_batch(torch.from_numpy(bx).cuda(), torch.from_numpy(by).cuda(), LR).cpu().numpy()[0]) / (128 * nb)
              for bx, by in hot_batches(name)]
    e_losses = float(np.max(np.abs(np.array(losses) - HOT[f"{name}/losses"]) / HOT[f"{name}/losses"]))
    record_margin(f"fp32_hot_{name}_losses_vs_reference_rel", e_losses)
    assert e_losses <= WIDEN * 2e-5, e_losses                         # test_hot_mlp_cpu: rtol 2e-5
    sd = state_dict(m2.get_weights(), len(hidden))
    for k, v in sd.items():
        if k.endswith("bias"):
            mv, rmv = v - init[k], HOT[f"{name}/after5/{k}"] - init[k]
            record_margin(f"fp32_hot_{name}_bias_movement_vs_reference_rel", rel(mv, rmv))
            assert rel(mv, rmv) <= WIDEN * 1e-3, (k, rel(mv, rmv))
        else:
            errs = summary_errors(name, f"{name}/moved5", k, v.astype(np.float64) - init[k])
            for f, e in errs.items():
                record_margin(f"fp32_hot_{name}_movement_{f}_vs_reference", e)
            assert errs["fro"] <= WIDEN * 2e-5 and errs["proj"] <= WIDEN * 5e-3 and errs["entry"] <= WIDEN * 2e-2, (k, errs)
    m.close()
    m2.close()


@pytest.mark.parametrize("name", list(HOT_CASES))
def test_it_is_the_float32_path(M, name):
    """A step is L forward GEMMs, L-1 data-gradient GEMMs, one weight-gradient and one optimiser launch (plus the input staging) -
    no chain kernel; and the default bf16 engine misses the float32 prediction bar by more than 10x on the same case."""
    from climsim_amd.group import kernel_family
    n_in, n_out, hidden, loss, nb = HOT_CASES[name]
    L = len(hidden) + 1
    x, y = hot_batches(name)[0]
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    m = make_hot(M, name)
    assert kernel_family(m) == 32
    kt = m.profile_step(xd, yd, LR)
    launched = {k: v[1] for k, v in kt.items() if v[1]}
    assert launched == {"prepare_input": 1, "gemm_fwd": L, "gemm_dgrad": L - 1, "wgrad": 1, "optimizer": 1}, launched
    b = make_hot(M, name, precision="bf16")
    rows, amax = hot_pred_rows(name), float(HOT[f"{name}/pred_absmax"])
    e_bf16 = float(np.abs(b.predict(xd, as_numpy=False).cpu().numpy()[rows] - HOT[f"{name}/pred_rows"]).max() / amax)
    assert e_bf16 > 10 * 1e-5, e_bf16
    m.close()
    b.close()


KERAS_SHAPES = {
    "v1": dict(n_in=124, hidden=(256, 384), n_out_lin=120, n_out_relu=8),
    "v2": dict(n_in=425, hidden=(384, 640), n_out_lin=360, n_out_relu=8),
}


@pytest.mark.parametrize("shape", list(KERAS_SHAPES))
@pytest.mark.parametrize("opt", ["Adam", "RAdam", "RMSprop", "SGD"])
@pytest.mark.parametrize("act", ["leakyrelu", "elu"])
def test_keras_rules_one_step(M, act, opt, shape):
    from conftest import record_margin
    s = KERAS_SHAPES[shape]
    cfg = O.MLPConfig(n_in=s["n_in"], hidden=s["hidden"], n_out_lin=s["n_out_lin"], n_out_relu=s["n_out_relu"], act=act)
    ws = O.glorot_init(cfg, 5)
    n = 600
    x, y = O.synth_columns(n, seed=11, n_in=cfg.n_in, n_out=cfg.n_out)
    m = M[0].MLPEmulator(units=cfg.hidden, activation=act, optimizer=opt, input_length=cfg.n_in, output_length_lin=cfg.n_out_lin,
                         output_length_relu=cfg.n_out_relu, max_batch=1024, seed=None, precision="fp32")
    m.set_weights(ws)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    pred = m.predict(xd)
    ref_pred = O.forward(ws, x, cfg, bf16=False)
    assert rel(pred, ref_pred) <= 1e-5, rel(pred, ref_pred)
    m.loss_grads(xd, yd)
    _, _, og, _ = O.loss_and_grads(ws, x, y, cfg, bf16=False)
    for i, (g, r) in enumerate(zip(m.get_gradients(1.0 / (cfg.n_out * n)), og)):
        record_margin("fp32_keras_grad_rel", rel(g, r))
        assert rel(g, r) <= 1e-5, (i, rel(g, r))
    m.apply_gradients(1e-3, 1.0 / (cfg.n_out * n))
    ows, _, _ = O.train_step(ws, O.Optimizer(kind=opt), x, y, cfg, 1e-3, bf16=False)
    for i, (w, r) in enumerate(zip(m.get_weights(), ows)):
        record_margin("fp32_keras_weights_after_step_rel", rel(w, r))
        assert rel(w, r) <= 1e-5, (i, rel(w, r))
    m.close()


@pytest.mark.parametrize("name", list(CASES))
def test_online_mlp_float32(M, name):
    """mse / mae / huber and output pruning against the reference's vectors: predictions and losses at 1e-5, gradients 1e-4 in norm,
    five steps' losses 1e-4.  mae and huber take sign-like gradients (sign(e), clamp(e)) where a rounding-level error could flip an
    entry; in float32 none does on these cases (measured 1e-6 in norm for all three losses), so they keep the mse bar."""
    from climsim_amd import online_mlp
    from conftest import record_margin
    n_in, n_out, hidden, prune, lev, loss, nb = CASES[name]
    m = online_mlp.MLP(n_in, n_out, hidden, len(hidden), output_prune=prune, strato_lev_out=lev, loss=loss, max_batch=256, seed=None,
                       precision="fp32")
    m.load_state_dict(init_state(name))
    x, y = batches(name)[0]
    pred = m.forward(x, as_numpy=True)
    gp = ONLINE[f"{name}/pred"]
    e = float(np.abs(pred - gp).max() / np.abs(gp).max())
    record_margin(f"fp32_online_{name}_pred_vs_reference_max", e)
    assert e <= 1e-5, e
    if prune:
        assert not pred[:, 60:60 + lev].any() and not pred[:, 240:240 + lev].any()
    lv = m.loss_grads(x, y)
    e = abs(lv - float(ONLINE[f"{name}/loss"])) / float(ONLINE[f"{name}/loss"])
    record_margin(f"fp32_online_{name}_loss_vs_reference_rel", e)
    assert e <= 1e-5, e
    g = m.gradients()
    bar = 1e-4
    for k in g:
        r = rel(g[k], ONLINE[f"{name}/grad/{k}"])
        record_margin(f"fp32_online_{name}_grad_vs_reference_rel", r)
        assert r <= bar, (k, r)
    losses = [m.train_step(bx, by, LR) for bx, by in batches(name)]
    e = float(np.max(np.abs(np.array(losses) - ONLINE[f"{name}/losses"]) / ONLINE[f"{name}/losses"]))
    record_margin(f"fp32_online_{name}_losses_vs_reference_rel", e)
    assert e <= 1e-4, e
    m.engine.close()


def test_online_mlp_float32_refuses_dropout(M):
    from climsim_amd import online_mlp
    with pytest.raises(ValueError, match="dropout"):
        online_mlp.MLP(124, 128, 128, 2, dropout=0.1, precision="fp32", max_batch=128)


RAGGED = [1, 127, 129, 3071, 8191, 8192]


def test_ragged_batches(M):
    """Every batch size against the float32 oracle on exactly its rows, gathered through row_idx from a staging buffer with NaN in
    every other row, with a canary behind row n of the prediction: a row dropped, doubled or read from the wrong place moves the
    loss of n rows by ~1/n (1.2e-4 at 8191) - the bars are 1e-5; prediction past max_batch in several chunks."""
    from conftest import record_margin
    mlp, _lib = M
    cfg = O.MLPConfig(hidden=(512, 512, 256), act="leakyrelu")
    ws = O.glorot_init(cfg, 3)
    xa, ya = O.synth_columns(3 * 8192 + 17, seed=7)
    m = mlp.MLPEmulator(units=cfg.hidden, optimizer="Adam", max_batch=8192, seed=None, precision="fp32")
    m.set_weights(ws)
    assert m.lib.cs_mlp_forward_limit(m._h) == 8192
    for n in RAGGED:
        x, y = xa[:n], ya[:n]
        rows = n + 300
        where = np.random.default_rng(n).permutation(rows)
        xs = np.full((rows, 124), np.nan, np.float32)
        ys = np.full((rows, 128), np.nan, np.float32)
        xs[where[:n]], ys[where[:n]] = x, y
        xd, yd, idx = torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda(), torch.from_numpy(where.astype(np.int64)).cuda()
        ol, omae, og, op = O.loss_and_grads(ws, x, y, cfg, bf16=False)
        yh = torch.full((rows, 128), 12345.0, device="cuda")
        m.forward_batch(xd, yhat=yh, row_idx=idx, n=n)
        out = yh.cpu().numpy()
        assert np.all(out[n:] == 12345.0), n
        e = float(np.abs(out[:n] - op).max() / np.abs(op).max())
        record_margin("fp32_ragged_pred_max", e)
        assert e <= 1e-5, (n, e)
        sums = m.loss_grads(xd, yd, row_idx=idx, n=n).cpu().numpy().astype(np.float64) / (128 * n)
        assert abs(sums[0] - ol) <= 1e-5 * ol and abs(sums[1] - omae) <= 1e-5 * omae, (n, sums, ol, omae)
        for g, r in zip(m.get_gradients(1.0 / (128 * n)), og):
            record_margin("fp32_ragged_grad_rel", rel(g, r))
            assert rel(g, r) <= 1e-5, (n, rel(g, r))
    # prediction beyond max_batch: MLPEmulator.predict chunks by cs_mlp_forward_limit
    pred = m.predict(torch.from_numpy(xa).cuda(), as_numpy=True)
    ref = O.forward(ws, xa, cfg, bf16=False)
    assert pred.shape == ref.shape and float(np.abs(pred - ref).max() / np.abs(ref).max()) <= 1e-5
    m.close()


def test_two_handles_are_bit_identical(M):
    name = "cfg_mlp_b8192"
    ms = [make_hot(M, name) for _ in range(2)]
    for bx, by in hot_batches(name):
        xd, yd = torch.from_numpy(bx).cuda(), torch.from_numpy(by).cuda()
        for m in ms:
            m.train_on_batch(xd, yd, LR)
    a, b = ms
    for u, v in zip(a.get_weights(), b.get_weights()):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    for su, sv in zip(a.get_optimizer_state()[:2], b.get_optimizer_state()[:2]):
        for u, v in zip(su, sv):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    for m in ms:
        m.close()


def test_refusals_leave_the_model_usable(M):
    mlp, _lib = M
    from climsim_amd.group import MLPGroup
    with pytest.raises(ValueError, match="cooperative"):
        mlp.MLPEmulator(units=(128, 128), max_batch=256, precision="fp32", cooperative=True)
    with pytest.raises(_lib.EngineError):
        mlp.MLPEmulator(units=(128, 128), max_batch=256, precision="fp32", flags=_lib.CS_FLAG_COOP)
    with pytest.raises(ValueError, match="precision"):
        mlp.MLPEmulator(units=(128, 128), max_batch=256, precision="fp16")
    m = mlp.MLPEmulator(units=(128, 128), max_batch=256, precision="fp32", seed=1)
    x, y = O.synth_columns(200, seed=3)
    before = m.predict(x)
    with pytest.raises(_lib.EngineError, match="FP32"):
        m.set_dropout(0.1)
    with pytest.raises(_lib.EngineError, match="FP32"):
        MLPGroup([m])
    other = mlp.MLPEmulator(units=(128, 128), max_batch=256, seed=1)
    with pytest.raises(_lib.EngineError):
        MLPGroup([other, m])
    assert np.array_equal(m.predict(x), before)
    l0 = float(m.train_on_batch(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 1e-3)[0])
    for _ in range(5):
        l1 = float(m.train_on_batch(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 1e-3)[0])
    assert np.isfinite(l1) and l1 < l0
    other.close()
    m.close()


def test_checkpoint_crosses_precisions(M, tmp_path):
    mlp, _ = M
    a = mlp.MLPEmulator(units=(256, 256), max_batch=512, seed=2, precision="fp32")
    x, y = O.synth_columns(400, seed=4)
    a.train_on_batch(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 1e-3)
    p = str(tmp_path / "w.npz")
    a.save_weights(p)
    b = mlp.MLPEmulator(units=(256, 256), max_batch=512, seed=None)
    b.load_weights(p)
    for u, v in zip(a.get_weights(), b.get_weights()):
        assert np.array_equal(u, v)
    c = mlp.MLPEmulator(units=(256, 256), max_batch=512, seed=None, precision="fp32")
    c.load_weights(p)
    assert np.array_equal(c.predict(x), a.predict(x))
    for m in (a, b, c):
        m.close()


ACCEPT_STEPS, ACCEPT_BATCH = 100, 1024


def test_equal_steps_acceptance_against_float32_cpu(M):
    """SURVEY 8(d) 'fp32 mode 1e-4 rel': the float32 engine and TorchMLP(bf16=False) (float32 torch on the CPU) train the cfg-MLP
    from the same weights on the same synthetic batches with Keras Adam; the held-out all-output MAE agrees within 1e-4 relative.
    Per-variable agreement (the 128 output columns) is recorded, not gated: columns whose error is near zero reorder freely."""
    from conftest import record_margin
    from oracle.mlp_torch_cpu import TorchMLP
    mlp, _ = M
    cfg = O.MLPConfig(act="leakyrelu")
    ws = O.glorot_init(cfg, 9)
    x, y = O.synth_columns(ACCEPT_STEPS * ACCEPT_BATCH + 4096, seed=21)
    xv, yv = x[-4096:], y[-4096:]
    m = mlp.MLPEmulator(units=cfg.hidden, optimizer="Adam", max_batch=ACCEPT_BATCH, seed=None, precision="fp32")
    m.set_weights(ws)
    t = TorchMLP(ws, cfg, bf16=False)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for s in range(ACCEPT_STEPS):
        lo = s * ACCEPT_BATCH
        m.train_on_batch(xd[lo:lo + ACCEPT_BATCH], yd[lo:lo + ACCEPT_BATCH], 1e-3)
        t.train_step(torch.from_numpy(x[lo:lo + ACCEPT_BATCH]), torch.from_numpy(y[lo:lo + ACCEPT_BATCH]), 1e-3)
    pe = m.predict(xv)
    with torch.no_grad():
        pt = t.forward(torch.from_numpy(xv)).numpy()
    mae_e, mae_t = float(np.abs(pe - yv).mean()), float(np.abs(pt - yv).mean())
    d = abs(mae_e - mae_t) / mae_t
    per_var = np.abs(np.abs(pe - yv).mean(0) - np.abs(pt - yv).mean(0)) / (np.abs(pt - yv).mean(0) + 1e-30)
    record_margin("fp32_accept_all_output_mae_rel", d)
    record_margin("fp32_accept_per_variable_mae_rel_max", float(per_var.max()))
    record_margin("fp32_accept_per_variable_mae_rel_median", float(np.median(per_var)))
    assert d <= 1e-4, (mae_e, mae_t, d)
    m.close()
