"""MLP kernels at ragged and changing batch sizes, row by row.

The engine picks its kernels by batch size, and every pick has its own code for the last, partly empty row tile and the ends of
the weight-gradient row splits.  Each case here holds one batch to the oracle ROW BY ROW: sentinel rows (oracle/ragged.py) sit at
row 0, row n-1, both sides of the last two tile boundaries and both sides of every row-split boundary of the launch in use; each
carries a target offset on a linear-head column of its own and so dominates that column's bias gradient and weight-gradient
column.  A sentinel dropped, doubled or gathered from the wrong row moves those by 100 % of its contribution; the bar is 1 %.
Every call goes through `n=` and `row_idx` on buffers of round_up(n, 256) + 256 rows: the logical rows sit scattered in storage,
every other row holds NaN, the `row_idx` entries past n point at NaN rows (in bounds), and prediction rows past n hold a canary.
Nothing is normalised (the in-kernel inf/nan -> 0 rule would hide an over-read).

Default dispatch of the cfg-MLP (124 -> 5 x 512 -> 128) on 256 CUs, restated in oracle/ragged.py:dispatch from chain_bm_of and
run_backward (73 weight-gradient tiles of 128 x 128, 21 of 256 x 256) and asserted there (tests/test_ragged_rows_cpu.py):

    n              tile   weight gradient            splits   training step     why it is here
    1, 33, 1023     32    k_wgrad3<4,64>             2        stored splits     tiny / one-row last tile
    2049, 8191      32    k_wgrad3<4,64>             3        stored splits     split count steps
    8193, 11263     64    k_wgrad3<4,64>             3        stored splits     32 -> 64-row tiles
    11265, 16383    64    k_wgrad3<4,32>             6        atomics           two workgroups per CU (73 x 6 > 256)
    16385, 22527   128    k_wgrad3<4,32>             6        atomics           64 -> 128-row tiles
    22529          128    k_wgrad2l                  12       atomics           256 x 256 tiles (n >= 22528)
    32769           64    k_wgrad2l                  12       atomics           back to 64-row tiles
    published widths 3071, 3073: k_chainw_fb (32-row tiles), k_wgrad3<4,64>, 2 splits; 16385: k_wgrad3<4,32>, 4 splits

profile_session tells kernel KINDS apart (one chain_fb launch, one wgrad launch; per-layer GEMMs; split chains), not template
arguments: the tile height and the weight-gradient kernel are what the table says because the CPU test holds the restatement.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import mlp_oracle as O  # noqa: E402
from oracle import ragged as R  # noqa: E402
from conftest import record_margin  # noqa: E402

CFG, PUB = R.CFG, R.PUB
CANARY = np.float32(-12345.5)
BASE_ROWS = 33024
DEFAULT_NS = [1, 33, 1023, 2049, 8191, 8193, 11263, 11265, 16383, 16385, 22527, 22529, 32769]


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from climsim_amd import build
    build.build()
    from climsim_amd import _lib, group, mlp
    return mlp, group, _lib


def weights(units, seed):
    cfg = O.MLPConfig(hidden=tuple(units))
    ws = O.glorot_init(cfg, seed)
    rng = np.random.default_rng(seed + 100)
    for i in range(1, len(ws), 2):
        ws[i] = rng.normal(0, 0.05, ws[i].shape).astype(np.float32)
    return cfg, ws


class Model:
    """One set of weights, the shared base rows, the cached oracle blocks and the sentinels."""

    def __init__(self, units, seed, base, rows):
        self.units = units
        self.cfg, self.ws = weights(units, seed)
        self.bx, self.by = base
        self.blocks = O.RowBlockOracle(self.ws, self.bx, self.by, self.cfg)
        self.sent = R.Sentinels(self.ws, self.cfg, self.blocks.leading(rows))      # (the quietest head columns at the largest batch)

    def batch(self, n, pos):
        k = len(pos)
        x, y = self.sent.batch(self.bx[:n - k], self.by[:n - k], pos)
        return x, y, self.sent.expected(self.blocks.leading(n - k), k)


@pytest.fixture(scope="module")
def base():
    return O.synth_columns(BASE_ROWS, seed=7)


@pytest.fixture(scope="module")
def cfg_model(base):
    return Model(CFG, 3, base, 32768)


@pytest.fixture(scope="module")
def pub_model(base):
    return Model(PUB, 4, base, 16384)


def stage(x, y, seed):
    """Device buffers of round_up(n, 256) + 256 rows: logical row i in storage row where[i], NaN everywhere else; row_idx entries
    past n name NaN rows."""
    n = x.shape[0]
    rows = R.round_up(n, 256) + 256
    where = np.random.default_rng(seed).permutation(rows)
    xs = np.full((rows, x.shape[1]), np.nan, np.float32)
    ys = np.full((rows, y.shape[1]), np.nan, np.float32)
    xs[where[:n]], ys[where[:n]] = x, y
    return (torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda(), torch.from_numpy(where.astype(np.int64)).cuda(), rows)


def in_ref_order(a, n, pos):
    """Rows of a logical batch in the oracle's order: the base rows, then the sentinels."""
    is_s = np.zeros(n, bool)
    is_s[pos] = True
    return np.concatenate([a[:n][~is_s], a[:n][pos]])


def loss_and_grads(m, d, n):
    loss = m.loss_grads(d[0], d[1], row_idx=d[2], n=n).cpu().numpy().astype(np.float64)
    return loss, m.get_gradients(1.0)


def step_grads(m, m_before, n):
    """The unscaled gradients of the Adam step just taken, from the first moments before / after it (m += (g s - m)(1 - b1),
    s = 1/(128 n))."""
    omb1, s = np.float32(1 - 0.9), np.float32(1.0 / (128.0 * n))
    after = m.get_optimizer_state()[0]
    return [(a.astype(np.float64) + (b.astype(np.float64) - a) / float(omb1)) / float(s) for a, b in zip(m_before, after)]


def check_predictions(m, d, n, pos, ref, tag):
    yh = torch.full((d[3], 128), float(CANARY), device="cuda")
    m.forward_batch(d[0], yhat=yh, row_idx=d[2], n=n)
    out = yh.cpu().numpy()
    assert np.all(out[n:] == CANARY), (tag, "prediction rows past n were written")
    pred = in_ref_order(out, n, pos)
    assert np.all(np.isfinite(pred)), (tag, "non-finite prediction")
    assert R.rel(pred, ref.yhat) <= 1e-3, (tag, R.rel(pred, ref.yhat))
    assert np.max(np.abs(pred - ref.yhat)) <= 6e-3 * np.max(np.abs(ref.yhat)), tag


def kinds(times):
    return {k: v[1] for k, v in times.items() if v[1]}


def run_case(M, model, n, d, flags=0, cooperative=False, expect=None, tag=""):
    """One fresh handle at n: loss_grads (two-call form) and a one-call Adam step, both against the oracle row by row, the
    forward pass against the oracle's predictions with a canary behind row n."""
    mlp, _, _lib = M
    pos = R.sentinel_positions(n, d)
    k = len(pos)
    x, y, ref = model.batch(n, pos)
    assert R.calibration(ref, model.sent, k) >= 0.3, (tag, n)
    dev = stage(x, y, seed=n)
    m = mlp.MLPEmulator(units=model.units, optimizer="Adam", max_batch=max(n, 128), seed=None, flags=flags, cooperative=cooperative)
    m.set_weights(model.ws)
    stream = __import__("ctypes").c_void_p(torch.cuda.current_stream().cuda_stream)
    with _lib.profile_session(stream) as p:
        loss, g = loss_and_grads(m, dev, n)
    if expect is not None:
        got = kinds(p.times)
        got.pop("memset", None)
        assert got == expect, (tag, n, got)
    worst = R.check(loss[0], loss[1], g, ref, model.sent, k, tag=f"{tag} n={n} loss_grads")
    check_predictions(m, dev, n, pos, ref, f"{tag} n={n}")
    m0 = m.get_optimizer_state()[0]
    loss = m.train_on_batch(dev[0], dev[1], 1e-3, row_idx=dev[2], n=n).cpu().numpy().astype(np.float64)
    worst = max(worst, R.check(loss[0], loss[1], step_grads(m, m0, n), ref, model.sent, k, tag=f"{tag} n={n} train_on_batch"))
    m.close()
    record_margin("ragged_sentinel_share_of_bar", worst)
    return worst


def _fb():
    return {"chain_fb": 1, "wgrad": 1}


@pytest.mark.parametrize("n", DEFAULT_NS)
def test_default_dispatch_at_every_boundary(M, cfg_model, n):
    run_case(M, cfg_model, n, R.dispatch(n), expect=_fb(), tag="default")


@pytest.mark.parametrize("n", [3071, 3073, 16385])
def test_published_widths(M, pub_model, n):
    run_case(M, pub_model, n, R.dispatch(n, PUB), expect=_fb(), tag="published")


def _flag(M, name):
    return getattr(M[2], name)


@pytest.mark.parametrize("n", [8193, 2500])
@pytest.mark.parametrize("variant", ["bm32", "bm64", "bm128", "no_chain", "no_chain_fb", "wgrad2", "splitk5", "splitk7"])
def test_forced_variants(M, cfg_model, monkeypatch, n, variant):
    L = len(CFG) + 2
    flags, env, kw, expect = 0, {}, {}, _fb()
    if variant.startswith("bm"):
        flags = _flag(M, f"CS_FLAG_CHAIN_BM{variant[2:]}")
        kw["tile"] = int(variant[2:])
    elif variant == "no_chain":
        flags, kw["per_layer"] = _flag(M, "CS_FLAG_NO_CHAIN"), True
        expect = {"prepare_input": 1, "gemm_fwd": L, "gemm_dgrad": L - 1, "wgrad": 1}
    elif variant == "no_chain_fb":
        flags = _flag(M, "CS_FLAG_NO_CHAIN_FB")
        expect = {"chain_fwd": 1, "chain_bwd": 1, "wgrad": 1}
    elif variant == "wgrad2":
        env["CS_WGRAD2"], kw["wgrad2"] = "1", True
    else:
        env["CS_WGRAD_SPLITK"], kw["splitk"] = variant[6:], int(variant[6:])
    for k, v in env.items():                       # (read per handle in cs_mlp_create)
        monkeypatch.setenv(k, v)
    run_case(M, cfg_model, n, R.dispatch(n, **kw), flags=flags, expect=expect, tag=variant)


@pytest.mark.parametrize("n", [1023, 2047])
def test_cooperative_chain(M, cfg_model, n):
    run_case(M, cfg_model, n, R.dispatch(n), cooperative=True, expect=_fb(), tag="coop")


def test_predict_and_evaluate_with_a_ragged_last_chunk(M, cfg_model):
    """predict / evaluate in chunks of 8192 rows over 3 x 8192 + 17: sentinels on both sides of the last chunk's start, in its
    middle and in its last row; NaN rows behind the set inside the allocation."""
    mlp = M[0]
    n = 3 * 8192 + 17
    pos = [3 * 8192 - 1, 3 * 8192, 3 * 8192 + 8, n - 1]
    x, y, ref = cfg_model.batch(n, pos)
    xs = torch.full((n + 256, 124), float("nan"), device="cuda")
    ys = torch.full((n + 256, 128), float("nan"), device="cuda")
    xs[:n], ys[:n] = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    m = mlp.MLPEmulator(units=CFG, max_batch=8192, seed=None)
    m.set_weights(cfg_model.ws)
    pred = in_ref_order(m.predict(xs[:n], batch_size=8192), n, pos)
    assert np.all(np.isfinite(pred))
    assert R.rel(pred, ref.yhat) <= 1e-3
    assert np.max(np.abs(pred - ref.yhat)) <= 6e-3 * np.max(np.abs(ref.yhat))
    ev = m.evaluate(xs[:n], ys[:n], batch_size=8192)
    R.check(ev["mse"] * 128 * n, ev["mae"] * 128 * n, None, ref, cfg_model.sent, len(pos), tag="evaluate")
    m.close()


def _adam_state(ws, seed):
    """A non-zero optimiser state (Adam's first step normalises each element to +-lr: a gradient element near zero could flip
    its sign with the order of float additions; later steps are smooth in the gradient)."""
    rng = np.random.default_rng(seed)
    m = [rng.normal(0, 1e-4, w.shape).astype(np.float32) for w in ws]
    v = [(np.abs(a) * 3 + 1e-5).astype(np.float32) ** 2 for a in m]
    return m, v, 10


def _live_and_fresh(M, model, sizes, cooperative, tag):
    mlp = M[0]
    live = mlp.MLPEmulator(units=CFG, optimizer="Adam", max_batch=max(sizes), seed=None, cooperative=cooperative)
    live.set_weights(model.ws)
    live.set_optimizer_state(*_adam_state(model.ws, 5))
    worst_g = worst_w = 0.0
    for s, n in enumerate(sizes):
        d = R.dispatch(n)
        pos = R.sentinel_positions(n, d)
        k = len(pos)
        w0 = live.get_weights()
        st = live.get_optimizer_state()
        sent = R.Sentinels(w0, model.cfg, cols=model.sent.cols)
        x, y = sent.batch(model.bx[:n - k], model.by[:n - k], pos)
        ref = sent.expected(O.row_sums(w0, model.bx[:n - k], model.by[:n - k], model.cfg), k)
        dev = stage(x, y, seed=1000 + s)
        fresh = mlp.MLPEmulator(units=CFG, optimizer="Adam", max_batch=max(sizes), seed=None, cooperative=cooperative)
        fresh.set_weights(w0)
        fresh.set_optimizer_state(*st)
        la, ga = loss_and_grads(live, dev, n)
        lb, gb = loss_and_grads(fresh, dev, n)
        R.check(la[0], la[1], ga, ref, sent, k, tag=f"{tag} step {s} n={n}")
        np.testing.assert_allclose(la, lb, rtol=1e-6)
        for a, b in zip(ga, gb):
            worst_g = max(worst_g, R.rel(a, b))
            assert R.rel(a, b) <= 1e-6, (tag, s, n, R.rel(a, b))
        live.train_on_batch(dev[0], dev[1], 1e-4, row_idx=dev[2], n=n)
        fresh.train_on_batch(dev[0], dev[1], 1e-4, row_idx=dev[2], n=n)
        plain = R.dispatch(n, in_step=True).plain
        for a, b in zip(live.get_weights() + live.get_optimizer_state()[0], fresh.get_weights() + fresh.get_optimizer_state()[0]):
            if plain:
                assert np.array_equal(a, b), (tag, s, n, "stored splits: bit-identical step")
            else:
                worst_w = max(worst_w, R.rel(a, b))
                assert R.rel(a, b) <= 1e-6, (tag, s, n, R.rel(a, b))
        fresh.close()
    live.close()
    record_margin(f"ragged_{tag}_live_vs_fresh_grad_rel", worst_g)
    record_margin(f"ragged_{tag}_live_vs_fresh_weight_rel", worst_w)


def test_one_handle_across_changing_batch_sizes(M, cfg_model):
    """One handle through 8192 -> 8100 -> 8192 -> 22529 -> 8193 -> 1023 -> 2049 -> 1 -> 8192: after each change of n its gradients
    (oracle, sentinels; a fresh handle with the same weights and optimiser state: 1e-6) and its step (bit-identical where the
    step stores its row splits, 1e-6 where atomics add them) are those of a handle that never saw another batch size."""
    _live_and_fresh(M, cfg_model, [8192, 8100, 8192, 22529, 8193, 1023, 2049, 1, 8192], False, "live")


def test_one_cooperative_handle_across_changing_batch_sizes(M, cfg_model):
    """The cooperative chain's launch shape (members per tile, tiles) changes and comes back: 1023 -> 2047 -> 3000 -> 1023."""
    _live_and_fresh(M, cfg_model, [1023, 2047, 3000, 1023], True, "coop")


def test_group_with_changing_ragged_batch_sizes(M, base):
    """Three cfg-MLP members, batch sizes 500 / 1023 / 1 -> 4113 / 0 / 4097 -> 1023 / 2049 / 33: the middle step's 8448 rows
    (the sum of round_up(n, 128)) take 64-row tiles, the others 32; member 1 sits out the middle step.  Each member's step is held
    to the oracle row by row (sentinels at its first and last rows, tile and split edges) and to a solo handle that takes the same
    step from the same state."""
    mlp, group, _ = M
    bx, by = base
    steps = [(500, 1023, 1), (4113, 0, 4097), (1023, 2049, 33)]
    models = [weights(CFG, 20 + i) for i in range(3)]
    mem = []
    for i, (cfg, ws) in enumerate(models):
        m = mlp.MLPEmulator(units=CFG, optimizer="Adam", max_batch=4113, seed=None)
        m.set_weights(ws)
        m.set_optimizer_state(*_adam_state(ws, 30 + i))
        mem.append(m)
    g = group.MLPGroup(mem)
    cols = {}
    worst = 0.0
    for s, ns in enumerate(steps):
        bm, sk, per = R.group_dispatch(ns)
        assert bm == (64 if s == 1 else 32)
        xs, ys, idx, before, refs = [], [], [], {}, {}
        for i, n in enumerate(ns):
            if not n:
                xs.append(None); ys.append(None); idx.append(None)
                continue
            cfg = models[i][0]
            w0, st = mem[i].get_weights(), mem[i].get_optimizer_state()
            if i not in cols:                                   # (each member's quietest head columns)
                cols[i] = R.Sentinels(w0, cfg, O.row_sums(w0, bx[:4096], by[:4096], cfg)).cols
            pos = R.sentinel_positions(n, per[i])
            assert 0 in pos and n - 1 in pos
            k = len(pos)
            sent = R.Sentinels(w0, cfg, cols=cols[i], A=40.0)        # (<= 4113 rows: a smaller offset holds 60 % of a column)
            x, y = sent.batch(bx[:n - k], by[:n - k], pos)
            ref = sent.expected(O.row_sums(w0, bx[:n - k], by[:n - k], cfg), k)
            assert R.calibration(ref, sent, k) >= 0.3
            dev = stage(x, y, seed=100 * s + i)
            xs.append(dev[0]); ys.append(dev[1]); idx.append(dev[2])
            before[i], refs[i] = (w0, st, dev), (ref, sent, k)
        loss = g.train_on_batch(xs, ys, 1e-4, row_idx=idx, n=list(ns), active=[bool(n) for n in ns]).cpu().numpy()
        for i, n in enumerate(ns):
            if not n:
                continue
            (w0, st, dev), (ref, sent, k) = before[i], refs[i]
            gr = step_grads(mem[i], st[0], n)
            # (whole-tensor bar 1e-2: member 0 at 500 rows measured 7.9e-3 on the first kernel - the same on the grouped step, a solo
            #  one-call step and a solo loss_grads, so not a property of the grouped launch; the per-sentinel bars are unchanged)
            worst = max(worst, R.check(float(loss[i, 0]), float(loss[i, 1]), gr, ref, sent, k, tag=f"group step {s} member {i} n={n}",
                                       grad_bar=1e-2))
            record_margin("ragged_group_whole_tensor_grad_rel", max(R.rel(a, b) for a, b in zip(gr, ref.grads)))
            solo = mlp.MLPEmulator(units=CFG, optimizer="Adam", max_batch=4113, seed=None)
            solo.set_weights(w0)
            solo.set_optimizer_state(*st)
            sl = solo.train_on_batch(dev[0], dev[1], 1e-4, row_idx=dev[2], n=n).cpu().numpy()
            np.testing.assert_allclose(loss[i], sl, rtol=1e-5)
            gs = step_grads(solo, st[0], n)
            for a, b in zip(gr, gs):
                record_margin("ragged_group_vs_solo_grad_rel", R.rel(a, b))
                assert R.rel(a, b) <= 1e-3, (s, i, R.rel(a, b))
            for a, b in zip(mem[i].get_weights(), solo.get_weights()):
                record_margin("ragged_group_vs_solo_weight_rel", R.rel(a, b))
                assert R.rel(a, b) <= 1e-5, (s, i, R.rel(a, b))
            solo.close()
        assert mem[1].iterations == 10 + (2 if s == 2 else 1)
    record_margin("ragged_sentinel_share_of_bar", worst)
    g.close()
    for m in mem:
        m.close()
