"""Ragged batches, row by row -- TEST INFRASTRUCTURE, NOT PRODUCT CODE (tests/test_ragged_batches_gpu.py, tests/test_oracle.py).

The MLP engine picks its kernels by batch size, and every pick has its own code for the last, partly empty row tile and for the
ends of its weight-gradient row splits.  One row is 1/n of a loss sum, so the whole-tensor bars of the parity tests (loss 2e-3,
gradients 5e-3 in norm) cannot see one row dropped, doubled or gathered from the wrong place at n ~ 10^4.  What this module adds:

  * `dispatch` / `group_dispatch`: the tile height and weight-gradient launch the engine picks at n, restated from
    climsim_amd/csrc/climsim_hip.hip (chain_bm_of, run_backward, cs_mlp_group_train_step);
  * `sentinel_positions`: the rows where an edge goes wrong at that pick;
  * `Sentinels`: rows whose target is offset by +A on one linear-head column of their own, so that each dominates the bias
    gradient and the weight-gradient column of that output - and `check`, which holds an engine result to the oracle per
    sentinel (1 % of the sentinel's own contribution) on top of the whole-tensor bars.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import mlp_oracle as O

F32 = np.float32
CFG = (512,) * 5
PUB = (768, 640, 512, 640, 640)
WG2_ROWS = 32           # rows per stage of k_wgrad2 / k_wgrad2l / k_wgrad3<4,32> / k_wgrad3_group (csrc/wgrad2.h)
WGRAD_PARTS = 2         # CS_WGRAD_PARTS (csrc/kernels.h): a training step stores up to 1 + 2 row splits without atomics
CWD_BM = 32             # the wide chain's row tile (csrc/chainw.h)


def round_up(n, m):
    return (n + m - 1) // m * m


def _tiles(units, tdim, n_in=124, n_out=128):
    dims = [n_in, *units, n_out, n_out]
    return sum(-(-round_up(dims[i], 128) // tdim) * -(-round_up(dims[i + 1], 128) // tdim) for i in range(len(dims) - 1))


def tuned_chain(units):
    """The tuned layer chain takes hidden widths of 128, 256 or 512 (cs_mlp_create); anything else runs the wide chain."""
    return all(u in (128, 256, 512) for u in units)


def chain_bm(n, n_cu=256):
    """chain_bm_of at default flags: 32-row tiles up to 8192 rows, above that the height with the fewest rounds of workgroups
    on the CUs times the cost of one workgroup (1 : 1.35 : 2.2 for 32 : 64 : 128 rows)."""
    if n <= 8192:
        return 32
    best, best_cost = 64, 1e30
    for bm, w in ((32, 1.0), (64, 1.35), (128, 2.2)):
        cost = -(-(-(-n // bm)) // n_cu) * w
        if cost < best_cost - 1e-9:
            best, best_cost = bm, cost
    return best


@dataclass
class Dispatch:
    tile: int                 # row-tile height of the layer chain (or the per-layer GEMMs' 128)
    kernel: str               # weight-gradient kernel
    splitk: int               # row splits of the weight-gradient launch
    rows: int                 # rows per stage of that kernel: splits end on multiples of it
    split_rows: List[int]     # first row of splits 1 .. splitk-1
    plain: bool               # a training step stores its splits (no float atomics) - the step is then bit-reproducible


def _split_rows(m_pad, rows, splitk):
    # k_wgrad2* / k_wgrad3 (csrc/wgrad2.h): steps = m_pad / rows; split s contracts steps [steps*s/splitk, steps*(s+1)/splitk)
    steps = m_pad // rows
    return [rows * (steps * s // splitk) for s in range(1, splitk)]


def dispatch(n, units=CFG, n_cu=256, tile=None, splitk=None, wgrad2=False, per_layer=False, in_step=False):
    """What run_forward / run_backward launch for a batch of n rows at default flags, or with the per-handle switches:
    `tile` = CS_FLAG_CHAIN_BM32/64/128, `splitk` = CS_WGRAD_SPLITK, `wgrad2` = CS_WGRAD2=1, `per_layer` = CS_FLAG_NO_CHAIN.
    `in_step`: the one-call training step (cs_mlp_train_step) rather than cs_mlp_loss_grads."""
    m_pad = round_up(n, 128)
    if per_layer:
        bm = 128
    elif not tuned_chain(units):
        bm = CWD_BM
    else:
        bm = tile or chain_bm(n, n_cu)
    big = wgrad2 or n >= 22528
    tiles = _tiles(units, 256 if big else 128)
    if splitk:
        sk = splitk
    elif big:
        sk = (256 + tiles // 2) // tiles
    else:
        sk = n_cu // tiles if n < 11264 else (7 * n_cu // 4) // tiles
        sk = min(sk, 2) if n < 2048 else min(sk, 3) if n < 6144 else sk
    sk = max(1, min(sk, m_pad // WG2_ROWS))
    if big:
        kernel, rows = "k_wgrad2l", WG2_ROWS
    elif tiles * sk <= n_cu and m_pad // 64 >= sk:
        kernel, rows = "k_wgrad3<4,64>", 64
    else:
        kernel, rows = "k_wgrad3<4,32>", WG2_ROWS
    plain = in_step and not big and 2 <= sk <= WGRAD_PARTS + 1
    return Dispatch(bm, kernel, sk, rows, _split_rows(m_pad, rows, sk), plain)


def group_dispatch(ns: Sequence[int], units=CFG, n_cu=256):
    """cs_mlp_group_train_step for members of one tuned-chain shape with batch sizes `ns` (0 = sits out): one chain launch that
    tiles by the SUM of the members' round_up(n, 128) and gives every member whole tiles from its own row 0, one k_wgrad3_group
    launch (32-row stages) whose split count follows the active members' tile count and smallest batch.
    Returns (tile, splitk, {member: Dispatch})."""
    act = [i for i, n in enumerate(ns) if n]
    total = sum(round_up(ns[i], 128) for i in act)
    bm = chain_bm(total, n_cu)
    tiles = _tiles(units, 128) * len(act)
    n_min = min(ns[i] for i in act)
    sk = max(1, (365 + tiles // 2) // tiles)
    sk = min(sk, 2) if n_min < 2048 else min(sk, 3) if n_min < 6144 else sk
    sk = min(sk, round_up(n_min, 128) // WG2_ROWS)
    per = {i: Dispatch(bm, "k_wgrad3_group", sk, WG2_ROWS, _split_rows(round_up(ns[i], 128), WG2_ROWS, sk), sk == 1) for i in act}
    return bm, sk, per


MAX_SENTINELS = 24


def sentinel_positions(n, d: Dispatch, limit=MAX_SENTINELS):
    """Row 0 and row n-1; both sides of the last two tile boundaries; both sides of every row-split boundary below n (latest
    first while more than `limit` rows are asked for)."""
    t = -(-n // d.tile)                                     # tiles that hold rows
    pos = [0, n - 1]
    for b in (d.tile * (t - 1), d.tile * (t - 2)):
        pos += [b - 1, b]
    for b in sorted(d.split_rows, reverse=True):
        pos += [b - 1, b]
    out = []
    for p in pos:
        if 0 <= p < n and p not in out:
            out.append(p)
    return sorted(out[:limit])


# ------------------------------------------------------------------------------- sentinels
class Sentinels:
    """Up to MAX_SENTINELS rows (inputs of their own) whose target carries +A on one linear-head column c_j each.  A = 500 on
    the quietest head columns makes every sentinel >= 30 % of d(loss)/d b_out[c_j] and of the norm of d(loss)/d W_out[:, c_j] at
    up to ~33k synthetic rows (asserted per batch: `calibration`).  The ReLU head (columns >= n_out_lin) is left alone: it could
    mask a sentinel."""

    A = 500.0

    def __init__(self, ws, cfg: O.MLPConfig, base: Optional[O.RowSums] = None, seed=4242, k=MAX_SENTINELS, cols=None, A=None):
        """`cols`: the output columns, else the k quietest of the linear head in `base` (an oracle result without sentinels)."""
        if cols is None:
            db, dw = np.abs(base.grads[-3]), np.linalg.norm(base.grads[-4], axis=0)
            quiet = db / db.max() + dw / dw.max()
            cols = np.argsort(quiet[:cfg.n_out_lin])[:k]
        self.cols = [int(c) for c in cols]
        if A is not None:
            self.A = float(A)
        self.x, y = O.synth_columns(k, seed=seed)
        self.y = y.copy()
        self.y[np.arange(k), self.cols] += F32(self.A)
        self.ws, self.cfg = ws, cfg
        self.rows = [O.row_sums(ws, self.x[j:j + 1], self.y[j:j + 1], cfg) for j in range(k)]

    def batch(self, bx, by, positions):
        """A logical batch of len(bx) + len(positions) rows: sentinel j at positions[j], the base rows in order around them."""
        n = len(bx) + len(positions)
        is_s = np.zeros(n, bool)
        is_s[positions] = True
        x = np.empty((n, bx.shape[1]), F32)
        y = np.empty((n, by.shape[1]), F32)
        x[~is_s], y[~is_s] = bx, by
        x[positions], y[positions] = self.x[:len(positions)], self.y[:len(positions)]
        return x, y

    def expected(self, base: O.RowSums, k):
        """Oracle result of `batch(...)` with k sentinels (order of rows aside: sums and row_sq / yhat of the base rows first)."""
        out = base
        for j in range(k):
            out = out + self.rows[j]
        return out


def calibration(ref: O.RowSums, sent: Sentinels, k):
    """Smallest share of its own output column that a sentinel holds in the oracle result (bias gradient and weight-gradient
    column norm)."""
    worst = np.inf
    for j in range(k):
        c, r = sent.cols[j], sent.rows[j]
        worst = min(worst, abs(r.grads[-3][c]) / (abs(ref.grads[-3][c]) + 1e-30),
                    np.linalg.norm(r.grads[-4][:, c]) / (np.linalg.norm(ref.grads[-4][:, c]) + 1e-30))
    return float(worst)


def rel(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / (np.linalg.norm(b) + 1e-30))


def check(got_sq, got_ab, got_grads: Optional[list], ref: O.RowSums, sent: Sentinels, k, tag="", grad_bar=5e-3):
    """Hold an engine result (unscaled loss sums, unscaled Keras-ordered gradients or None) to the oracle's `ref` for a batch
    with the first k sentinels: the whole-tensor bars of the parity tests and, per sentinel, the bias gradient and the weight-
    gradient column of its output within 1 % of its own contribution, the loss sums within 5 % of the smallest sentinel's
    error.  Raises AssertionError; returns the largest per-sentinel deviation as a share of its bar (<= 1)."""
    worst = 0.0
    assert np.isfinite(got_sq) and np.isfinite(got_ab), (tag, got_sq, got_ab)
    assert abs(got_sq - ref.sq) <= 2e-3 * ref.sq, (tag, "sq", got_sq, ref.sq)
    assert abs(got_ab - ref.ab) <= 2e-3 * ref.ab, (tag, "ab", got_ab, ref.ab)
    if k:
        bar_sq = 0.05 * min(float(r.row_sq[0]) for r in sent.rows[:k])
        bar_ab = 0.05 * min(r.ab for r in sent.rows[:k])
        assert abs(got_sq - ref.sq) <= bar_sq, (tag, "sq vs smallest sentinel", got_sq - ref.sq, bar_sq)
        assert abs(got_ab - ref.ab) <= bar_ab, (tag, "ab vs smallest sentinel", got_ab - ref.ab, bar_ab)
        worst = max(abs(got_sq - ref.sq) / bar_sq, abs(got_ab - ref.ab) / bar_ab)
    if got_grads is None:
        return worst
    for i, (g, r) in enumerate(zip(got_grads, ref.grads)):
        assert np.all(np.isfinite(g)), (tag, "non-finite gradient", i)
        assert rel(g, r) <= grad_bar, (tag, "gradient", i, rel(g, r))
    for j in range(k):
        c, own = sent.cols[j], sent.rows[j]
        bar_b = 0.01 * abs(own.grads[-3][c])
        bar_w = 0.01 * np.linalg.norm(own.grads[-4][:, c])
        db = abs(float(got_grads[-3][c]) - ref.grads[-3][c])
        dw = float(np.linalg.norm(np.asarray(got_grads[-4][:, c], np.float64) - ref.grads[-4][:, c]))
        assert db <= bar_b, (tag, f"sentinel {j} (column {c}): bias gradient off by {db:.4g} > {bar_b:.4g}")
        assert dw <= bar_w, (tag, f"sentinel {j} (column {c}): weight-gradient column off by {dw:.4g} > {bar_w:.4g}")
        worst = max(worst, db / bar_b, dw / bar_w)
    return worst
