"""The row-by-row checks of tests/test_ragged_batches_gpu.py without a GPU: the dispatch restatement gives the table of that
file's docstring, and the assertion helper (oracle/ragged.py: `check`) rejects oracle results that were mutated the way an edge
bug would mutate them - a sentinel dropped or doubled, the first / last row of a tile dropped, a sentinel's target paired with
its neighbour's input - while it accepts the unmutated result."""
import numpy as np
import pytest

from oracle import mlp_oracle as O
from oracle import ragged as R

# n -> (tile, weight-gradient kernel, splits, stored splits in a training step) on 256 CUs
TABLE = {1: (32, "k_wgrad3<4,64>", 2, True), 33: (32, "k_wgrad3<4,64>", 2, True), 1023: (32, "k_wgrad3<4,64>", 2, True),
         2049: (32, "k_wgrad3<4,64>", 3, True), 8191: (32, "k_wgrad3<4,64>", 3, True),
         8193: (64, "k_wgrad3<4,64>", 3, True), 11263: (64, "k_wgrad3<4,64>", 3, True),
         11265: (64, "k_wgrad3<4,32>", 6, False), 16383: (64, "k_wgrad3<4,32>", 6, False),
         16385: (128, "k_wgrad3<4,32>", 6, False), 22527: (128, "k_wgrad3<4,32>", 6, False),
         22529: (128, "k_wgrad2l", 12, False), 32769: (64, "k_wgrad2l", 12, False)}


@pytest.mark.parametrize("n", sorted(TABLE))
def test_dispatch_table(n):
    d = R.dispatch(n, in_step=True)
    assert (d.tile, d.kernel, d.splitk, d.plain) == TABLE[n]
    # split boundaries are multiples of the kernel's stage rows, strictly increasing, inside the padded batch
    assert all(b % d.rows == 0 for b in d.split_rows)
    assert d.split_rows == sorted(set(d.split_rows)) and all(0 < b < R.round_up(n, 128) for b in d.split_rows)


def test_dispatch_of_the_published_widths_and_groups():
    assert [(R.dispatch(n, R.PUB).tile, R.dispatch(n, R.PUB).kernel, R.dispatch(n, R.PUB).splitk) for n in (3071, 3073, 16385)] == \
        [(32, "k_wgrad3<4,64>", 2), (32, "k_wgrad3<4,64>", 2), (32, "k_wgrad3<4,32>", 4)]
    for ns, tile, sk in (((500, 1023, 1), 32, 2), ((4113, 0, 4097), 64, 3), ((1023, 2049, 33), 32, 2)):
        bm, k, per = R.group_dispatch(ns)
        assert (bm, k) == (tile, sk)
        assert sorted(per) == [i for i, n in enumerate(ns) if n]


@pytest.fixture(scope="module")
def setup():
    cfg = O.MLPConfig()
    ws = O.glorot_init(cfg, 3)
    rng = np.random.default_rng(103)
    for i in range(1, len(ws), 2):
        ws[i] = rng.normal(0, 0.05, ws[i].shape).astype(np.float32)
    n = 2500
    d = R.dispatch(n)
    pos = R.sentinel_positions(n, d)
    k = len(pos)
    bx, by = O.synth_columns(n - k, seed=7)
    base = O.row_sums(ws, bx, by, cfg)
    sent = R.Sentinels(ws, cfg, base)
    x, y = sent.batch(bx, by, pos)
    ref = sent.expected(base, k)
    return cfg, ws, n, d, pos, k, x, y, sent, ref


def _engine_like(ws, x, y, cfg):
    r = O.row_sums(ws, x, y, cfg)
    return r.sq, r.ab, [g.astype(np.float32) for g in r.grads]


def test_sentinels_are_calibrated_and_placed(setup):
    cfg, ws, n, d, pos, k, x, y, sent, ref = setup
    t = -(-n // d.tile)
    want = {0, n - 1, d.tile * (t - 1) - 1, d.tile * (t - 1), d.tile * (t - 2) - 1, d.tile * (t - 2)}
    for b in d.split_rows:
        want |= {b - 1, b}
    assert set(pos) == want and len(d.split_rows) == 2
    assert R.calibration(ref, sent, k) >= 0.3
    assert len(set(sent.cols[:k])) == k and max(sent.cols) < cfg.n_out_lin


def test_check_accepts_the_unmutated_batch(setup):
    cfg, ws, n, d, pos, k, x, y, sent, ref = setup
    assert R.check(*_engine_like(ws, x, y, cfg), ref, sent, k) < 1e-3


def _mutations(setup):
    cfg, ws, n, d, pos, k, x, y, sent, ref = setup
    t = -(-n // d.tile)
    first_of_last_tile = d.tile * (t - 1)
    mid = pos[len(pos) // 2]
    swap = np.arange(n)
    swap[[mid, mid + 1]] = swap[[mid + 1, mid]]
    return {
        "sentinel dropped": (np.delete(x, mid, 0), np.delete(y, mid, 0)),
        "sentinel doubled": (np.insert(x, mid, x[mid], 0), np.insert(y, mid, y[mid], 0)),
        "first row of the last tile dropped": (np.delete(x, first_of_last_tile, 0), np.delete(y, first_of_last_tile, 0)),
        "last row of a tile dropped": (np.delete(x, first_of_last_tile - 1, 0), np.delete(y, first_of_last_tile - 1, 0)),
        "last row of a split dropped": (np.delete(x, d.split_rows[0] - 1, 0), np.delete(y, d.split_rows[0] - 1, 0)),
        "target paired with the neighbour's input": (x[swap], y),
        "row n-1 dropped": (x[:-1], y[:-1]),
    }


@pytest.mark.parametrize("what", ["sentinel dropped", "sentinel doubled", "first row of the last tile dropped", "last row of a tile dropped",
                                  "last row of a split dropped", "target paired with the neighbour's input", "row n-1 dropped"])
def test_check_rejects_every_mutation(setup, what):
    cfg, ws, n, d, pos, k, x, y, sent, ref = setup
    mx, my = _mutations(setup)[what]
    with pytest.raises(AssertionError):
        R.check(*_engine_like(ws, mx, my, cfg), ref, sent, k)
