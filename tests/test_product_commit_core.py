"""The device commit's algorithm (host build of csrc/commit_core.h) on a plan with a product leaf: a record created
through the leaf fills BOTH columns of the new row (value column cc of the chosen option), duplicates merge, rows are
collected and their ids reused — equal to the product's host commit; the gathered form over two shards equals the single
form; and a plan handed over without the leaf's stride is refused (PCC_FB_PLAN), nothing modified."""
import copy

import numpy as np

import commit_emul_cols
import indexed_program as ip
from pclean_amd.parallel import Comm, exchange_and_commit
from test_commit_core import _stats_and_moved

NA, NB = len(ip.DEGREES), len(ip.SPECS)


def _outputs(tr, rng, n_new=10, n_move=16):
    t = tr.tables["Doc"]
    n = tr.cur.shape[1]
    choice = tr.cur.copy()
    rows = rng.choice(n, size=n_new + n_move, replace=False)
    new = np.sort(rows[:n_new]).astype(np.int32)
    choice[0, rows[n_new:]] = rng.choice(np.flatnonzero(t.live[:t.n]), size=n_move)
    choice[0, new] = -1
    chosen = rng.integers(1, 4, size=n).astype(np.int32)
    vals = np.stack([-1 - chosen[new], rng.integers(0, NA * NB, size=n_new)], axis=1).astype(np.int32)
    vals[1, 1] = vals[0, 1]  # two rows propose the same pair: one row is created
    return choice.astype(np.int32), chosen, {0: (new, vals)}


def test_product_leaf_records_fill_both_columns():
    S = ip.product_program(seed=6)
    lw, tr = S["lw"], S["trace"]
    dev = commit_emul_cols.EmulatedDeviceCols(lw, tr, slack=256)
    gat = commit_emul_cols.EmulatedDeviceCols(lw, copy.deepcopy(tr), slack=256)
    assert dev.supported, dev.why
    rng = np.random.default_rng(3)
    n = tr.cur.shape[1]
    t, ci = tr.tables["Doc"], lw.colidx["Doc"]
    reused = off_diagonal = 0
    try:
        for sweep in range(5):
            choice, chosen, new_rows = _outputs(tr, rng)
            rows, vals = new_rows[0]
            stats, moved = _stats_and_moved(lw, tr, choice)
            reused += int(len(t.free) > 0)
            fb, n_changed, nrec, ndist = dev.commit(choice, chosen, new_rows, stats, sweep)
            assert fb == 0 and int(nrec[0]) == 10 and int(ndist[0]) == len(np.unique(vals[:, 1])) <= 9
            cut = n // 3
            shards = [(lo, hi, choice[:, lo:hi].copy(), chosen[lo:hi].copy(),
                       {0: ((rows[(rows >= lo) & (rows < hi)] - lo).astype(np.int32), vals[(rows >= lo) & (rows < hi)])})
                      for lo, hi in ((0, cut), (cut, n))]
            fb2, n_changed2, _, _ = gat.commit_gathered(shards, stats, sweep)
            assert fb2 == 0 and n_changed2 == n_changed
            # the emulated table itself: both columns of every created row
            cols, cur = dev.tab["Doc"]["cols"], dev.cur[0]
            for j, i in enumerate(rows):
                a, b = int(vals[j, 1]) // NB, int(vals[j, 1]) % NB
                assert (cols[ci["degree"], cur[i]], cols[ci["spec"], cur[i]]) == (a, b), (sweep, i)
                off_diagonal += int(a != b)
            changed = exchange_and_commit(tr, lw, Comm(), 0, choice, stats, new_rows, global_cur=True, moved_local=moved,
                                          n_local=n, sweep_idx=sweep)
            assert changed == n_changed
            dev.assert_equals_trace(tr, f"sweep {sweep}")
            gat.assert_equals_trace(tr, f"sweep {sweep}, two shards")
            tr.check_consistency()
        assert reused > 0 and off_diagonal > 10  # (column 0 and column 1 differed: reading one column for both would show)
    finally:
        dev.close()
        gat.close()


def test_a_plan_without_the_leafs_stride_is_refused():
    S = ip.product_program(seed=6)
    lw, tr = S["lw"], S["trace"]
    dev = commit_emul_cols.EmulatedDeviceCols(lw, tr, slack=64, with_strides=False)
    try:
        choice, chosen, new_rows = _outputs(tr, np.random.default_rng(3))
        stats, _ = _stats_and_moved(lw, tr, choice)
        before = copy.deepcopy(dev.tab), dev.cur.copy()
        fb, _, _, _ = dev.commit(choice, chosen, new_rows, stats, 0)
        assert fb & 8, fb  # PCC_FB_PLAN
        for k in ("cols", "counts", "live", "free", "state"):
            assert np.array_equal(dev.tab["Doc"][k], before[0]["Doc"][k]), k
        assert np.array_equal(dev.cur, before[1])
    finally:
        dev.close()
