"""The device commit's algorithm (the host build of csrc/commit_core.h, tests/commit_emul.py) on the keyed form of the
indexed proportions: records created through the keyed leaf — option (value, key), the value column read by the new row —
with duplicates, collections and reuse of freed rows, against the product's host commit; the gathered form over two
shards against the single form."""
import copy

import numpy as np

import commit_emul
import indexed_program as ip
from pclean_amd.parallel import Comm, exchange_and_commit
from test_commit_core import _stats_and_moved


def _outputs(S, tr, rng, n_new=12, n_move=20):
    """a sweep's outputs made by hand: n_move rows join a random live row, n_new propose a new row (some of them the same
    one) whose city option lies under the key its state leaf took"""
    lw = S["lw"]
    t = tr.tables["Doc"]
    n = tr.cur.shape[1]
    nk, nb, nc = len(ip.STATES), len(ip.CITIES), len(lw.latent_dom[("Doc", "npi")])
    choice = tr.cur.copy()
    rows = rng.choice(n, size=n_new + n_move, replace=False)
    new = np.sort(rows[:n_new]).astype(np.int32)
    choice[0, rows[n_new:]] = rng.choice(np.flatnonzero(t.live[:t.n]), size=n_move)
    choice[0, new] = -1
    chosen = rng.integers(1, 4, size=n).astype(np.int32)
    key = rng.integers(0, nk, size=n_new)
    vals = np.stack([-1 - chosen[new], rng.integers(0, nc, size=n_new), key, key * nb + rng.integers(0, nb, size=n_new)],
                    axis=1).astype(np.int32)
    vals[1, 1:] = vals[0, 1:]  # two rows propose the same new row: one row is created
    return choice.astype(np.int32), chosen, {0: (new, vals)}


def test_keyed_leaf_records_commit_like_the_host():
    S = ip.draw_program(seed=2)
    lw = S["lw"]
    tr = S["trace"]
    two = copy.deepcopy(tr)
    dev = commit_emul.EmulatedDevice(lw, tr, slack=256)
    gat = commit_emul.EmulatedDevice(lw, two, slack=256)
    assert dev.supported, dev.why
    rng = np.random.default_rng(8)
    n = tr.cur.shape[1]
    t = tr.tables["Doc"]
    reused = 0
    try:
        for sweep in range(5):
            choice, chosen, new_rows = _outputs(S, tr, rng)
            stats, moved = _stats_and_moved(lw, tr, choice)
            free_before = len(t.free)
            fb, n_changed, nrec, ndist = dev.commit(choice, chosen, new_rows, stats, sweep)
            n_distinct = len(np.unique(new_rows[0][1][:, 1:], axis=0))  # (identical proposals become one row)
            assert fb == 0 and int(nrec[0]) == 12 and int(ndist[0]) == n_distinct <= 11
            # the same sweep cut in two shards of unequal size
            cut = n // 3
            rows, vals = new_rows[0]
            shards = [(lo, hi, choice[:, lo:hi].copy(), chosen[lo:hi].copy(),
                       {0: ((rows[(rows >= lo) & (rows < hi)] - lo).astype(np.int32), vals[(rows >= lo) & (rows < hi)])})
                      for lo, hi in ((0, cut), (cut, n))]
            fb2, n_changed2, _, _ = gat.commit_gathered(shards, stats, sweep)
            assert fb2 == 0 and n_changed2 == n_changed
            changed = exchange_and_commit(tr, lw, Comm(), 0, choice, stats, new_rows, global_cur=True, moved_local=moved,
                                          n_local=n, sweep_idx=sweep)
            assert changed == n_changed
            dev.assert_equals_trace(tr, f"sweep {sweep}")
            gat.assert_equals_trace(tr, f"sweep {sweep}, two shards")
            tr.check_consistency()
            # a created row holds the value column of its option and the key its state leaf took
            ci = lw.colidx["Doc"]
            for j, i in enumerate(rows):
                r = tr.cur[0, i]
                assert t.cols[ci["city"], r] == vals[j, 3] % len(ip.CITIES) and t.cols[ci["state"], r] == vals[j, 3] // len(ip.CITIES)
                assert t.cols[ci["npi"], r] == vals[j, 1]
            reused += int(free_before > 0)
        assert reused > 0 and np.array_equal(tr.params[("Doc", "theta")].counts, tr.recount("Doc", "city"))
    finally:
        dev.close()
        gat.close()
