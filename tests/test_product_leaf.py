"""The sibling-choice index of an IndexedProportionsParameter on the CPU: the product leaf's option order, its two value
columns, the terms' columns, the colmap of a new row, the latent plan's pair root; host commits through it (new rows fill
both columns, latent commits write both) with the [key][option] counts held against a recount."""
import numpy as np

import indexed_program as ip
from pclean_amd import _lib
from pclean_amd.inference import commit_latent, latent_current_choices
from pclean_amd.engine import InferenceConfig
from pclean_amd.parallel import Comm, exchange_and_commit
from test_commit_core import _stats_and_moved


def test_product_leaf_lowering():
    for uniform in (False, True):
        S = ip.product_program(uniform_index=uniform)
        lw = S["lw"]
        na, nb = len(ip.DEGREES), len(ip.SPECS)
        assert lw.indexed == {("Doc", "spec"): ("product", "degree")} and lw.product_index == {("Doc", "degree"): "spec"}
        cols = lw.option_cols[("Doc", "spec")]
        assert cols.shape == (2, na * nb)
        for a in range(na):
            for b in range(nb):  # option a * |B| + b holds (a, b)
                assert tuple(cols[:, a * nb + b]) == (a, b)
        blk = lw.blocks[0]
        assert [i["kind"] for i in blk["node_info"]] == ["fk", "leaf"]  # one leaf for both choices
        leaf = blk["nodes"][1]
        assert leaf[0] == _lib.NODE_LEAF and leaf[1] == lw.option_id[("Doc", "spec")] and leaf[8] == 0  # not cacheable
        assert blk["node_info"][1]["product"] == ("degree", "spec")
        terms = blk["terms"][leaf[2]:leaf[2] + leaf[3]]
        # the index's observation reads value column 0, the choice's column 1, in declaration order
        assert [(t[0], t[1], t[3]) for t in terms] == [(lw.obs_index["deg_obs"], 0, _lib.DENS_ADD_TYPOS),
                                                       (lw.obs_index["spec_obs"], 1, _lib.DENS_ADD_TYPOS)]
        ci = lw.colidx["Doc"]
        cm = blk["colmap"]
        assert (cm[2 * ci["degree"]], cm[2 * ci["degree"] + 1]) == (1, 0) and (cm[2 * ci["spec"]], cm[2 * ci["spec"] + 1]) == (1, 1)
        pl = lw.latent_plans["Doc"]
        assert pl["roots"] == [0] and pl["root_attr"] == [("degree", "spec")] and pl["nodes"][0][3] == 2
        assert [(t[1], t[3]) for t in pl["terms"]] == [(0, _lib.DENS_ADD_TYPOS), (1, _lib.DENS_ADD_TYPOS)]
        # nothing to exclude, no dummy: the latent sweep's excl row stays -1
        excl = latent_current_choices(lw, S["trace"], "Doc", np.arange(3), InferenceConfig(1, 2))
        assert excl.shape == (1, 3) and (excl == -1).all()


def test_host_commits_through_the_product_leaf():
    S = ip.product_program(seed=4)
    lw, tr = S["lw"], S["trace"]
    t, ci = tr.tables["Doc"], lw.colidx["Doc"]
    na, nb = len(ip.DEGREES), len(ip.SPECS)
    n = tr.cur.shape[1]
    rng = np.random.default_rng(1)
    theta, deg = tr.params[("Doc", "theta")], tr.params[("Doc", "deg_p")]

    def recount():
        live = np.flatnonzero(t.live[:t.n])
        want = np.zeros((na, nb), dtype=np.int64)
        for r in live:
            want[t.cols[ci["degree"], r], t.cols[ci["spec"], r]] += 1
        assert np.array_equal(theta.counts, want) and np.array_equal(deg.counts, want.sum(axis=1))

    recount()
    for sweep in range(4):
        choice = tr.cur.copy()
        rows = rng.choice(n, size=20, replace=False)
        new = np.sort(rows[:8]).astype(np.int32)
        choice[0, rows[8:]] = rng.choice(np.flatnonzero(t.live[:t.n]), size=12)
        choice[0, new] = -1
        opt = rng.integers(0, na * nb, size=8)
        vals = np.stack([np.full(8, -1), opt], axis=1).astype(np.int32)
        stats, moved = _stats_and_moved(lw, tr, choice)
        if sweep % 2:
            exchange_and_commit(tr, lw, Comm(), 0, choice, stats, {0: (new, vals)}, global_cur=True, sweep_idx=sweep)
        else:
            tr.commit(choice, {0: (new, vals)})
        for j, i in enumerate(new):  # a created row holds both columns of its option
            r = tr.cur[0, i]
            assert (t.cols[ci["degree"], r], t.cols[ci["spec"], r]) == (opt[j] // nb, opt[j] % nb)
        tr.check_consistency()
        recount()
        live = np.flatnonzero(t.live[:t.n]).astype(np.int32)
        chosen = (np.arange(len(live)) % 2).astype(np.int32)
        lv = rng.integers(0, na * nb, size=(len(live), 1)).astype(np.int32)
        assert commit_latent(lw, tr, "Doc", live, chosen, lv) > 0
        sel = live[chosen > 0]
        assert np.array_equal(t.cols[ci["degree"], sel], lv[chosen > 0, 0] // nb)
        assert np.array_equal(t.cols[ci["spec"], sel], lv[chosen > 0, 0] % nb)
        tr.check_consistency()
        recount()
    assert len(t.free) + int(t.live[:t.n].sum()) == t.n
