"""The programs of tests/memo_program.py on the oracle alone (no GPU): the conditions without which test_gpu_leaf_memo.py
could pass on a broken memo.  They are conditions on the INPUTS: when one fails after a change of the programs, change the
data (seeds, pools) until the oracle meets it again; do not loosen it.

  * every row list has at least 4 096 items (the memo's threshold) and more than 75 % distinct tuples (lists with more
    duplicates are de-duplicated before the memo sees them), rows whose every observed cell is missing, and tuples that recur;
  * the new-row score of the scored slot takes at least a quarter as many distinct values as there are items: a memo that
    answers with another tuple's marginal changes what is compared;
  * every perturbation of the reset tests (other option log-probabilities, the other distance mode, other class densities,
    another max_typos, other fn-table contents) changes the leaf's marginal on at least half of the items: a memo that
    survives the change serves visibly stale values;
  * in ctx2, items with equal observed tuples and different ctx values get different marginals.

The frozen oracle does not know tabulated terms, so `tab`'s leaf marginal is restated here in float64 from the pieces of
tests/tabulated_program.py (a restatement of the inputs' diversity, not a reference for the device's bits)."""
import numpy as np
import pytest

import helpers
import memo_program as mp
import tabulated_program as tp

HALF_LOG26 = 1.629048269010741


@pytest.fixture(scope="module")
def programs():
    return {name: make() for name, make in mp.PROGRAMS.items()}


@pytest.mark.parametrize("name", sorted(mp.PROGRAMS) + ["two"])
def test_lists_reach_the_memo_with_missing_rows_and_recurring_tuples(programs, name):
    S = programs[name] if name != "two" else mp.two()
    if name == "two":  # both leaves: block 0 reads columns 0, 1 and block 1 columns 2, 3 — the same integers but for a few cells
        obs = S["obs"]
        assert (obs[0] == obs[2]).mean() > 0.9 and (obs[1] == obs[3]).mean() > 0.9
        S = dict(S, key_cols=[0, 1], ctx=None)
    assert np.array_equal(mp.FIRST, mp.AGAIN)
    assert len(np.intersect1d(mp.FIRST, mp.SHIFTED)) == len(np.setdiff1d(mp.SHIFTED, mp.FIRST)) == mp.N_FIRST // 2
    for what, rows in mp.LISTS.items():
        keys = mp.keys_of(S, rows)
        assert len(rows) >= 4096
        assert len(set(keys)) > 0.75 * len(rows), (name, what, len(set(keys)))
        assert len(set(keys)) < len(rows), (name, what)
        if name in ("cols3", "cols6", "ctx2"):  # the saturation test's programs: more keys than its larger table has slots
            assert len(set(keys)) > 4096, (name, what)
        n_obs = len(S["key_cols"])
        assert sum(all(v < 0 for v in k[:n_obs]) for k in keys) >= 8, (name, what)
        if S["ctx"] is None:
            # families: many keys agree in the leading words of the stored key and differ in the last, and the other way
            # round — a lookup that compares only a part of the key answers with a relative's marginal wherever it passes one
            cut = n_obs - 2 if n_obs >= 4 else n_obs - 1
            for part in (range(cut), range(n_obs - cut, n_obs)):
                by = {}
                for k in keys:
                    by.setdefault(tuple(k[p] for p in part), set()).add(k)
                assert sum(len(by[tuple(k[p] for p in part)]) > 8 for k in keys) >= 400, (name, what, list(part))
    # SHIFTED's new half holds tuples of neither earlier list, some of them twice (two inserts of one key in the partial launch)
    seen = set(mp.keys_of(S, mp.FIRST))
    fresh = [k for k in mp.keys_of(S, mp.SHIFTED) if k not in seen]
    assert len(fresh) > 1000 and len(set(fresh)) < len(fresh), (name, len(fresh))
    assert len(fresh) < len(mp.SHIFTED) - 1000


@pytest.mark.parametrize("name", mp.ORACLE_PROGRAMS + ("cols7",))
def test_new_row_scores_are_diverse(oracle, programs, name):
    S = programs[name]
    world = mp.oracle_world(oracle, helpers, S)
    for what, rows in mp.LISTS.items():
        lse, scores, draws = mp.oracle_slot(world, S, rows)
        assert np.isfinite(lse).all() and np.isfinite(scores[:, -1]).all()
        assert len(np.unique(scores[:, -1])) * 4 >= len(rows), (name, what)
        assert (draws < 0).any() and (draws >= 0).any(), (name, what)


def _changed(a, b):
    assert a.shape == b.shape and np.isfinite(a).all() and np.isfinite(b).all()
    return int((a != b).sum())


@pytest.mark.parametrize("name", mp.ORACLE_PROGRAMS)
def test_perturbations_move_the_oracles_leaf_marginal(oracle, programs, name):
    S = programs[name]
    lw, rows = S["lw"], mp.FIRST
    base_logp = helpers.option_logp_cpu(oracle, lw, S["trace"])
    before = mp.oracle_leaf(mp.oracle_world(oracle, helpers, S), S, rows)
    # other option log-probabilities, the same values
    other_logp = dict(base_logp)
    other_logp[S["leaf_attr"]] = mp.other_option_logp(S)
    after = mp.oracle_leaf(mp.oracle_world(oracle, helpers, S, option_logp=other_logp), S, rows)
    assert _changed(before, after) * 2 >= len(rows), name
    # the other distance mode
    after = mp.oracle_leaf(mp.oracle_world(oracle, helpers, S, dist_mode=1), S, rows)
    assert _changed(before, after) * 2 >= len(rows), name
    # another max_typos on one term of the leaf
    world = mp.oracle_world(oracle, helpers, S)
    world.load_block(S["block"], *mp.other_max_typos(S))
    after = mp.oracle_leaf(world, S, rows)
    assert _changed(before, after) * 2 >= len(rows), name
    if name == "ctx2":  # other contents of the fn table under the same id
        world = mp.oracle_world(oracle, helpers, S)
        world.set_fn(*mp.other_fn_table(S))
        after = mp.oracle_leaf(world, S, rows)
        assert _changed(before, after) * 2 >= len(rows), name


def test_ctx2_equal_observations_with_another_ctx_value_have_another_marginal(oracle, programs):
    S = programs["ctx2"]
    world = mp.oracle_world(oracle, helpers, S)
    n_same = n_other = n_differ = 0
    for what, rows in mp.LISTS.items():
        leaf = mp.oracle_leaf(world, S, rows)
        keys = mp.keys_of(S, rows)
        at = {int(r): j for j, r in enumerate(rows)}
        for j, r in enumerate(rows):
            r = int(r)
            if not mp.is_repeat(r) or r - mp.REPEAT_BACK not in at:
                continue
            j0 = at[r - mp.REPEAT_BACK]
            assert keys[j][:2] == keys[j0][:2]
            if keys[j][2] == keys[j0][2]:
                n_same += 1
                assert leaf[j] == leaf[j0]
            elif not all(v < 0 for v in keys[j][:2]) and keys[j][1] >= 0:  # (the ctx value is read by the term of column v)
                n_other += 1
                n_differ += int(leaf[j] != leaf[j0])
    # (a random string in column v may be as far from f(x, z) as from f(x', z) for every z; the three quarters of the pool
    # that are made from one joined string are not)
    assert n_same >= 100 and n_other >= 100 and n_differ * 4 >= n_other * 3, (n_same, n_other, n_differ)
    # ... and the other way round: one ctx value under many observed tuples
    assert len(set(k[2] for k in mp.keys_of(S, mp.FIRST))) == len(S["lw"].latent_dom[("A", "x")])


# ---- tab: the leaf's marginal restated ------------------------------------------------------------------------------------
def tab_leaf_marginals(oracle, S, rows, T=None):
    """float64 log-marginal of tab's leaf per item: uniform prior + FormatName's tabulated term (T: its densities, default
    the program's own) + the AddTypos term"""
    lw, obs = S["lw"], S["obs"]
    terms = lw.block_arrays(0)[1][S["leaf_terms"]]
    (pid_t, (rule, cls, T0)), = tp.term_tables(lw).items()
    T = T0 if T is None else T
    sym, off, _, _ = lw.pool.arrays()
    typo = {pid: oracle.pair_table(sym, off, odom.id_array(), ldom.id_array(), 0).astype(np.int64)
            for pid, odom, ldom in lw.pair_id.values()}
    ldom = lw.latent_dom[S["leaf_attr"]]
    L = np.array([len(ldom.string(v)) for v in range(len(ldom))])
    _, _, _, nb, logl = helpers.density_tables_cpu(oracle, int(lw.pool.lens.max()))
    assert int(terms[0]["pair_table"]) == pid_t and set(int(t["pair_table"]) for t in terms[1:]) == set(typo)
    n = S["n_options"]
    out = np.empty(len(rows))
    for j, r in enumerate(rows):
        sc = np.full(n, -np.log(n))
        o = int(obs[int(terms[0]["obs_col"]), r])
        sc = sc + (T[:, 3] if o < 0 else T[np.arange(n), cls[o]])
        for t in terms[1:]:
            o = int(obs[int(t["obs_col"]), r])
            if o >= 0:  # an AddTypos term skips a missing observation
                d = typo[int(t["pair_table"])][o]
                sc = sc + (nb[(L + 4) // 5, d] - logl[L] * d - HALF_LOG26 * d)
        m = sc.max()
        out[j] = m + np.log(np.exp(sc - m).sum())
    return out


def other_class_density(S):
    (pid, (rule, cls, T)), = tp.term_tables(S["lw"]).items()
    return pid, np.tile(np.log([0.7, 0.25, 0.05, 0.5]), (len(T), 1))


def test_tab_other_class_densities_move_the_leaf_marginal(oracle, programs):
    S = programs["tab"]
    terms = S["lw"].block_arrays(0)[1][S["leaf_terms"]]
    from pclean_amd import _lib
    assert [int(t["dens_kind"]) for t in terms] == [_lib.DENS_TABULATED, _lib.DENS_ADD_TYPOS, _lib.DENS_ADD_TYPOS]
    before = tab_leaf_marginals(oracle, S, mp.FIRST)
    after = tab_leaf_marginals(oracle, S, mp.FIRST, other_class_density(S)[1])
    assert _changed(before, after) * 2 >= len(mp.FIRST)
    assert len(np.unique(before)) * 4 >= len(mp.FIRST)
    # every class of the rule occurs among the observed cells
    (_, (rule, cls, T)), = tp.term_tables(S["lw"]).items()
    o = S["obs"][int(terms[0]["obs_col"])]
    assert set(np.unique(cls[o[o >= 0]])) == {0, 1, 2}
