"""What tests/test_gpu_root_variants.py relies on, checked on the oracle and the NumPy model of the ladder alone (no GPU):
every row kind of every shape of tests/root_variants_program.py takes the path it is named for, and the oracle's own
draws keep the comparison meaningful (flat posteriors in the few / cap / slack / block families, the new-row candidate
drawn and the current referent kept at least once per shape)."""
import numpy as np
import pytest

import helpers
import root_variants_program as rvp

SHAPES = sorted(rvp.SHAPES)


@pytest.mark.parametrize("name", SHAPES)
def test_every_row_kind_takes_its_path(oracle, name):
    S = rvp.build(name, oracle, helpers)
    t = S["trace"].tables["Ent"]
    cur_all = S["trace"].cur[0]
    assert cur_all.min() >= -1 and cur_all.max() < t.n and t.live[cur_all[cur_all >= 0]].all()  # every index in range
    assert np.array_equal(t.counts[:t.n], np.bincount(cur_all[cur_all >= 0], minlength=t.n))    # counts == references
    n_dead = int((~t.live[:t.n]).sum())
    assert n_dead >= 2 and (np.flatnonzero(~t.live[:t.n]) < t.n - 1).all(), "dead rows below the high-water mark"
    if name == "groups":
        assert len(np.unique(np.concatenate([S["obs"], S["trace"].cur[:1]]), axis=1).T) >= rvp.SETTLE_MIN_GROUPS
    rows = rvp.sample_rows(S)
    world = rvp.oracle_world(oracle, helpers, S)
    E = rvp.expected_paths(S, oracle, helpers, rows=rows, world=world)
    kind = S["kind"][rows]
    print(f"{name}: {len(S['kind'])} rows ({len(rows)} modelled), {t.n} entities ({n_dead} dead), n_pre {E['n_pre']}, kblk {E['kblk']}; "
          f"refine {int(E['refine'].sum())}, overflow {int(E['overflow'].sum())}, settle {int(E['settle'].sum())}")
    rvp.check_paths(name, S, E, kind)
    cur = S["trace"].cur[0, rows]
    lse, _, draws = rvp.oracle_root(world, S, rows, cur)
    assert np.isfinite(lse).all()
    rvp.check_draws(name, S, kind, cur, draws)


def test_leaf_program(oracle):
    S = rvp.leaf_program()
    world = rvp.oracle_world(oracle, helpers, S)
    n_opt = len(S["words"])
    assert n_opt >= rvp.MIN_CAND and np.mean([len(w) for w in S["words"]]) >= 16
    rows = np.arange(S["obs"].shape[1], dtype=np.int32)
    E = rvp.expected_paths(S, oracle, helpers, rows=rows, world=world, node_id=1)
    assert E["n_pre"] == 3 and E["refine"].all() and E["certain"].all()  # (an option list has no bound: always guess-and-refine)
    assert E["overflow"].any() and not E["overflow"].all() and (E["widen"] >= 1).any()
    assert {"by_term", "per_lane", "over"} <= set(E["scheme"])
    lse, _, draws = world.score_node(0, 1, rows, seed=1, sweep=2, n_draws=rvp.N_DRAWS, n_cand=n_opt)
    assert np.isfinite(lse).all() and (rvp.diversity(draws) >= 3).sum() * 8 >= len(rows)
