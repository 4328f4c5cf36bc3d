"""What tests/test_gpu_enum_variants.py relies on, checked on the oracle alone (no GPU): the programs of
enum_variants_program.py keep the posteriors flat enough for draws to tell a wrong prefix or a wrong owning lane from a
right one, and the shapes sit where the launch ladder's thresholds are.

Draw condition: for every option-list length of the GPU test, at least a quarter of the first 64 rows have 3 or more
distinct values among 7 oracle draws of the leaf.  FK condition: at least a quarter of the items of every
reference-slot shape draw 2 or more distinct referents, some item draws the new-row candidate and some item keeps its
current referent.  Evidence: every latent row has evidence, one has more than 64 rows, one has only missing cells."""
import numpy as np
import pytest

import enum_variants_program as evp
import helpers


def lds_bytes(nc):
    return ((nc + 1) & ~1) * 8 + 640


def test_shapes_sit_on_the_thresholds():
    """(restated from pclean_launch_enum; the GPU test's counters say whether the library still agrees)"""
    assert lds_bytes(2480) <= 20 * 1024 < lds_bytes(2481)
    assert lds_bytes(10160) <= 80 * 1024 < lds_bytes(10161)
    assert lds_bytes(20400) == 160 * 1024 < lds_bytes(20401)
    for n in (256, 257, 1024, 1025, 4095, 4096, 10161, 20400, 20401):
        assert n in evp.LEAF_SHAPES
    assert {s[0] + 1 for s in evp.FK_SHAPES} >= {258, 1026, 4095, 4096, 4097, 1101, 20401}
    assert {s[0] for s in evp.EV_SHAPES} >= {300, 2047, 2048, 20401} and max(s[1] for s in evp.EV_SHAPES) > 1024
    rows = evp.big_sample(65537)
    assert len(rows) == 256 == len(set(rows.tolist())) and set(rows.tolist()) >= {0, 65536, 1023, 1024, 32767, 32768, 32769}


def test_program_data():
    S = evp.program(300, 700, 50, evp.SEED, crowd=10)
    y, words = S["dirty"]["Y"], S["words"]
    assert len(y) == 710 and len(set(words)) == 300 and all(4 <= len(w) <= 8 and set(w) <= set("abcdefgh") for w in words)
    ent = [i % 50 for i in range(700)] + [0] * 10
    clean = [i for i in range(710) if y[i] is not None and y[i] == words[ent[i]]]
    missing = [i for i in range(710) if y[i] is None]
    other = {y[i] for i in range(710) if y[i] is not None and y[i] != words[ent[i]]}
    assert len(clean) >= 710 // 3 - len(missing) and 0 < len(missing) < 40
    assert other and len(other) <= evp.POOL and all(len(s) == 5 for s in other) and not (other & set(words))
    S["trace"].check_consistency()
    assert S["trace"].tables["A"].n == 50 and np.array_equal(S["trace"].cur[0], ent)
    # more entities than options: entities that hold the same word stay apart
    S = evp.fk_program(1025)
    S["trace"].check_consistency()
    t = S["trace"].tables["A"]
    assert t.n == 1025 and t.counts[0] == 1 + evp.CROWD and (t.counts[1:t.n] == 1).all()
    assert np.array_equal(t.cols[0, :300], t.cols[0, 300:600]) and len(np.unique(t.cols[0, :t.n])) == 300


@pytest.mark.parametrize("n_options", sorted(evp.LEAF_SHAPES))
def test_leaf_draws_are_not_near_deterministic(oracle, n_options):
    S = evp.leaf_program(n_options)
    world = evp.oracle_world(oracle, helpers, S)
    lse, _, draws = evp.oracle_leaf(world, S, np.arange(64, dtype=np.int32), evp.N_DRAWS)
    div = evp.diversity(draws)
    print(f"{n_options} options: {int((div >= 3).sum())} of 64 rows with >= 3 distinct values among {evp.N_DRAWS} draws")
    assert np.isfinite(lse).all() and (div >= 3).sum() >= 16
    assert draws.min() >= 0 and draws.max() < n_options and draws.max() >= n_options // 2


@pytest.mark.parametrize("n_latent,items", [s[:2] for s in evp.FK_SHAPES])
def test_fk_draws_move_create_and_stay(oracle, n_latent, items):
    S = evp.fk_program(n_latent)
    world = evp.oracle_world(oracle, helpers, S)
    rows = evp.fk_items(n_latent, items)
    assert len(rows) == items == len(set(rows.tolist())) and rows.max() < S["obs"].shape[1]
    excl = S["trace"].cur[0, rows]
    lse, _, draws = evp.oracle_fk(world, S, rows, excl)
    div = evp.diversity(draws)
    new, stay = (draws < 0).any(axis=1), (draws == excl[:, None]).any(axis=1)
    print(f"{n_latent} latent rows, {items} items: {int((div >= 2).sum())} draw >= 2 distinct referents, "
          f"{int(new.sum())} the new-row candidate, {int(stay.sum())} keep their referent")
    assert np.isfinite(lse).all() and (div >= 2).sum() * 4 >= items
    assert new.any() and stay.any() and not new.all()
    assert draws.max() >= n_latent // 2  # (referents from the far end of the table too)
    # the oracle's restatement of the new-row branch == its recursive evaluation of the sub-tree
    for k in (0, items - 1):
        assert world.eval_tree(0, 0, rows[k], None, excl[k], n_latent + 1)[0] == lse[k]


@pytest.mark.parametrize("n_options,n_latent", [s[:2] for s in evp.EV_SHAPES])
def test_evidence_sets(oracle, n_options, n_latent):
    from pclean_amd._lib import InferConfig
    from pclean_amd.engine import InferenceConfig
    from pclean_amd.inference import build_evidence, latent_current_choices
    S = evp.ev_program(n_options, n_latent)
    lw, tr = S["lw"], S["trace"]
    live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "A")
    n_ev = np.diff(ev_off)
    assert len(live) == n_latent and n_ev.min() >= 1 and n_ev.max() > 64
    y = np.array([v is None for v in S["dirty"]["Y"]])
    all_missing = [t for t in range(n_latent) if y[ev_rows[ev_off[t]:ev_off[t + 1]]].all()]
    assert len(all_missing) == 1
    world = evp.oracle_world(oracle, helpers, S)
    pl = lw.latent_plans["A"]
    for P, mh in evp.EV_CONFIGS:
        excl = latent_current_choices(lw, tr, "A", live, InferenceConfig(1, P, use_mh_instead_of_pg=mh))
        chosen, vals = world.sweep_latent(InferConfig(1, P, 1, 1, int(mh), 50, 100), 9, 1, pl["block_id"], pl["roots"], live,
                                          ev_off, ev_rows, ev_ctx, excl, len(pl["nodes"]))
        moved = int((vals[:, 0] != tr.tables["A"].cols[0, live]).sum())
        print(f"{n_options} options, {n_latent} latent rows, P = {P}: {moved} rows take another value, "
              f"{len(np.unique(vals))} distinct values")
        assert moved * 4 >= n_latent and len(np.unique(vals)) * 4 >= min(n_latent, n_options)
