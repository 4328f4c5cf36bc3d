"""Several Gaussian observations in one block (tests/two_gauss_program.py): lowering, refusals, the per-term conjugate
draws of the mean parameters and the reported numeric columns.  CPU only."""
import math

import numpy as np
import pytest

import addnoise_program as ap
import two_gauss_program as tg
from pclean_amd import _lib
from pclean_amd.analysis import reconstructed_pool_ids
from pclean_amd.engine import make_gauss
from pclean_amd.model import (AddNoise, ChooseUniformly, IndexedLookup, IndexedMeanParameter, LoweredModel, Query,
                              Transformation, TransformedGaussian)


def test_two_terms_lower_onto_the_root_and_the_open_leaf():
    S = tg.setup(tg.two_model, 300)
    lw = S["lw"]
    assert [sp["gauss_attr"] for sp in lw.gauss_specs] == ["rent", "deposit"] and lw.gauss_spec is lw.gauss_specs[0]
    assert [sp["mean_table"] for sp in lw.gauss_specs] == [0, 1]
    assert [sp["param"] for sp in lw.gauss_specs] == [("Obs", "avg_rent"), ("Obs", "avg_deposit")]
    assert [sp["x_col"] for sp in lw.gauss_specs] == [0, 1] and lw.xnum.shape == (2, 300) and not lw.num_derived
    assert lw.locals == {0: ["br"]} and lw.gauss_block == 0
    # node (0, 0): rent first, deposit behind it, the same own choice
    root, more = lw.gauss[(0, 0)], lw.gauss_more[(0, 0)]
    assert root["gauss_attr"] == "rent" and [t["gauss_attr"] for t in more] == ["deposit"]
    for t in [root] + more:
        assert t["n_locals"] == 1 and t["local_n"] == [5] and t["local_obs"] == [lw.obs_index["br"]]
        assert [k[0] for k in t["kinds"]] == ["cand", "cand", "local"] and t["transform"] == ("none", -1)
    assert (make_gauss(root).mean_table, make_gauss(more[0]).mean_table) == (0, 1)
    assert (make_gauss(root).x_col, make_gauss(more[0]).x_col) == (0, 1)
    assert make_gauss(more[0]).sigma == 80.0
    # the open leaf (state: the one candidate-side index value that may be missing) carries both terms too
    leaf = next(nid for nid, info in enumerate(lw.blocks[0]["node_info"]) if info["kind"] == "leaf" and info["path"] == "state")
    assert lw.gauss[(0, leaf)]["gauss_attr"] == "rent" and [t["gauss_attr"] for t in lw.gauss_more[(0, leaf)]] == ["deposit"]
    for t in [lw.gauss[(0, leaf)]] + lw.gauss_more[(0, leaf)]:
        assert [k[0] for k in t["kinds"]] == ["cand", "obs", "local"] and t["kinds"][0] == ("cand", 0)
    assert lw.blocks[0]["nodes"][leaf][8] == 0
    # the latent County plan: both terms as evidence, the shared own choice from ctx slot 0 of the evidence row
    pb = lw.latent_plans["County"]["block_id"]
    lat = [(k, g) for k, g in lw.gauss.items() if k[0] == pb]
    assert len(lat) == 1
    key, first = lat[0]
    for t in [first] + lw.gauss_more[key]:
        assert t["n_locals"] == 0 and ("evctx", 0) in t["kinds"] and t["transform"] == ("none", -1)
    assert [t["gauss_attr"] for t in lw.gauss_more[key]] == ["deposit"] and lw.latent_ev_locals == {"County": 0}
    assert sorted(set(lw.gauss_more)) == sorted([(0, 0), (0, leaf), key])
    # the other declaration order swaps the terms and the mean tables
    lw2 = tg.setup(tg.two_model_swapped, 300)["lw"]
    assert [sp["gauss_attr"] for sp in lw2.gauss_specs] == ["deposit", "rent"]
    assert [sp["mean_table"] for sp in lw2.gauss_specs] == [0, 1] and lw2.gauss[(0, 0)]["gauss_attr"] == "deposit"


def test_mixed_terms_share_the_own_choices_and_derived_columns_follow_per_term():
    lw = tg.setup(tg.mixed_model, 200)["lw"]
    assert lw.locals == {0: ["br", "unit"]}
    rent, dep = lw.gauss[(0, 0)], lw.gauss_more[(0, 0)][0]
    assert rent["transform"] == ("local", 1) and dep["transform"] == ("none", -1)
    assert rent["n_locals"] == dep["n_locals"] == 2 and rent["local_n"] == dep["local_n"] == [5, 2]
    assert [k for k in dep["kinds"] if k[0] == "local"] == [("local", 0)]  # deposit indexes br alone; unit is still enumerated
    assert rent["t_scale"] == [1.0, 1000.0] and dep["t_scale"] == [1.0]

    # non-linear units: each term's derived columns behind the observed numeric ones, term by term
    def nl_model(dirty):
        m, o = ap._county_and_obs(dirty)
        o.choice("unit", ChooseUniformly([Transformation(math.exp, math.log, math.exp), tg.rents_units()[0]]))
        o.julia("rent_base", IndexedLookup("avg_rent"), list(tg.FULL))
        o.choice("rent", TransformedGaussian("rent_base", 150.0, "unit"))
        o.julia("corrected", lambda unit, rent: round(unit.backward(rent)), ["unit", "rent"])
        o.param("avg_deposit", IndexedMeanParameter(2000, 1000))
        o.julia("deposit_base", IndexedLookup("avg_deposit"), list(tg.FULL))
        o.choice("deposit", TransformedGaussian("deposit_base", 80.0, "unit"))
        o.julia("deposit_corrected", lambda unit, deposit: round(unit.backward(deposit)), ["unit", "deposit"])
        return m
    lw = tg.setup(nl_model, 100)["lw"]
    assert lw.gauss_specs[0]["t_x_col"] == [2, -1] and lw.gauss_specs[0]["t_lad_col"] == [3, -1]
    assert lw.gauss_specs[1]["t_x_col"] == [4, -1] and lw.gauss_specs[1]["t_lad_col"] == [5, -1]
    assert [d[0] for d in lw.num_derived] == [0, 0, 1, 1] and lw.xnum.shape == (6, 100)
    ok = ~np.isnan(lw.xnum[1])
    assert np.allclose(lw.xnum[4][ok], np.log(lw.xnum[1][ok])) and np.isnan(lw.xnum[4][~ok]).all()


def test_one_term_programs_lower_as_before():
    lw = ap.setup(ap.addnoise_model, 300)["lw"]
    assert lw.gauss_specs == [lw.gauss_spec] and lw.gauss_specs[0] is lw.gauss_spec and lw.gauss_more == {}
    assert lw.gauss_spec["gauss_attr"] == "rent" and lw.gauss_spec["mean_table"] == 0
    pb = lw.latent_plans["County"]["block_id"]
    assert sorted(k[0] for k in lw.gauss) == [0, 0, pb] and (0, 0) in lw.gauss
    assert lw.gauss[(0, 0)]["n_locals"] == 1 and lw.gauss[(0, 0)]["transform"] == ("none", -1)
    assert make_gauss(lw.gauss[(0, 0)]).mean_table == 0
    tr = ap.setup(ap.addnoise_model, 300)["trace"]
    assert tr.mean_params == [tr.mean_param] and tr.mean_params[0] is tr.mean_param


def _refusal_model(dirty, build):
    m, o = ap._county_and_obs(dirty)
    cols = {"CountyKey": "county.countykey", "County": ("county.name", "county_name"), "State": "county.state",
            "Room Type": "br"}
    build(m, o, cols)
    return m, Query(m, "Obs", cols)


def test_refusals_name_the_attribute():
    dirty, clean = ap.ex.rents_data()
    dirty = {c: v[:200] for c, v in dirty.items()}
    clean = {c: v[:200] for c, v in clean.items()}
    dirty, _ = tg.with_deposit(dirty, clean)
    for k in range(5):
        dirty[f"N{k}"] = dirty["Deposit"]

    def same_parameter(m, o, cols):
        o.julia("rent_base", IndexedLookup("avg_rent"), list(tg.FULL))
        o.choice("rent", AddNoise("rent_base", 150.0))
        o.julia("other_base", IndexedLookup("avg_rent"), list(tg.FULL))
        o.choice("deposit", AddNoise("other_base", 80.0))
        cols.update({"Monthly Rent": ("rent_base", "rent"), "Deposit": ("other_base", "deposit")})
    m, q = _refusal_model(dirty, same_parameter)
    with pytest.raises(NotImplementedError, match="deposit.*avg_rent"):
        LoweredModel(m, q, dirty)

    def five_terms(m, o, cols):
        for k in range(5):
            o.param(f"p{k}", IndexedMeanParameter(2000, 1000))
            o.julia(f"b{k}", IndexedLookup(f"p{k}"), list(tg.FULL))
            o.choice(f"n{k}", AddNoise(f"b{k}", 80.0))
            cols[f"N{k}"] = (f"b{k}", f"n{k}")
    m, q = _refusal_model(dirty, five_terms)
    with pytest.raises(NotImplementedError, match="n4.*more than 4"):
        LoweredModel(m, q, dirty)

    def other_leaf(m, o, cols):
        # rent leaves `state` open (CountyKey is always observed); the deposit's only candidate-side index is the name
        o.julia("rent_base", IndexedLookup("avg_rent"), list(tg.FULL))
        o.choice("rent", AddNoise("rent_base", 150.0))
        o.param("avg_deposit", IndexedMeanParameter(2000, 1000))
        o.julia("deposit_base", IndexedLookup("avg_deposit"), ["county.name", "br"])
        o.choice("deposit", AddNoise("deposit_base", 80.0))
        cols.update({"Monthly Rent": ("rent_base", "rent"), "Deposit": ("deposit_base", "deposit")})
    m, q = _refusal_model(dirty, other_leaf)
    with pytest.raises(NotImplementedError, match="deposit.*same candidate-side"):
        LoweredModel(m, q, dirty)

    def three_own_choices(m, o, cols):
        o.choice("unit", ChooseUniformly(tg.rents_units()))
        o.choice("unit2", ChooseUniformly(tg.rents_units()))
        o.julia("rent_base", IndexedLookup("avg_rent"), list(tg.FULL))
        o.choice("rent", TransformedGaussian("rent_base", 150.0, "unit"))
        o.param("avg_deposit", IndexedMeanParameter(2000, 1000))
        o.julia("deposit_base", IndexedLookup("avg_deposit"), list(tg.FULL))
        o.choice("deposit", TransformedGaussian("deposit_base", 80.0, "unit2"))
        cols.update({"Monthly Rent": ("rent_base", "rent"), "Deposit": ("deposit_base", "deposit")})
    m, q = _refusal_model(dirty, three_own_choices)
    with pytest.raises(NotImplementedError, match="at most two enumerated own choices"):
        LoweredModel(m, q, dirty)
    assert _lib.MAX_GAUSS == 4


def test_each_mean_parameter_is_resampled_from_its_own_term():
    """Trace.resample_parameters on a fixed assignment: every cell that holds a row lies within 6 posterior standard
    deviations of its closed-form conjugate mean (add_noise.jl:74-82), per term"""
    S = tg.setup(tg.two_model, 3000)
    lw, tr = S["lw"], S["trace"]
    assert len(tr.mean_params) == 2 and tr.mean_param is tr.mean_params[0]
    br = S["obs"][lw.obs_index["br"]]
    tr.locals[0][:, 0] = np.where(br >= 0, br, np.arange(3000) % 5)
    tr.resample_parameters("Obs")
    for g, (prior_mean, sigma) in enumerate([(1500.0, 150.0), (2000.0, 80.0)]):
        rows, idx, xs = tr.gaussian_index(g)
        x = lw.xnum[lw.gauss_specs[g]["x_col"]]
        assert np.array_equal(rows, np.flatnonzero(~np.isnan(x))) and np.array_equal(xs, x[rows])
        n = np.bincount(idx, minlength=len(tr.mean_params[g].value))
        sm = np.bincount(idx, weights=xs, minlength=len(tr.mean_params[g].value))
        cells = np.flatnonzero(n >= 1)  # (the closed form holds for any count: the assignment is fixed)
        assert len(cells) >= 50 and n.max() >= 20
        var = 1.0 / (1.0 / 1000.0 ** 2 + n[cells] / sigma ** 2)
        post = var * (prior_mean / 1000.0 ** 2 + sm[cells] / sigma ** 2)
        assert (np.abs(tr.mean_params[g].value[cells] - post) <= 6 * np.sqrt(var)).all(), g
    # the two parameters are different tables drawn from different rows
    assert not np.array_equal(tr.gaussian_index(0)[0], tr.gaussian_index(1)[0])


def test_both_numeric_columns_are_reported():
    S = tg.setup(tg.mixed_model, 400)
    lw, tr = S["lw"], S["trace"]
    tr.locals[0][:, 0] = 0
    tr.locals[0][:, 1] = np.arange(400) % 2
    ours = reconstructed_pool_ids(lw, tr)
    assert isinstance(ours["Monthly Rent"], tuple) and isinstance(ours["Deposit"], tuple)
    rent, dep = lw.xnum[0], lw.xnum[1]
    ok = ~np.isnan(rent)
    scale = np.where(np.arange(400) % 2 == 1, 1000.0, 1.0)
    assert np.array_equal(ours["Monthly Rent"][1][ok], np.round(rent * scale)[ok])
    ok = ~np.isnan(dep)
    assert ok.sum() > 300 and np.array_equal(ours["Deposit"][1][ok], np.round(dep[ok]))
    assert np.isnan(ours["Deposit"][1][~ok]).all()
