"""Three and four Gaussian observations in one block, and own choices that fill the 16 combinations
(tests/multi_gauss_program.py): lowering, the 16-combination refusal, the preconditions the GPU tests of
tests/test_gpu_multi_gauss.py rest on (presence patterns, power of the restatement, decided rows), the precision of the
restatement itself, and the per-term conjugate draws.  CPU only."""
import numpy as np
import pytest

import addnoise_program as ap
import multi_gauss_program as mg
import two_gauss_program as tg
from pclean_amd import _lib
from pclean_amd.engine import make_gauss
from pclean_amd.model import (AddNoise, ChooseUniformly, IndexedLookup, LoweredModel, Query, TransformedGaussian)

MODELS = {fn.__name__: fn for fn in (mg.three_model, mg.four_model, mg.four_model_permuted, mg.four_mixed_model,
                                     mg.sixteen_8x2, mg.sixteen_4x4, mg.sixteen_4x4_linear)}
ORDER = {"three_model": ["rent", "deposit", "fee"], "four_model": ["rent", "deposit", "fee", "util"],
         "four_model_permuted": ["util", "rent", "fee", "deposit"], "four_mixed_model": ["rent", "deposit", "fee", "util"],
         "sixteen_8x2": ["rent", "deposit", "fee"], "sixteen_4x4": ["rent", "deposit", "fee"],
         "sixteen_4x4_linear": ["rent", "deposit", "fee"]}
_cache = {}
PI = np.longdouble("3.141592653589793238462643383279502884")


def _setup(name, spread=mg.SCORE_SPREAD):
    """one lowered program per (model, spread) for the whole module; nothing below changes it"""
    if (name, spread) not in _cache:
        S = mg.setup(MODELS[name])
        mg.seed_means(S, spread)
        _cache[(name, spread)] = S
    return _cache[(name, spread)]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_lowering_puts_every_further_term_on_root_leaf_and_latent_plan(name):
    S = _setup(name)
    lw, attrs = S["lw"], ORDER[name]
    k = len(attrs)
    assert [sp["gauss_attr"] for sp in lw.gauss_specs] == attrs
    assert [sp["mean_table"] for sp in lw.gauss_specs] == list(range(k))
    assert [sp["param"] for sp in lw.gauss_specs] == [("Obs", f"avg_{a}") for a in attrs]
    # numeric columns in the query's order, each term reading its own
    assert [lw.num_cols[sp["x_col"]] for sp in lw.gauss_specs] == [mg.TERMS[a][0] for a in attrs]
    assert len({sp["sigma"] for sp in lw.gauss_specs}) == k
    leaf = next(nid for nid, info in enumerate(lw.blocks[0]["node_info"]) if info["kind"] == "leaf" and info["path"] == "state")
    pb = lw.latent_plans["County"]["block_id"]
    lat = [key for key in lw.gauss if key[0] == pb]
    assert len(lat) == 1
    assert sorted(lw.gauss_more) == sorted([(0, 0), (0, leaf), lat[0]])
    for key in [(0, 0), (0, leaf), lat[0]]:
        terms = [lw.gauss[key]] + lw.gauss_more[key]
        assert len(lw.gauss_more[key]) == k - 1 and k - 1 in (2, 3)
        assert [t["gauss_attr"] for t in terms] == attrs
        assert [make_gauss(t).mean_table for t in terms] == list(range(k))
        assert [make_gauss(t).x_col for t in terms] == [sp["x_col"] for sp in lw.gauss_specs]
        assert [make_gauss(t).sigma for t in terms] == [mg.TERMS[a][1] for a in attrs]
        for t in terms:  # the own choices are the block's: the same on every term
            assert (t["n_locals"], t["local_n"], t["local_obs"]) == (terms[0]["n_locals"], terms[0]["local_n"], terms[0]["local_obs"])
        if key[0] == pb:
            assert all(t["n_locals"] == 0 for t in terms)


def test_strides_and_own_choices_of_the_mixed_program():
    lw = _setup("four_mixed_model")["lw"]
    assert lw.locals == {0: ["br", "unit"]}
    assert [sp["strides"] for sp in lw.gauss_specs] == [[850, 5, 1], [850, 5, 1], [170, 1], [850, 5, 1]]
    assert [sp["n_mean"] for sp in lw.gauss_specs] == [40800, 40800, 8160, 40800]
    root = [lw.gauss[(0, 0)]] + lw.gauss_more[(0, 0)]
    assert [t["transform"] for t in root] == [("local", 1)] + [("none", -1)] * 3
    assert [[kd[0] for kd in t["kinds"]] for t in root] == [["cand", "cand", "local"]] * 2 + [["cand", "cand"]] + [["cand", "cand", "local"]]
    assert all(t["n_locals"] == 2 and t["local_n"] == [5, 2] for t in root)  # fee indexes no own choice; both are enumerated
    g = make_gauss(root[2])
    assert (g.n_dims, list(g.stride)[:2], g.n_locals) == (2, [170, 1], 2)


def test_sixteen_combinations_fill_every_transformation_slot():
    lw = _setup("sixteen_8x2")["lw"]
    assert lw.locals == {0: ["tier", "unit"]} and lw.gauss_specs[0]["local_n"] == [8, 2]
    # three linear scales and one option that is not linear: t_scale[2] and t_logabsderiv[2] hold values of their own,
    # option 3 reads the derived columns
    lw = _setup("sixteen_4x4")["lw"]
    assert lw.locals == {0: ["tier", "unit"]} and lw.gauss_specs[0]["local_n"] == [4, 4]
    rent, dep, fee = lw.gauss_specs
    assert rent["t_linear"] == dep["t_linear"] == [True, True, True, False]
    # derived columns behind the three observed ones, term by term: the rent's option 3, then the deposit's
    assert rent["t_x_col"] == [-1, -1, -1, 3] and rent["t_lad_col"] == [-1, -1, -1, 4]
    assert dep["t_x_col"] == [-1, -1, -1, 5] and dep["t_lad_col"] == [-1, -1, -1, 6]
    assert [d[0] for d in lw.num_derived] == [0] * 2 + [1] * 2 and lw.xnum.shape == (7, 600)
    c = np.log(1500.0) / 1500.0
    for spec, col in ((rent, 3), (dep, 5)):
        x = lw.xnum[spec["x_col"]]
        ok = ~np.isnan(x)
        assert ok.sum() >= 250
        bx = np.log(np.maximum(x[ok], 1.0)) / c
        np.testing.assert_allclose(lw.xnum[col][ok], bx, rtol=1e-15)
        np.testing.assert_allclose(lw.xnum[col + 1][ok], np.log(c) + c * bx, rtol=1e-13, atol=1e-13)
        assert np.isnan(lw.xnum[col][~ok]).all() and np.isnan(lw.xnum[col + 1][~ok]).all()
    lads = [0.0, float(np.log(1 / 1000.0)), float(np.log(1 / 100.0))]
    for name, scales, lad in (("sixteen_4x4", [1.0, 1000.0, 100.0, 1.0], lads + [0.0]),
                              ("sixteen_4x4_linear", mg.LINEAR_SCALES, lads + [float(np.log(1 / 10.0))])):
        lw = _setup(name)["lw"]
        assert len(set(scales[:3])) == 3 and scales[2] not in (1.0, 1000.0)
        n_terms = 0
        for key, first in lw.gauss.items():
            for t in [first] + lw.gauss_more[key]:
                g = make_gauss(t)
                if t["gauss_attr"] == "fee":
                    assert g.transform_src_kind == -1 and list(g.t_x_col) == [-1] * 4
                    continue
                # what the spec holds, and what make_gauss copies of it: four slots, none a default
                assert len(t["t_scale"]) == len(t["t_lad"]) == 4 and t["t_scale"] == scales and t["t_lad"] == lad
                assert list(g.t_scale) == scales and list(g.t_logabsderiv) == lad and g.transform_src == 1
                assert list(g.t_x_col) == t["t_x_col"] and list(g.t_lad_col) == t["t_lad_col"]
                if name == "sixteen_4x4":
                    assert g.t_x_col[3] >= 3 and g.t_lad_col[3] == g.t_x_col[3] + 1 and list(g.t_x_col)[:3] == [-1] * 3
                else:
                    assert list(g.t_x_col) == list(g.t_lad_col) == [-1] * 4 and lw.xnum.shape == (3, 600)
                n_terms += 1
        assert n_terms == 6  # rent and deposit on the root, the open leaf and the latent plan


@pytest.mark.parametrize("name", ["sixteen_4x4", "sixteen_4x4_linear"])
def test_every_transformation_option_explains_a_share_of_the_visited_rows(name):
    """the numbers of row i are written in unit i % 4, so in the marginal over the own choices the best combination's
    Transformation is option 0, 1, 2 and 3 each for several visited rows: a scale read from the wrong slot moves the
    candidate and new-row scores, not only the scores at fixed own choices"""
    S = _setup(name)
    pres = mg.presence(S)
    best = []
    for i, c in _visited_pairs(S):
        if pres[:2, i].any():
            combos, sc = mg.combo_scores(S, i, mg.referent_values(S, c))
            best.append(combos[int(np.argmax(sc))][1])
    n_best = np.bincount(best, minlength=4)
    print(f"{name}: best Transformation option of {len(best)} visited rows with a rent or a deposit: {n_best.tolist()}")
    assert (n_best >= 6).all()


def _combination_model(dirty, n_first, n_units):
    m, o = ap._county_and_obs(dirty, with_br=False)
    o.choice("tier", ChooseUniformly(mg.tier_names(n_first)))
    cols = {"CountyKey": "county.countykey", "County": ("county.name", "county_name"), "State": "county.state",
            "Monthly Rent": ("rent_base", "rent")}
    o.julia("rent_base", IndexedLookup("avg_rent"), list(mg.TIERED))
    if n_units > 1:
        o.choice("unit", ChooseUniformly((mg.four_units() * 2)[:n_units]))
        o.choice("rent", TransformedGaussian("rent_base", 150.0, "unit"))
    else:
        o.choice("rent", AddNoise("rent_base", 150.0))
    return m, Query(m, "Obs", cols)


@pytest.mark.parametrize("n_first,n_units,refused", [(9, 2, True), (17, 1, True), (8, 2, False), (4, 4, False), (16, 1, False)])
def test_more_than_sixteen_combinations_are_refused(n_first, n_units, refused):
    dirty, _ = ap.ex.rents_data()
    dirty = {c: v[:200] for c, v in dirty.items()}
    m, q = _combination_model(dirty, n_first, n_units)
    if refused:
        with pytest.raises(NotImplementedError, match="at most 16 combinations"):
            LoweredModel(m, q, dirty)
    else:
        lw = LoweredModel(m, q, dirty)
        assert lw.gauss_specs[0]["local_n"] == ([n_first, n_units] if n_units > 1 else [n_first])
        g = make_gauss(lw.gauss[(0, 0)])
        assert int(np.prod(list(g.local_n))) == 16
    assert _lib.MAX_GAUSS == 4


# ---- preconditions of the GPU tests --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["three_model", "four_model", "four_mixed_model", "sixteen_8x2", "sixteen_4x4",
                                  "sixteen_4x4_linear"])
def test_every_presence_pattern_occurs_a_dozen_times_with_and_without_the_own_choice(name):
    S = _setup(name)
    pres, own = mg.presence(S), mg.own_observed(S)
    k = len(pres)
    assert pres.shape == (k, 600)
    pat = (pres * (1 << np.arange(k))[:, None]).sum(axis=0)
    assert np.bincount(pat, minlength=1 << k).min() >= 12 and np.bincount(pat).shape == (1 << k,)
    assert np.bincount(pat[own], minlength=1 << k).min() >= 3 and np.bincount(pat[~own], minlength=1 << k).min() >= 3
    assert (pat == 0).sum() >= 12  # all-missing included
    rows, _ = mg.rows_visited(S, 4)
    assert set(pat[rows]) == set(range(1 << k)) and own[rows].any() and (~own[rows]).any()
    if name.startswith("sixteen"):  # rows that enumerate all 16 combinations, with at least one number to score
        assert sum(1 for i in rows if pat[i] and len(mg.combo_scores(S, int(i), mg.referent_values(S, int(S["trace"].cur[0, i])))[0]) == 16) >= 12
    # sigmas and mean tables all distinct
    assert len({sp["sigma"] for sp in S["lw"].gauss_specs}) == k
    tabs = [mp.value for mp in S["trace"].mean_params]
    assert all(not np.array_equal(tabs[a][:100], tabs[b][:100]) for a in range(k) for b in range(a + 1, k))


def _visited_pairs(S):
    """(row, its current referent) of the visited rows: index values that the new-row test scores for every visited row, and
    the candidate test for every row that is not its referent's only reference"""
    rows, _ = mg.rows_visited(S, 4)
    return [(int(i), int(S["trace"].cur[0, i])) for i in rows]


@pytest.mark.parametrize("name", ["three_model", "four_mixed_model", "sixteen_8x2", "sixteen_4x4", "sixteen_4x4_linear"])
def test_the_restatement_tells_every_misreading_apart(name):
    """power: a kernel that dropped a term, exchanged two sigmas, read another term's table, exchanged two strides or read
    Transformation option u from slot u & 1 would move the Gaussian part of at least a dozen visited (row, candidate) pairs
    by 1000 tolerances or more"""
    S = _setup(name)
    pairs = _visited_pairs(S)
    right = [tg.gauss_part(S, i, mg.referent_values(S, c)) for i, c in pairs]
    tol = np.array([mg.score_tolerance(n_comb, want) for want, n_comb in right])
    weakest = None
    for pname, kw in mg.perturbations(S).items():
        P = mg.perturbed(S, **kw)
        moved = np.array([abs(tg.gauss_part(P, i, mg.referent_values(S, c))[0] - want) for (i, c), (want, _) in zip(pairs, right)])
        n_far = int((moved >= 1000.0 * tol).sum())
        if weakest is None or n_far < weakest[0]:
            weakest = (n_far, pname)
        assert n_far >= 12, (pname, n_far)
    print(f"{name}: {len(mg.perturbations(S))} misreadings over {len(pairs)} pairs, the weakest moves {weakest[0]} of them ({weakest[1]})")


def _long_double_part(S, i, index_values):
    """two_gauss_program.gauss_part with every operation in np.longdouble (x, the means and log|deriv| are data)"""
    L = np.longdouble
    lw = S["lw"]
    if not mg.presence(S)[:, i].any():
        return L(0.0)
    spec0 = lw.gauss_specs[0]
    ranges, lp = [], L(0.0)
    for n, oc in zip(spec0["local_n"], spec0["local_obs"]):
        o = S["obs"][oc, i] if oc >= 0 else -1
        ranges.append([int(o)] if o >= 0 else list(range(n)))
        lp += -np.log(L(n))
    combos = [[]]
    for r in ranges:
        combos = [c + [v] for c in combos for v in r]
    vals = []
    for c in combos:
        s = lp
        for g, spec in enumerate(lw.gauss_specs):
            x = lw.xnum[spec["x_col"], i]
            if x != x:
                continue
            idx = sum(st * (index_values[d[1]] if d[0] == "cand" else c[d[1]]) for d, st in zip(spec["dims"], spec["strides"]))
            unit = spec["units"][0 if spec["t_local"] is None else c[spec["t_local"]]]
            bx = float(unit.backward(float(x)))
            lad = L(float(np.log(abs(float(unit.deriv(bx))))))
            z = (L(bx) - L(S["trace"].mean_params[g].value[idx])) / L(spec["sigma"])
            s += -L(0.5) * z * z - np.log(L(spec["sigma"])) - L(0.5) * np.log(L(2) * PI)
            s -= lad
        vals.append(s)
    vals = np.array(vals, dtype=L)
    m = vals.max()
    return m + np.log(np.sum(np.exp(vals - m))) if len(vals) > 1 else vals[0]


@pytest.mark.parametrize("name", ["three_model", "four_mixed_model", "sixteen_8x2", "sixteen_4x4", "sixteen_4x4_linear"])
def test_the_restatement_is_exact_to_1e_13(name):
    """float64 against long double on the visited pairs: 1e-13 relative, a tenth of the 1e-12 the GPU tests allow"""
    assert np.finfo(np.longdouble).eps < 1e-18
    S = _setup(name)
    worst = 0.0
    for i, c in _visited_pairs(S):
        iv = mg.referent_values(S, c)
        got, _ = tg.gauss_part(S, i, iv)
        diff = float(_long_double_part(S, i, iv) - np.longdouble(got))
        worst = max(worst, abs(diff) / max(abs(got), 1e-300) if got else abs(diff))
        assert abs(diff) <= 1e-13 * abs(got), (i, c, got, diff)
    print(f"{name}: float64 restatement within {worst:.2e} relative of the long-double one")


def test_combination_scores_marginalise_to_the_gaussian_part():
    for name in ("four_mixed_model", "sixteen_4x4"):
        S = _setup(name)
        for i, c in _visited_pairs(S):
            iv = mg.referent_values(S, c)
            combos, sc = mg.combo_scores(S, i, iv)
            want, n_comb = tg.gauss_part(S, i, iv)
            assert len(combos) == n_comb or not mg.presence(S)[:, i].any()
            if mg.presence(S)[:, i].any():
                m = sc.max()
                assert (m + np.log(np.sum(np.exp(sc - m))) if len(sc) > 1 else sc[0]) == want
            else:
                assert (sc == 0.0).all() and want == 0.0


@pytest.mark.parametrize("name", ["four_mixed_model", "sixteen_8x2"])
def test_enough_rows_have_their_own_choices_decided(name):
    """precondition of the own-choice test: with the means spread DECIDED_SPREAD sigmas, at the current referent, one
    combination outweighs all others (the runner-up's fixed-point weight is 0) for at least 100 rows, 30 of them with the
    first own choice unobserved"""
    S = _setup(name, mg.DECIDED_SPREAD)
    own, tr = mg.own_observed(S), S["trace"]
    n_decided = n_unobserved = 0
    for i in range(600):
        d = mg.decided(S, i, mg.referent_values(S, int(tr.cur[0, i])))[3]
        n_decided += d
        n_unobserved += d and not own[i]
    print(f"{name}: {n_decided} of 600 rows decided, {n_unobserved} of them with the first own choice unobserved")
    assert n_decided >= 100 and n_unobserved >= 30


def test_each_of_four_mean_parameters_is_resampled_from_its_own_term():
    """Trace.resample_parameters on a fixed assignment: every occupied cell lies within 6 posterior standard deviations of
    its closed-form conjugate mean (add_noise.jl:74-82), per term"""
    S = mg.setup(mg.four_model, 3000)
    lw, tr = S["lw"], S["trace"]
    assert len(tr.mean_params) == 4 and tr.mean_param is tr.mean_params[0]
    mg.fix_locals(S)
    tr.resample_parameters("Obs")
    seen = []
    for g, attr in enumerate(ORDER["four_model"]):
        _, sigma, prior_mean, _ = mg.TERMS[attr]
        rows, idx, xs = tr.gaussian_index(g)
        x = lw.xnum[lw.gauss_specs[g]["x_col"]]
        assert np.array_equal(rows, np.flatnonzero(~np.isnan(x))) and np.array_equal(xs, x[rows])
        n = np.bincount(idx, minlength=len(tr.mean_params[g].value))
        sm = np.bincount(idx, weights=xs, minlength=len(tr.mean_params[g].value))
        cells = np.flatnonzero(n >= 1)
        assert len(cells) >= 50 and n.max() >= 10
        var = 1.0 / (1.0 / mg.PRIOR_STD ** 2 + n[cells] / sigma ** 2)
        post = var * (prior_mean / mg.PRIOR_STD ** 2 + sm[cells] / sigma ** 2)
        assert (np.abs(tr.mean_params[g].value[cells] - post) <= 6 * np.sqrt(var)).all(), attr
        seen.append(rows)
    assert all(not np.array_equal(seen[a], seen[b]) for a in range(4) for b in range(a + 1, 4))
