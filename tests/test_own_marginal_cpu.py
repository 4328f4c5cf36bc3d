"""Exact marginals of a flat class, everything that needs no GPU: the NumPy twin of pclean_own_marginals' definition
(own_marginal_program.marginal_twin with the oracle library's fixw) against the literal conditional within the derived
bound, the power of that comparison, the conditions the device leg relies on (ties inside the top, the share of rows whose
MAP the literal decides), and the host functions map_pool_ids / map_table / evaluate_map_accuracy / save_results."""
import numpy as np
import pytest

import own_choice_program as ocp
import own_marginal_program as omp
from pclean_amd.analysis import (evaluate_map_accuracy, f1_from_counts, counts_given, map_pool_ids, map_table,
                                 save_results)
from pclean_amd.engine import Engine
from pclean_amd.trace import Trace


def _fixer(oracle):
    f = oracle.lib().pco_fixw
    return lambda d: np.array([f(float(x)) for x in d], dtype=np.uint64)


def _worst(fixw, S, params, choice, top, mutate=None):
    """largest |twin probability - literal pi| over every reported option of every row; the twin scores what `mutate`
    leaves, the literal the program as it is"""
    rows = omp.exact_rows(S, params, choice)
    scored = omp.exact_rows(S, params, choice, mutate) if mutate else rows
    names = S["choices"][choice]
    opt, prob, _, _ = omp.marginal_twin(np.array([sc for sc, _ in scored]), fixw, top)
    worst = 0.0
    for i, (_, pi) in enumerate(rows):
        for t in range(top):
            if opt[t, i] >= 0:
                worst = max(worst, abs(prob[t, i] - pi.get(names[opt[t, i]], 0.0)))
    return worst, opt, prob, rows


@pytest.mark.parametrize("prog", ["flat3", "flat2b"])
def test_twin_lies_within_the_bound_of_the_literal_conditional(oracle, prog):
    S, params = omp.literal_cases()[prog]
    for choice, names in S["choices"].items():
        K = len(names)
        worst, opt, prob, rows = _worst(_fixer(oracle), S, params, choice, omp.MAX_TOP)
        assert worst <= omp.bound(K), (choice, worst, omp.bound(K))
        pis = [pi for _, pi in rows]
        for i in omp.compared_rows(S, pis, choice):
            assert names[opt[0, i]] == max(pis[i], key=pis[i].get)
        # the reported probabilities are ordered, and sum to one where every possible option is reported
        assert (np.diff(prob, axis=0) <= 0).all()
        full = (opt >= 0).sum(axis=0) < omp.MAX_TOP
        assert np.allclose(prob[:, full].sum(axis=0), 1.0, atol=omp.bound(K) * K)
    # the condition of the device leg: the literal alone decides the MAP option of at least 90 % of the cells
    assert omp.compared_share(S, params) >= 0.9


def test_the_comparison_has_power(oracle):
    S, params = omp.literal_cases()["flat3"]
    K = len(S["choices"]["name"])

    def no_prior(S_, par):
        return S_, {"p": np.full(K, 1.0 / K)}

    def no_term(S_, par):
        return dict(S_, terms={"name": [t for t in S_["terms"]["name"] if t[0] != "B"]}), par

    exact, _, _, _ = _worst(_fixer(oracle), S, params, "name", 3)
    assert exact <= omp.bound(K)
    for name, mutate in (("prior dropped", no_prior), ("one term dropped", no_term)):
        worst, _, _, _ = _worst(_fixer(oracle), S, params, "name", 3, mutate)
        assert worst > 1e6 * omp.bound(K), (name, worst)


def test_twin_slots_ties_and_impossible_rows(oracle):
    f = _fixer(oracle)
    sc = np.array([[0.0, -1.0, 0.0, -np.inf], [-np.inf] * 4, [-3.0, -50.0, -np.inf, -np.inf], [1.5, 1.5, 1.5, 1.5]])
    opt, prob, u, U = omp.marginal_twin(sc, f, 3)
    assert opt[:, 0].tolist() == [0, 2, 1] and prob[0, 0] == prob[1, 0] > prob[2, 0] > 0
    assert opt[:, 1].tolist() == [-1, -1, -1] and prob[:, 1].tolist() == [0.0, 0.0, 0.0] and U[1] == 0
    assert opt[:, 2].tolist() == [0, -1, -1] and prob[:, 2].tolist() == [1.0, 0.0, 0.0]  # (e^-47 is below 2^-40: weight 0)
    assert opt[:, 3].tolist() == [0, 1, 2] and prob[:, 3].tolist() == [0.25] * 3
    assert omp.current_twin(u, U, [1, 0, -1, 3]).tolist() == [float(np.float64(u[0, 1]) / np.float64(U[0])), 0.0, 0.0, 0.25]


def test_the_ties_program_ties(oracle):
    """on the literal's scores: every option of a row without an observation, and the two options of a tie pair"""
    S = omp.ties()
    words = S["choices"]["state"]
    rows = omp.exact_rows(S, {}, "state")
    opt, prob, u, U = omp.marginal_twin(np.array([sc for sc, _ in rows]), _fixer(oracle), omp.MAX_TOP)
    none = [i for i in range(S["n_rows"]) if S["dirty"]["Y"][i] is None]
    assert len(none) == 5
    for i in none:
        assert opt[:, i].tolist() == list(range(omp.MAX_TOP)) and len(set(u[i].tolist())) == 1
    for a, b, o in omp.TIE_PAIRS:
        ka, kb = sorted((words.index(a), words.index(b)))
        hit = [i for i in range(S["n_rows"]) if S["dirty"]["Y"][i] == o]
        assert hit
        for i in hit:
            assert u[i, ka] == u[i, kb] and opt[:2, i].tolist() == [ka, kb] and prob[0, i] == prob[1, i]


# ---- the host functions, on hand-made marginals ------------------------------------------------------------------------
def _hand_made():
    S = ocp.flat2b(n_rows=12, seed=4)
    lw, _ = ocp.lower(S)
    n = S["n_rows"]
    truth = S["truth"]
    marg = {}
    for choice, col in (("city", "City"), ("state", "State"), ("cond", "Cond")):
        names = S["choices"][choice]
        k = np.array([names.index(t) for t in truth[col]], dtype=np.int32)
        opt = np.stack([k, (k + 1) % len(names)]).astype(np.int32)
        prob = np.stack([np.full(n, 0.8), np.full(n, 0.2)])
        marg[choice] = (opt, prob, np.zeros(n))
    return S, lw, marg


def test_map_pool_ids_and_table():
    S, lw, marg = _hand_made()
    dirty = {c: list(v) for c, v in S["dirty"].items()}
    truth = S["truth"]
    marg["city"][0][0, 2] = -1  # no possible option in row 2
    marg["city"][1][0, 2] = 0.0
    ids = map_pool_ids(lw, marg)
    assert set(ids) == {"City", "State", "Cond"}
    assert ids["City"][2] == -1 and [lw.pool.strings[i] for i in ids["State"]] == truth["State"]
    table, conf = map_table(lw, marg, dirty)
    assert table["State"] == truth["State"] and table["Cond"] == truth["Cond"]
    assert table["City"][2] is None and table["City"][:2] + table["City"][3:] == truth["City"][:2] + truth["City"][3:]
    assert conf["City"][2] == 0.0 and conf["State"].tolist() == [0.8] * S["n_rows"]
    # thresholding: a cell below min_confidence keeps its dirty value, a missing dirty cell takes the MAP value all the same
    dirty["State"][0], dirty["State"][1], dirty["State"][3] = "not-in-the-pool", None, truth["State"][4]
    marg["state"][1][0, :] = [0.4, 0.4, 0.95, 0.4] + [0.95] * (S["n_rows"] - 4)
    table, conf = map_table(lw, marg, dirty, min_confidence=0.5)
    assert table["State"][0] == "not-in-the-pool" and table["State"][1] == truth["State"][1]
    assert table["State"][2] == truth["State"][2] and table["State"][3] == truth["State"][4]
    assert table["State"][4:] == truth["State"][4:]
    assert map_table(lw, marg, dirty, min_confidence=0.4)[0]["State"] == truth["State"]  # (>=: at the threshold MAP stands)
    plain = map_table(lw, marg, dirty)[0]["City"]  # 0.8 everywhere but in row 2, which has no possible option
    assert table["City"][:2] + table["City"][3:] == plain[:2] + plain[3:]
    assert table["City"][2] == dirty["City"][2] and plain[2] is None


def test_evaluate_map_accuracy():
    S, lw, marg = _hand_made()
    dirty, clean = S["dirty"], S["truth"]
    n = S["n_rows"]
    acc = evaluate_map_accuracy(lw, marg, dirty, clean)
    assert acc == f1_from_counts(counts_given(lw, map_pool_ids(lw, marg), n, dirty, clean))
    errors = sum(d is not None and d != c for col in clean for d, c in zip(dirty[col], clean[col]))
    missing = sum(d is None for col in clean for d in dirty[col])
    assert errors and acc["errors"] == errors == acc["changed"] == acc["cleaned"]
    assert acc["imputed"] == missing == acc["correctly_imputed"] and acc["f1"] == 1.0
    # above every confidence: nothing but the missing cells changes
    high = evaluate_map_accuracy(lw, marg, dirty, clean, min_confidence=0.9)
    assert high["changed"] == 0 and high["cleaned"] == 0 and high["imputed"] == missing == high["correctly_imputed"]
    assert high["errors"] == errors
    # one column confident: only its errors are repaired
    marg["cond"][1][0, :] = 0.99
    one = evaluate_map_accuracy(lw, marg, dirty, clean, min_confidence=0.9)
    cond_errors = sum(d is not None and d != c for d, c in zip(dirty["Cond"], clean["Cond"]))
    assert one["changed"] == one["cleaned"] == cond_errors


def test_save_results_writes_confidence_columns(tmp_path):
    import filecmp
    import os

    import pandas as pd
    S, lw, marg = _hand_made()
    tr = Trace.from_clean_values(lw, {0: {"city": S["truth"]["City"], "state": S["truth"]["State"]},
                                      1: {"cond": S["truth"]["Cond"]}}, S["n_rows"], seed=0)
    plain = save_results(str(tmp_path), "plain", lw, tr, S["dirty"], timestamp=False)
    with_m = save_results(str(tmp_path), "map", lw, tr, S["dirty"], timestamp=False, marginals=marg)
    assert sorted(os.listdir(plain)) == ["reconstructed_Obs.csv"]
    assert sorted(os.listdir(with_m)) == ["map_Obs.csv", "reconstructed_Obs.csv"]
    assert filecmp.cmp(f"{plain}/reconstructed_Obs.csv", f"{with_m}/reconstructed_Obs.csv", shallow=False)
    saved = pd.read_csv(f"{with_m}/map_Obs.csv", dtype=str)
    assert list(saved.columns) == ["City", "City__confidence", "State", "State__confidence", "Cond", "Cond__confidence"]
    assert saved["City"].tolist() == S["truth"]["City"] and saved["Cond__confidence"].astype(float).tolist() == [0.8] * S["n_rows"]


def test_engine_refuses_a_class_that_is_not_flat():
    T = ocp.twin1(ocp.flat1())
    from pclean_amd.model import LoweredModel
    lw = LoweredModel(T["model"], T["query"], T["dirty"])

    class Stub:
        pass

    stub = Stub()
    stub.lw = lw
    with pytest.raises(Exception, match="Engine.own_marginals: the observed class is not flat"):
        Engine.own_marginals(stub, Trace(lw, T["n_rows"]))
