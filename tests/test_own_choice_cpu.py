"""Own string choices of the observed class (flat models): lowering, refusals, host bookkeeping, and the power of the
device leg's distribution test — everything that needs no GPU.

tests/own_choice_program.py holds the programs (FLAT1, FLAT3, FLAT2B and their TWINs behind a slot).  The plan arrays are
pinned here; the exact conditional they are later held against (tests/test_gpu_own_choice.py) comes from oracle/literal.py on
the strings.  The power self-test samples with NumPy from the closed-form outputs (posterior_exact.pg_one_block /
mh_one_block on equal weights) under four mistakes a sweep could make, with exactly the rows, the S and the pooling of the
device leg: each must be rejected at posterior_exact.ALPHA and the exact sampler must pass."""
import math

import numpy as np
import pytest

import own_choice_program as ocp
import posterior_exact as pe
from pclean_amd import _lib
from pclean_amd import inference as inf
from pclean_amd.analysis import evaluate_accuracy, evaluate_accuracy_up_to, reconstructed_table
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.model import (AddNoise, AddTypos, ChooseProportionally, ChooseUniformly, FormatName, IndexedLookup,
                              IndexedMeanParameter, IndexedProportionsParameter, LoweredModel, Model, ProportionsParameter,
                              Query, StringPrior)
from pclean_amd.tally import ReconPlan
from pclean_amd.trace import Trace

LEAF = lambda table, tb, nt: (_lib.NODE_LEAF, table, tb, nt, 0, 0, -1, -1, 0, 0, 0, 0)  # noqa: E731
TERM = lambda obs, pair, dens=_lib.DENS_ADD_TYPOS, mt=-1: (obs, 0, pair, dens, mt, -1, -1, 0)  # noqa: E731


# ---- lowering ----------------------------------------------------------------------------------------------------
def test_flat1_lowers_to_one_leaf():
    S = ocp.flat1()
    lw, obs = ocp.lower(S)
    assert lw.flat and lw.own_leaf == {"city": (0, 0)} and not lw.latent_plans and not lw.layout
    blk = lw.blocks[0]
    assert blk["own"] and not blk.get("score")
    assert blk["nodes"] == [LEAF(lw.option_id[("Obs", "city")], 0, 1)]
    assert blk["terms"] == [TERM(0, lw.pair_id[("y", ("Obs", "city"))][0])]
    assert blk["children"] == [] and blk["colmap"] == [] and blk["ctx_src_block"] == []
    assert list(lw.option_values[("Obs", "city")]) == list(range(40))
    assert [lw.latent_dom[("Obs", "city")].string(k) for k in range(40)] == S["choices"]["city"]
    assert obs.shape == (1, S["n_rows"]) and (obs[0] == -1).sum() == 2
    nodes, terms = lw.own_block_arrays(0)
    assert nodes.dtype == _lib.NODE_DTYPE and terms.dtype == _lib.TERM_DTYPE and len(nodes) == 1 and len(terms) == 1


def test_flat3_term_order_and_pair_ids():
    S = ocp.flat3()
    lw, obs = ocp.lower(S)
    key = ("Obs", "name")
    assert lw.flat and lw.own_leaf == {"name": (0, 0)}
    pa, pb = lw.pair_id[("a", key)][0], lw.pair_id[("b", key)][0]
    pc = next(iter(lw.class_pairs))
    pe_ = lw.eq_pairs[("eq", key)][0]
    assert (pa, pb, pc, pe_) == (0, 1, 2, 3)  # in declaration order, the direct observation last
    assert lw.class_pairs[pc][0] == _lib.CLASS_FORMAT_NAME
    blk = lw.blocks[0]
    assert blk["nodes"] == [LEAF(lw.option_id[key], 0, 4)]
    assert blk["terms"] == [TERM(lw.obs_index["a"], pa), TERM(lw.obs_index["b"], pb, mt=2),
                            TERM(lw.obs_index["c"], pc, _lib.DENS_TABULATED), TERM(lw.obs_index["name"], pe_, _lib.DENS_EQUAL)]
    assert lw.direct_obs == {"name": key}
    # the twin's new-row leaf carries the same terms in the same order (what the parity test relies on)
    T = ocp.twin3(S)
    tl = LoweredModel(T["model"], T["query"], T["dirty"])
    leaf = tl.blocks[0]["nodes"][1]
    assert [t[2:5] for t in tl.blocks[0]["terms"][leaf[2]:leaf[2] + leaf[3]]] == [t[2:5] for t in blk["terms"]]


def test_flat2b_two_blocks_three_leaves():
    S = ocp.flat2b()
    lw, _ = ocp.lower(S)
    assert lw.flat and lw.own_leaf == {"city": (0, 0), "state": (0, 1), "cond": (1, 0)}
    b0, b1 = lw.blocks
    oid = lw.option_id
    assert b0["nodes"] == [LEAF(oid[("Obs", "city")], 0, 1), LEAF(oid[("Obs", "state")], 1, 1)]
    assert b0["terms"] == [TERM(0, lw.pair_id[("city_obs", ("Obs", "city"))][0]),
                           TERM(1, lw.pair_id[("state_obs", ("Obs", "state"))][0])]
    assert b1["nodes"] == [LEAF(oid[("Obs", "cond")], 0, 1)]
    assert b1["terms"] == [TERM(2, lw.pair_id[("cond_obs", ("Obs", "cond"))][0], mt=3)]
    assert lw.block_group == [0, 1]


def test_relower_and_load_blocks_rebuild_the_own_blocks():
    S = ocp.flat2b()
    lw, _ = ocp.lower(S)
    before = [(b["nodes"], b["terms"]) for b in lw.blocks]
    lw.relower({})
    assert lw.flat and [(b["nodes"], b["terms"]) for b in lw.blocks] == before

    class Target:
        def __init__(self):
            self.loaded = []

        def load_own_block(self, bi, nodes, terms):
            self.loaded.append((bi, len(nodes), len(terms)))

    t = Target()
    lw.load_blocks_into(t)
    assert t.loaded == [(0, 2, 2), (1, 1, 1)]
    with pytest.raises(NotImplementedError, match="does not know own blocks"):
        lw.load_blocks_into(object())


# ---- refusals ----------------------------------------------------------------------------------------------------
WORDS = ["alpha", "bravo", "charlie"]


def _latent(m):
    a = m.add_class("A")
    a.choice("x", ChooseUniformly(WORDS))


def _lower(m, bindings, data):
    return LoweredModel(m, Query(m, "Obs", bindings), data)


def test_refuses_own_choice_in_a_class_with_a_reference_slot_block():
    m = Model()
    _latent(m)
    o = m.add_class("Obs")
    o.param("p", ProportionsParameter())
    with o.block():
        o.fk("r", "A")
        o.choice("x_obs", AddTypos("r.x"))
    with o.block():
        o.choice("city", ChooseProportionally(WORDS, "p"))
        o.choice("y", AddTypos("city"))
    with pytest.raises(NotImplementedError, match=r"Obs\.city: .*also has reference-slot blocks \(r\).*mixed classes"):
        _lower(m, {"X": ("r.x", "x_obs"), "Y": ("city", "y")}, {"X": ["alpha"], "Y": ["bravo"]})


def test_refuses_own_choice_in_a_block_with_a_reference_slot():
    m = Model()
    _latent(m)
    o = m.add_class("Obs")
    o.param("p", ProportionsParameter())
    with o.block():
        o.fk("r", "A")
        o.choice("city", ChooseProportionally(WORDS, "p"))
        o.choice("y", AddTypos("city"))
    with pytest.raises(NotImplementedError, match=r"y: AddTypos of a non-reference: the own choice city .*slot r.*jointly"):
        _lower(m, {"Y": ("city", "y")}, {"Y": ["bravo"]})
    m = Model()
    _latent(m)
    o = m.add_class("Obs")
    with o.block():
        o.fk("r", "A")
        o.choice("city", ChooseUniformly(WORDS))
        o.choice("y", FormatName("city"))
    with pytest.raises(NotImplementedError, match=r"y: FormatName of the own choice city .*slot r .*joint enumeration"):
        _lower(m, {"Y": ("city", "y")}, {"Y": ["bravo"]})


def test_refuses_dummy_valued_own_choices():
    m = Model()
    o = m.add_class("Obs")
    with o.block():
        o.choice("s", StringPrior(1, 10, WORDS))
        o.choice("y", AddTypos("s"))
    with pytest.raises(NotImplementedError, match=r"Obs\.s: a StringPrior own choice is not lowered .*dummy value"):
        _lower(m, {"Y": ("s", "y")}, {"Y": ["bravo"]})
    from pclean_amd.model import NumberCodePrior, TimePrior
    m = Model()
    o = m.add_class("Obs")
    with o.block():
        o.choice("k", ChooseUniformly(["a", "b"]))
        o.choice("t", TimePrior({"a": ["1:00 a.m."], "b": ["2:00 p.m."]}, "k"))
        o.choice("y", AddTypos("t"))
    with pytest.raises(NotImplementedError, match=r"Obs\.t: a TimePrior own choice is not lowered"):
        _lower(m, {"Y": ("t", "y")}, {"Y": ["1:00 a.m."]})
    m = Model()
    o = m.add_class("Obs")
    with o.block():
        o.choice("code", NumberCodePrior())
    with pytest.raises(NotImplementedError, match=r"Obs\.code: NumberCodePrior among the observed class's own choices"):
        _lower(m, {"Code": "code"}, {"Code": ["12"]})


def test_refuses_an_observation_of_two_own_choices_or_of_a_julia_node():
    m = Model()
    o = m.add_class("Obs")
    with o.block():
        for n in ("f", "mid", "l"):
            o.choice(n, ChooseUniformly(WORDS))
        o.choice("full", FormatName(first="f", middle="mid", last="l"))
    with pytest.raises(NotImplementedError, match=r"Obs\.full: FormatName\(f, mid, l\) reads several own choices"):
        _lower(m, {"Full": ("f", "full")}, {"Full": ["alpha bravo"]})
    m = Model()
    o = m.add_class("Obs")
    with o.block():
        o.choice("city", ChooseUniformly(WORDS))
        o.julia("shout", lambda s: s.upper(), ["city"])
        o.choice("y", AddTypos("shout"))
    with pytest.raises(NotImplementedError, match=r"Obs\.y: AddTypos of the JuliaNode shout of an own choice"):
        _lower(m, {"Y": ("city", "y")}, {"Y": ["BRAVO"]})


def test_refuses_an_observation_in_another_block_than_its_choice():
    m = Model()
    o = m.add_class("Obs")
    with o.block():
        o.choice("city", ChooseUniformly(WORDS))
    with o.block():
        o.choice("other", ChooseUniformly(WORDS))
        o.choice("y", AddTypos("city"))
    with pytest.raises(NotImplementedError, match=r"Obs\.y: its choice city is declared in another block"):
        _lower(m, {"Y": ("city", "y")}, {"Y": ["bravo"]})


def test_refuses_index_and_gaussian_in_an_own_block():
    m = Model()
    o = m.add_class("Obs")
    o.param("w_p", IndexedProportionsParameter())
    with o.block():
        o.choice("k", ChooseUniformly(WORDS))
        o.choice("w", ChooseProportionally(WORDS, "w_p", index="k"))
        o.choice("y", AddTypos("w"))
    with pytest.raises(NotImplementedError, match=r"Obs\.w: an indexed choice among the observed class's own choices"):
        _lower(m, {"Y": ("w", "y")}, {"Y": ["bravo"]})
    m = Model()
    o = m.add_class("Obs")
    o.param("mu", IndexedMeanParameter(0.0, 1.0))
    with o.block():
        o.choice("k", ChooseUniformly(WORDS))
        o.julia("mean", IndexedLookup("mu"), ["k"])
        o.choice("x", AddNoise("mean", 1.0))
    with pytest.raises(NotImplementedError, match=r"Obs\.x: a Gaussian observation in a block without a reference slot"):
        _lower(m, {"X": ("mean", "x")}, {"X": [1.0]})


def test_refuses_a_directly_observed_value_outside_the_options():
    m = Model()
    o = m.add_class("Obs")
    with o.block():
        o.choice("city", ChooseUniformly(WORDS))
        o.choice("y", AddTypos("city"))
    with pytest.raises(ValueError, match=r"Obs\.city: observed value 'delta' is not among the options"):
        _lower(m, {"Y": ("city", "y"), "City": "city"}, {"Y": ["bravo", "alpha"], "City": [None, "delta"]})
    _lower(m, {"Y": ("city", "y"), "City": "city"}, {"Y": ["bravo", "alpha"], "City": [None, "alpha"]})


class _Stub:
    """an engine that must not be reached: the refusal comes first"""

    def __init__(self, lw):
        self.lw = lw
        self.row_offset = 0


class _World2:
    rank, world = 0, 2


def test_refuses_several_ranks_and_prior_proposals():
    S = ocp.flat1()
    lw, _ = ocp.lower(S)
    tr = Trace(lw, S["n_rows"])
    cfg = InferenceConfig(1, 2)
    with pytest.raises(NotImplementedError, match="world_size > 1"):
        inf.initialize_trace(_Stub(lw), tr, cfg, 0, comm=_World2())
    with pytest.raises(NotImplementedError, match="world_size > 1"):
        inf.observed_sweep(_Stub(lw), tr, cfg, 0, 0, comm=_World2())
    with pytest.raises(NotImplementedError, match="use_dd_proposals=False"):
        Engine.sweep_own(_Stub(lw), tr, InferenceConfig(1, 2, use_dd_proposals=False), 0, 0)


# ---- host bookkeeping ----------------------------------------------------------------------------------------------
def _clean_trace(S, lw, seed=0):
    return Trace.from_clean_values(lw, {0: {"city": S["truth"]["City"], "state": S["truth"]["State"]},
                                        1: {"cond": S["truth"]["Cond"]}}, S["n_rows"], seed=seed)


def test_trace_counts_resampling_and_consistency():
    S = ocp.flat2b()
    lw, _ = ocp.lower(S)
    tr = _clean_trace(S, lw, seed=3)
    assert [a for a, _, _ in tr.own_leaves()] == ["city", "state", "cond"] and tr.own.shape == (3, S["n_rows"])
    for li, pname in ((0, "city_p"), (2, "cond_p")):
        st = tr.params[("Obs", pname)]
        assert np.array_equal(st.counts, np.bincount(tr.own[li], minlength=len(st.counts)))
        assert np.array_equal(tr.own_counts(li), st.counts)
    tr.check_consistency()
    # resample_parameters: Dirichlet(concentration + counts) from the trace's own generator, in declaration order
    import copy
    rng = copy.deepcopy(tr.rng)
    want = {p: rng.dirichlet(tr.params[("Obs", p)].alpha + tr.params[("Obs", p)].counts) for p in ("city_p", "cond_p")}
    assert tr.params[("Obs", "cond_p")].alpha[0] == 2.0
    tr.resample_parameters("Obs")
    for p, v in want.items():
        assert np.array_equal(tr.params[("Obs", p)].value, v)
    assert tr.has_parameters("Obs") and tr.has_learned_parameters("Obs")
    # a host edit is counted at the next move, and a count that is off is caught
    tr.own[0, 0] = (tr.own[0, 0] + 1) % 25
    with pytest.raises(AssertionError, match=r"Obs\.city: Dirichlet counts out of sync"):
        tr.check_consistency()
    tr.refresh_own_counts()
    tr.check_consistency()
    tr.params[("Obs", "cond_p")].counts[0] += 1
    with pytest.raises(AssertionError, match=r"Obs\.cond: Dirichlet counts out of sync"):
        tr.check_consistency()
    tr.refresh_own_counts()
    tr.own[1, 5] = -1
    with pytest.raises(AssertionError, match="some but not all"):
        tr.check_consistency()
    cp = copy.deepcopy(tr)
    assert cp._own_dev is None and np.array_equal(cp.own, tr.own) and cp.own is not tr.own


def test_evaluate_accuracy_reads_own_columns(tmp_path):
    S = ocp.flat2b(n_rows=60)
    lw, _ = ocp.lower(S)
    tr = _clean_trace(S, lw)
    clean, dirty = S["truth"], S["dirty"]
    import pandas as pd
    from pclean_amd.analysis import save_results
    d = save_results(str(tmp_path), "flat", lw, tr, dirty, timestamp=False)
    saved = pd.read_csv(f"{d}/reconstructed_Obs.csv", dtype=str)
    assert saved["City"].tolist() == clean["City"] and saved["Cond"].tolist() == clean["Cond"]
    acc = evaluate_accuracy(lw, tr, dirty, clean)
    errors = sum(d is not None and d != c for col in clean for d, c in zip(dirty[col], clean[col]))
    missing = sum(d is None for col in clean for d in dirty[col])
    assert acc["errors"] == errors == acc["changed"] == acc["cleaned"] and acc["imputed"] == missing == acc["correctly_imputed"]
    assert acc["f1"] == 1.0
    # one wrong cell: a dirty cell that was right is now changed, not cleaned
    i = next(i for i in range(60) if dirty["City"][i] == clean["City"][i])
    tr.own[0, i] = (tr.own[0, i] + 1) % 25
    acc2 = evaluate_accuracy(lw, tr, dirty, clean)
    assert acc2["changed"] == errors + 1 and acc2["cleaned"] == errors and acc2["f1"] < 1.0
    up = evaluate_accuracy_up_to(lw, tr, dirty, clean, 30)
    assert up["changed"] <= acc2["changed"] and up["errors"] == errors
    tab = reconstructed_table(lw, tr, dirty)
    assert tab["State"] == clean["State"] and tab["City"][i] != clean["City"][i]
    tr.own[:, 3] = -1
    assert reconstructed_table(lw, tr, dirty)["Cond"][3] is None
    # the device tally does not serve them: they stay with the host path, with and without own=True
    for own in (False, True):
        plan = ReconPlan(lw, own=own)
        assert plan.columns == [] and plan.host_strings == ["City", "State", "Cond"]


# ---- the exact conditional -----------------------------------------------------------------------------------------
def test_exact_conditional_is_prior_times_likelihood_on_the_strings():
    S = ocp.flat3(K=8)
    p = np.random.default_rng(0).dirichlet(np.ones(8))
    names = S["choices"]["name"]
    for i in range(0, S["n_rows"], 7):
        sc = ocp.exact_scores(S, {"p": p}, "name", i)
        a, b, c, d = (S["dirty"][col][i] for col in ("A", "B", "C", "Name"))
        for k, o in enumerate(names):
            want = math.log(p[k]) + pe.lit.add_typos_logpdf(a, o) + pe.lit.add_typos_logpdf(b, o, 2) + pe.lit.format_name_logpdf(c, o)
            if d is not None and d != o:
                want = -math.inf
            assert sc[o] == want
        pi = ocp.exact_pi(S, {"p": p}, "name", i)
        assert abs(sum(pi.values()) - 1.0) < 1e-12
        if d is not None:
            assert pi == {d: 1.0}
    none = next(i for i in range(S["n_rows"]) if all(S["dirty"][col][i] is None for col in ("A", "B", "C", "Name")))
    pi = ocp.exact_pi(S, {"p": p}, "name", none)  # nothing observed: the prior (FormatName's -5 is the same for every name)
    assert np.allclose([pi[o] for o in names], p, rtol=1e-12)


# ---- the power of the device leg's distribution test -----------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    return ocp.dist_case()


def _mutated_pis(S, params, drop_prior=False, drop_term=None):
    memo, out = {}, []
    terms = S["terms"]["name"]
    T = dict(S, terms={"name": [t for t in terms if t[0] != drop_term]})
    par = {"p": np.full(len(params["p"]), 1.0 / len(params["p"]))} if drop_prior else params
    for i in range(S["n_rows"]):
        key = tuple(S["dirty"][c][i] for c in ("A", "B", "C", "Name"))
        if key not in memo:
            memo[key] = ocp.exact_pi(T, par, "name", i)
        out.append(memo[key])
    return out


def _gof(expected, observed):
    return pe.gof([(i, e, o) for i, (e, o) in enumerate(zip(expected, observed))])


@pytest.mark.parametrize("P,mh", [(2, False), (2, True), (9, False)], ids=["P2", "P2-MH", "P9"])
def test_power_of_the_distribution_test(case, P, mh):
    S, params, _, pis, cur = case
    rng = np.random.default_rng(1000 + P + mh)
    exact = [ocp.expected_output(pi, s, P, mh) for pi, s in zip(pis, cur)]
    res = _gof(exact, ocp.sample_rows(rng, exact, pe.S_GPU))
    assert res["p"] > pe.ALPHA, pe.describe(res)
    names = S["choices"]["name"]
    shift = {o: names[(k + 1) % len(names)] for k, o in enumerate(names)}
    mutations = {
        "prior dropped": [ocp.expected_output(pi, s, P, mh) for pi, s in zip(_mutated_pis(S, params, drop_prior=True), cur)],
        "one term dropped": [ocp.expected_output(pi, s, P, mh) for pi, s in zip(_mutated_pis(S, params, drop_term="B"), cur)],
        "draw off by one": [{shift[o]: v for o, v in e.items()} for e in exact],
    }
    if not mh and P > 2:  # (at P = 2 twice the weight is all of it; MH has no 1/P)
        def heavy(pi, s):
            out = {k: (1.0 - 2.0 / P) * v for k, v in pi.items()}
            out[s] = out.get(s, 0.0) + 2.0 / P
            return out
        mutations["retained particle weighted 2/P"] = [heavy(pi, s) for pi, s in zip(pis, cur)]
    for name, dists in mutations.items():
        res = _gof(exact, ocp.sample_rows(rng, dists, pe.S_GPU))
        print(f"P={P}{' MH' if mh else ''} {name}: p = {res['p']:.3g}")
        assert res["p"] < pe.ALPHA, (name, pe.describe(res))


def test_power_without_current_values(case):
    S, params, _, pis, _ = case
    rng = np.random.default_rng(77)
    res = _gof(pis, ocp.sample_rows(rng, pis, pe.S_GPU))
    assert res["p"] > pe.ALPHA, pe.describe(res)
    for name, dists in {"prior dropped": _mutated_pis(S, params, drop_prior=True),
                        "one term dropped": _mutated_pis(S, params, drop_term="B")}.items():
        res = _gof(pis, ocp.sample_rows(rng, dists, pe.S_GPU))
        assert res["p"] < pe.ALPHA, (name, pe.describe(res))
