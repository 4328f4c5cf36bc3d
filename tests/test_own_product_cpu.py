"""An own choice indexed by a sibling own choice (flat classes), host side: the lowered plan, the refusals, the layout of
Trace.own and its joint device encoding, the counts, the parameter moves and the readers of the cleaned table."""
import json
import os

import numpy as np
import pytest

import own_choice_program as ocp
import own_product_program as opp
from pclean_amd import _lib
from pclean_amd.analysis import evaluate_accuracy, reconstructed_table
from pclean_amd.engine import option_prior
from pclean_amd.model import (OWN_MAX_OPTIONS, AddTypos, ChooseProportionally, ChooseUniformly, IndexedProportionsParameter,
                              LoweredModel, Model, ProportionsParameter, Query, Unmodeled)
from pclean_amd.trace import IndexedProportionsState, ProportionsState, Trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "own_flat_plans.json")
WORDS = ["alpha", "bravo", "charlie", "delta"]


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def test_plain_plan_is_one_leaf_on_the_two_column_table():
    S = opp.flatp(3, 4, long_run=False)
    lw, obs = opp.lower(S)
    assert lw.flat and len(lw.blocks) == 1
    nodes, terms = lw.own_block_arrays(0)
    assert len(nodes) == 1 and nodes[0]["kind"] == _lib.NODE_LEAF and nodes[0]["table"] == lw.option_id[("Obs", "b")]
    assert (nodes[0]["term_begin"], nodes[0]["n_terms"], nodes[0]["parent"]) == (0, 2, -1)
    oi = lw.obs_index
    assert [(t["obs_col"], t["cand_col"], t["dens_kind"]) for t in terms] == [
        (oi["a_obs"], 0, _lib.DENS_ADD_TYPOS), (oi["b_obs"], 1, _lib.DENS_ADD_TYPOS)]
    assert lw.indexed == {("Obs", "b"): ("product", "a")} and lw.product_index == {("Obs", "a"): "b"}
    assert lw.own_product == {"b": "a"} and lw.own_leaf == {"a": (0, 0), "b": (0, 0)}
    cols = lw.option_cols[("Obs", "b")]
    assert np.array_equal(cols, [np.repeat(np.arange(3), 4), np.tile(np.arange(4), 3)])  # key-major: a * |B| + b
    assert lw.blocks[0]["node_info"][0]["product"] == ("a", "b")
    tr = Trace(lw, S["n_rows"], 0)
    assert [x[0] for x in tr.own_leaves()] == ["a", "b"] and tr.own.shape == (2, S["n_rows"])
    assert tr.own_pairs() == {1: 0} and tr.own_device_leaves() == [(0, 0, (0, 1))]
    assert isinstance(tr.params[("Obs", "pa")], ProportionsState) and tr.params[("Obs", "pa")].counts.shape == (3,)
    assert isinstance(tr.params[("Obs", "theta")], IndexedProportionsState) and tr.params[("Obs", "theta")].counts.shape == (3, 4)
    # the joint prior: log pa[a] + log theta[a][b], added in that order, bit for bit
    pa, th = opp.draw_params(S, 3)
    tr.params[("Obs", "pa")].value, tr.params[("Obs", "theta")].value = pa, th
    want = (np.log(pa)[:, None] + np.log(th)).reshape(-1)
    assert np.array_equal(option_prior(lw, tr, "Obs", "b").view(np.uint64), want.view(np.uint64))


def test_variant_plan_orders_the_terms_by_choice_then_declaration_equality_last():
    S = opp.flatp(5, 3, long_run=False, variant=True)
    lw, _ = opp.lower(S)
    nodes, terms = lw.own_block_arrays(0)
    oi = lw.obs_index
    assert len(nodes) == 1 and nodes[0]["n_terms"] == 5
    assert [(t["obs_col"], t["cand_col"], t["dens_kind"], t["max_typos"]) for t in terms] == [
        (oi["a_obs"], 0, _lib.DENS_ADD_TYPOS, -1), (oi["a_fmt"], 0, _lib.DENS_TABULATED, -1), (oi["a"], 0, _lib.DENS_EQUAL, -1),
        (oi["b_obs"], 1, _lib.DENS_ADD_TYPOS, -1), (oi["b_obs2"], 1, _lib.DENS_ADD_TYPOS, 2)]


def test_other_choices_of_the_block_stay_separable_leaves():
    m = Model()
    o = m.add_class("Obs")
    o.param("pa", ProportionsParameter(1.0))
    o.param("pc", ProportionsParameter(1.0))
    o.param("theta", IndexedProportionsParameter(1.0))
    with o.block():
        o.choice("a", ChooseProportionally(WORDS, "pa"))
        o.choice("c", ChooseProportionally(WORDS[:3], "pc"))
        o.choice("b", ChooseProportionally(WORDS[:2], "theta", index="a"))
        o.choice("u", ChooseUniformly(WORDS))
        for x in "acbu":
            o.choice(x + "_obs", AddTypos(x))
    q = Query(m, "Obs", {x.upper(): (x, x + "_obs") for x in "acbu"})
    lw = LoweredModel(m, q, {x.upper(): ["alpha", None] for x in "acbu"})
    nodes, terms = lw.own_block_arrays(0)
    assert [n["table"] for n in nodes] == [lw.option_id[("Obs", x)] for x in "cbu"]
    assert [(n["term_begin"], n["n_terms"]) for n in nodes] == [(0, 1), (1, 2), (3, 1)]
    assert [t["cand_col"] for t in terms] == [0, 0, 1, 0]
    assert lw.own_leaf == {"c": (0, 0), "a": (0, 1), "b": (0, 1), "u": (0, 2)}
    tr = Trace(lw, 2, 0)
    assert [x[0] for x in tr.own_leaves()] == ["c", "a", "b", "u"]
    assert tr.own_device_leaves() == [(0, 0, (0,)), (0, 1, (1, 2)), (0, 2, (3,))]


def _describe(lw):
    out = []
    for bi in range(len(lw.blocks)):
        nodes, terms = lw.own_block_arrays(bi)
        out.append(dict(nodes=[np.asarray(list(n)).tolist() for n in nodes], terms=[np.asarray(list(t)).tolist() for t in terms]))
    return dict(blocks=out, own_leaf={k: list(v) for k, v in lw.own_leaf.items()},
                option_id={f"{c}.{a}": i for (c, a), i in lw.option_id.items()}, obs_cols=list(lw.obs_cols))


def test_programs_without_a_product_leaf_lower_as_before():
    """tests/golden/own_flat_plans.json: the plans of the flat programs of own_choice_program as the code lowered them before
    own choices could be indexed"""
    want = json.load(open(GOLDEN))
    for name, S in (("flat1", ocp.flat1()), ("flat3", ocp.flat3()), ("flat2b", ocp.flat2b())):
        lw, _ = ocp.lower(S)
        assert _describe(lw) == want[name], name
        assert lw.own_product == {} and lw.indexed == {}
        tr = Trace(lw, S["n_rows"], 0)
        assert tr.own_pairs() == {} and [r for _, _, r in tr.own_device_leaves()] == [(li,) for li in range(len(tr.own_leaves()))]


# ---- the refusals -----------------------------------------------------------------------------------------------------------
def _program(build, cols, dirty=None):
    m = Model()
    o = m.add_class("Obs")
    o.param("pa", ProportionsParameter(1.0))
    o.param("theta", IndexedProportionsParameter(1.0))
    build(m, o)
    q = Query(m, "Obs", cols)
    return LoweredModel(m, q, dirty or {c: ["alpha", None] for c in cols})


def test_refusals_by_name():
    def uniform(m, o):
        with o.block():
            o.choice("a", ChooseUniformly(WORDS))
            o.choice("b", ChooseProportionally(WORDS, "theta", index="a"))
            o.choice("y", AddTypos("b"))
    with pytest.raises(NotImplementedError, match=r"Obs\.b: an indexed choice among the observed class's own choices is not "
                                                  r"lowered when its index \(a\) is a ChooseUniformly choice"):
        _program(uniform, {"Y": ("b", "y")})

    def slot(m, o):
        d = m.add_class("Doc")
        d.choice("k", Unmodeled())
        o.fk("d", "Doc")
        with o.block():
            o.choice("a", ChooseProportionally(WORDS, "pa"))
            o.choice("b", ChooseProportionally(WORDS, "theta", index="a"))
            o.choice("y", AddTypos("b"))
    with pytest.raises(NotImplementedError, match=r"Obs\.b: an indexed own choice in a class with a reference-slot block \(d\)"):
        _program(slot, {"Y": ("b", "y"), "K": "d.k"})

    def keyed(m, o):
        with o.block():
            o.choice("a", Unmodeled())
            o.choice("b", ChooseProportionally(WORDS, "theta", index="a"))
            o.choice("y", AddTypos("b"))
    with pytest.raises(NotImplementedError, match=r"Obs\.b: the index a is observed directly and is not a choice \(the keyed form\)"):
        _program(keyed, {"Y": ("b", "y"), "A": "a"}, {"Y": ["alpha", None], "A": ["x", "y"]})

    def nested(m, o):
        o.param("theta2", IndexedProportionsParameter(1.0))
        with o.block():
            o.choice("a", ChooseProportionally(WORDS, "pa"))
            o.choice("b", ChooseProportionally(WORDS, "theta", index="a"))
            o.choice("c", ChooseProportionally(WORDS, "theta2", index="b"))
            o.choice("y", AddTypos("c"))
    with pytest.raises(NotImplementedError, match=r"Obs\.c: the index b is itself indexed"):
        _program(nested, {"Y": ("c", "y")})

    def two(m, o):
        o.param("theta2", IndexedProportionsParameter(1.0))
        with o.block():
            o.choice("a", ChooseProportionally(WORDS, "pa"))
            o.choice("b", ChooseProportionally(WORDS, "theta", index="a"))
            o.choice("c", ChooseProportionally(WORDS, "theta2", index="a"))
            o.choice("y", AddTypos("c"))
    with pytest.raises(NotImplementedError, match=r"Obs\.c: a already indexes b; two dependents on one index"):
        _program(two, {"Y": ("c", "y")})

    def other_block(m, o):
        with o.block():
            o.choice("a", ChooseProportionally(WORDS, "pa"))
            o.choice("x", AddTypos("a"))
        with o.block():
            o.choice("b", ChooseProportionally(WORDS, "theta", index="a"))
            o.choice("y", AddTypos("b"))
    with pytest.raises(NotImplementedError, match=r"Obs\.b: the index a is declared in another block"):
        _program(other_block, {"X": ("a", "x"), "Y": ("b", "y")})

    def between(m, o):
        with o.block():
            o.choice("a", ChooseProportionally(WORDS, "pa"))
            o.choice("x", AddTypos("a"))
            o.choice("b", ChooseProportionally(WORDS, "theta", index="a"))
            o.choice("y", AddTypos("b"))
    with pytest.raises(NotImplementedError, match=r"Obs\.b: x, declared between the index a and the choice, reads the index"):
        _program(between, {"X": ("a", "x"), "Y": ("b", "y")})

    def after(m, o):
        with o.block():
            o.choice("b", ChooseProportionally(WORDS, "theta", index="a"))
            o.choice("a", ChooseProportionally(WORDS, "pa"))
            o.choice("y", AddTypos("b"))
    with pytest.raises(NotImplementedError, match=r"Obs\.b: the index a must be declared before the choice"):
        _program(after, {"Y": ("b", "y")})


def test_a_grid_beyond_the_option_limit_is_refused_at_lowering():
    na = OWN_MAX_OPTIONS // 2 + 1
    big = [f"w{k}" for k in range(na)]

    def build(m, o):
        with o.block():
            o.choice("a", ChooseProportionally(big, "pa"))
            o.choice("b", ChooseProportionally(WORDS[:2], "theta", index="a"))
            o.choice("y", AddTypos("b"))
    with pytest.raises(NotImplementedError, match=rf"Obs\.b: the product with a has {na} x 2 = {2 * na} options, more than the "
                                                  rf"{OWN_MAX_OPTIONS} an own option list holds"):
        _program(build, {"Y": ("b", "y")})


# ---- Trace.own, counts, parameter moves -------------------------------------------------------------------------------------
class _FakeHip:
    """set_own / get_own / own_counts of a device that holds what it was given"""

    def __init__(self):
        self.vals = {}

    def set_own(self, block, vals):
        self.vals[block] = np.array(vals, dtype=np.int32)

    def get_own(self, block, n_nodes, n_rows):
        assert self.vals[block].shape == (n_nodes, n_rows)
        return self.vals[block].copy()

    def own_counts(self, block, node, k):
        v = self.vals[block][node]
        return np.bincount(v[v >= 0], minlength=k).astype(np.int64)


def _fake_engine():
    from pclean_amd.engine import Engine
    eng = object.__new__(Engine)
    eng.hip = _FakeHip()
    return eng


def test_own_round_trip_through_the_joint_encoding():
    S = opp.flatp(5, 3, long_run=False)
    lw, _ = opp.lower(S)
    n = S["n_rows"]
    tr = Trace(lw, n, 0)
    rng = np.random.default_rng(0)
    own = np.stack([rng.integers(5, size=n), rng.integers(3, size=n)]).astype(np.int32)
    own[:, ::7] = -1
    tr.own = own.copy()
    eng = _fake_engine()
    eng._push_own(tr)
    dev = eng.hip.vals[0]
    assert dev.shape == (1, n) and np.array_equal(dev[0], np.where(own[0] < 0, -1, own[0] * 3 + own[1]))
    tr._own[:] = 0
    eng.pull_own(tr)
    assert np.array_equal(tr._own, own)
    # the counts while the device is ahead: the joint histogram, reshaped, and its row sums
    tr._own_dev = eng
    tr.refresh_own_counts()
    tr._own_dev = None
    want = np.zeros((5, 3), dtype=np.int64)
    ok = own[0] >= 0
    np.add.at(want, (own[0][ok], own[1][ok]), 1)
    assert np.array_equal(tr.params[("Obs", "theta")].counts, want)
    assert np.array_equal(tr.params[("Obs", "pa")].counts, want.sum(axis=1))
    tr.check_consistency()
    # ... and from the host array
    tr.params[("Obs", "theta")].counts[:] = 0
    tr.params[("Obs", "pa")].counts[:] = 0
    tr.refresh_own_counts()
    assert np.array_equal(tr.params[("Obs", "theta")].counts, want) and np.array_equal(tr.params[("Obs", "pa")].counts, want.sum(axis=1))
    # a row with only one of the two set
    bad = own.copy()
    bad[1, 3] = -1 if bad[1, 3] >= 0 else 0
    bad[0, 3] = 2 if bad[1, 3] < 0 else -1
    tr.own = bad
    with pytest.raises(ValueError, match=r"row 3: only one of the own choices a and b is set"):
        _fake_engine()._push_own(tr)


def test_resample_moves_both_parameters():
    S = opp.flatp(4, 3, long_run=False)
    lw, _ = opp.lower(S)
    n = S["n_rows"]
    tr = Trace(lw, n, 5)
    tr.own = np.stack([np.arange(n) % 4, np.arange(n) % 3]).astype(np.int32)
    pa0, th0 = tr.params[("Obs", "pa")].value.copy(), tr.params[("Obs", "theta")].value.copy()
    tr.resample_parameters("Obs")
    pa1, th1 = tr.params[("Obs", "pa")].value, tr.params[("Obs", "theta")].value
    assert pa1.shape == (4,) and th1.shape == (4, 3) and not np.array_equal(pa0, pa1) and not np.array_equal(th0, th1)
    assert np.allclose(pa1.sum(), 1.0) and np.allclose(th1.sum(axis=1), 1.0)
    assert tr.params[("Obs", "theta")].counts.sum() == n and tr.params[("Obs", "pa")].counts.sum() == n


def test_from_clean_values_reads_back_as_the_truth():
    S = opp.planted(n_rows=120, na=6)
    lw, _ = opp.lower(S)
    n = S["n_rows"]
    tr = Trace.from_clean_values(lw, {0: {"a": S["truth"]["Degree"], "b": S["truth"]["Spec"]}}, n)
    tr.check_consistency()
    assert [lw.latent_dom[("Obs", "a")].string(int(k)) for k in tr.own[0]] == S["truth"]["Degree"]
    table = reconstructed_table(lw, tr, S["dirty"])
    assert table["Degree"] == S["truth"]["Degree"] and table["Spec"] == S["truth"]["Spec"]
    acc = evaluate_accuracy(lw, tr, S["dirty"], S["truth"])
    assert acc["f1"] == 1.0 and acc["cleaned"] == acc["errors"] > 0 and acc["correctly_imputed"] == acc["imputed"] > 0
    th = tr.params[("Obs", "theta")].counts
    assert th.sum() == n and (np.count_nonzero(th, axis=1) == 1).all()  # b is a function of a


# ---- several ranks, prior proposals -------------------------------------------------------------------------------------------
class _Stub:
    """an engine that must not be reached: the refusal comes first"""

    def __init__(self, lw):
        self.lw = lw
        self.row_offset = 0


class _World2:
    rank, world = 0, 2


def test_refuses_several_ranks_and_prior_proposals_with_a_product_leaf():
    from pclean_amd import inference as inf
    from pclean_amd.engine import Engine, InferenceConfig
    S = opp.flatp(3, 4, long_run=False)
    lw, _ = opp.lower(S)
    assert lw.own_product == {"b": "a"}
    tr = Trace(lw, S["n_rows"])
    cfg = InferenceConfig(1, 2)
    with pytest.raises(NotImplementedError, match="world_size > 1"):
        inf.initialize_trace(_Stub(lw), tr, cfg, 0, comm=_World2())
    with pytest.raises(NotImplementedError, match="world_size > 1"):
        inf.observed_sweep(_Stub(lw), tr, cfg, 0, 0, comm=_World2())
    with pytest.raises(NotImplementedError, match="world_size > 1"):
        inf.run_inference(_Stub(lw), tr, cfg, 0, comm=_World2())
    with pytest.raises(NotImplementedError, match="use_dd_proposals=False"):
        Engine.sweep_own(_Stub(lw), tr, InferenceConfig(1, 2, use_dd_proposals=False), 0, 0)
    assert (tr.own == -1).all()  # nothing was swept
