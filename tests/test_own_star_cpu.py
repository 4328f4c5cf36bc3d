"""Several dependents on one index in a flat class (own_star=True), host side: the lowered plan, the refusals, Trace.own and
the counts, the contract restated in float64 against the literal densities, and the grid rule of pclean_link_own_star under
sanitizers (a program of its own: tests/own_star_host)."""
import itertools
import json
import math
import os
import subprocess

import numpy as np
import pytest

import own_choice_program as ocp
import own_product_program as opp
import own_star_program as osp
import posterior_exact as pe
from pclean_amd import _lib
from pclean_amd.engine import Engine, InferenceConfig, option_prior
from pclean_amd.model import (OWN_MAX_OPTIONS, OWN_STAR_LDS_MAX, OWN_STAR_MAX_ARMS, OWN_STAR_MAX_K, AddNoise, AddTypos,
                              ChooseProportionally, ChooseUniformly, IndexedLookup, IndexedMeanParameter,
                              IndexedProportionsParameter, LoweredModel, Model, ProportionsParameter, Query, Unmodeled)
from pclean_amd.trace import IndexedProportionsState, Trace

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "own_flat_plans.json")
SRC = os.path.join(HERE, "own_star_host", "own_star_host.cpp")
WORDS = ["alpha", "bravo", "charlie", "delta"]


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def test_star_plan_is_a_head_and_one_arm_per_dependent():
    S = osp.starp(3, (4, 2), long_run=False)
    lw, obs = osp.lower(S)
    assert lw.flat and len(lw.blocks) == 1
    nodes, terms = lw.own_block_arrays(0)
    assert [n["kind"] for n in nodes] == [_lib.NODE_LEAF] * 3
    assert [n["table"] for n in nodes] == [lw.option_id[("Obs", x)] for x in ("a", "b0", "b1")]
    assert [(n["term_begin"], n["n_terms"], n["parent"]) for n in nodes] == [(0, 1, -1), (1, 1, -1), (2, 1, -1)]
    oi = lw.obs_index
    assert [(t["obs_col"], t["cand_col"], t["dens_kind"]) for t in terms] == [
        (oi["a_obs"], 0, _lib.DENS_ADD_TYPOS), (oi["b0_obs"], 1, _lib.DENS_ADD_TYPOS), (oi["b1_obs"], 1, _lib.DENS_ADD_TYPOS)]
    assert lw.indexed == {("Obs", "b0"): ("star", "a"), ("Obs", "b1"): ("star", "a")}
    assert lw.product_index == {} and lw.own_product == {} and lw.star_index == {("Obs", "a"): ["b0", "b1"]}
    assert lw.own_leaf == {"a": (0, 0), "b0": (0, 1), "b1": (0, 2)} and lw.own_star == {(0, 0): [1, 2]}
    assert ("Obs", "a") not in lw.option_cols and np.array_equal(lw.option_values[("Obs", "a")], np.arange(3))
    assert np.array_equal(lw.option_cols[("Obs", "b0")], [np.repeat(np.arange(3), 4), np.tile(np.arange(4), 3)])  # key-major
    assert np.array_equal(lw.option_cols[("Obs", "b1")], [np.repeat(np.arange(3), 2), np.tile(np.arange(2), 3)])
    assert [i["star"] for i in lw.blocks[0]["node_info"]] == [("a", ("b0", "b1"))] * 3
    tr = Trace(lw, S["n_rows"], 0)
    assert [x[0] for x in tr.own_leaves()] == ["a", "b0", "b1"] and tr.own.shape == (3, S["n_rows"])
    assert tr.own_pairs() == {} and tr.own_stars() == {0: [1, 2]}
    assert tr.own_device_leaves() == [(0, 0, (0,)), (0, 1, (1,)), (0, 2, (2,))]  # one row of `own` per node: no joint encoding
    assert isinstance(tr.params[("Obs", "theta0")], IndexedProportionsState) and tr.params[("Obs", "theta1")].counts.shape == (3, 2)
    # an arm's prior is log theta_j[a][b] ALONE, key-major; log pa belongs to the head
    pa, ths = osp.draw_params(S, 3)
    tr.params[("Obs", "pa")].value = pa
    for j, th in enumerate(ths):
        tr.params[("Obs", f"theta{j}")].value = th
        assert np.array_equal(option_prior(lw, tr, "Obs", f"b{j}").view(np.uint64), np.log(th).reshape(-1).view(np.uint64))
    assert np.array_equal(option_prior(lw, tr, "Obs", "a").view(np.uint64), np.log(pa).view(np.uint64))
    # relower keeps the flag
    lw.relower({})
    assert lw.own_star_enabled and lw.own_star == {(0, 0): [1, 2]}


def test_variant_plan_orders_the_terms_by_node_then_declaration_equality_last():
    S = osp.starp(5, (7, 3), long_run=False, variant=True)
    lw, _ = osp.lower(S)
    nodes, terms = lw.own_block_arrays(0)
    oi = lw.obs_index
    assert [(n["term_begin"], n["n_terms"]) for n in nodes] == [(0, 3), (3, 2), (5, 0)]  # (the last arm observes nothing)
    assert [(t["obs_col"], t["cand_col"], t["dens_kind"], t["max_typos"]) for t in terms] == [
        (oi["a_obs"], 0, _lib.DENS_ADD_TYPOS, -1), (oi["a_fmt"], 0, _lib.DENS_TABULATED, -1), (oi["a"], 0, _lib.DENS_EQUAL, -1),
        (oi["b0_obs"], 1, _lib.DENS_ADD_TYPOS, -1), (oi["b0_obs2"], 1, _lib.DENS_ADD_TYPOS, 2)]


def test_other_choices_of_the_block_follow_the_star():
    m = Model()
    o = m.add_class("Obs")
    for p in ("pa", "pc"):
        o.param(p, ProportionsParameter(1.0))
    for p in ("t0", "t1"):
        o.param(p, IndexedProportionsParameter(1.0))
    with o.block():
        o.choice("c", ChooseProportionally(WORDS[:3], "pc"))
        o.choice("a", ChooseProportionally(WORDS, "pa"))
        o.choice("b0", ChooseProportionally(WORDS[:2], "t0", index="a"))
        o.choice("u", ChooseUniformly(WORDS))
        o.choice("b1", ChooseProportionally(WORDS[:3], "t1", index="a"))
        for x in ("c", "a", "b0", "u", "b1"):
            o.choice(x + "_obs", AddTypos(x))
    q = Query(m, "Obs", {x.upper(): (x, x + "_obs") for x in ("c", "a", "b0", "u", "b1")})
    lw = LoweredModel(m, q, {x.upper(): ["alpha", None] for x in ("c", "a", "b0", "u", "b1")}, own_star=True)
    nodes, _ = lw.own_block_arrays(0)
    assert [n["table"] for n in nodes] == [lw.option_id[("Obs", x)] for x in ("c", "a", "b0", "b1", "u")]
    assert lw.own_star == {(0, 1): [2, 3]} and lw.own_leaf == {"c": (0, 0), "a": (0, 1), "b0": (0, 2), "b1": (0, 3), "u": (0, 4)}


def test_one_dependent_with_the_flag_is_the_product_plan():
    S = opp.flatp(3, 4, long_run=False)
    plain = LoweredModel(S["model"], S["query"], S["dirty"])
    star = LoweredModel(S["model"], S["query"], S["dirty"], own_star=True)
    for f in ("indexed", "product_index", "own_product", "own_leaf", "option_id"):
        assert getattr(plain, f) == getattr(star, f), f
    assert star.own_star == {} and star.star_index == {}
    for x, y in zip(plain.own_block_arrays(0), star.own_block_arrays(0)):
        assert np.array_equal(x, y)


def _describe(lw):
    out = []
    for bi in range(len(lw.blocks)):
        nodes, terms = lw.own_block_arrays(bi)
        out.append(dict(nodes=[np.asarray(list(n)).tolist() for n in nodes], terms=[np.asarray(list(t)).tolist() for t in terms]))
    return dict(blocks=out, own_leaf={k: list(v) for k, v in lw.own_leaf.items()},
                option_id={f"{c}.{a}": i for (c, a), i in lw.option_id.items()}, obs_cols=list(lw.obs_cols))


def test_programs_without_an_index_lower_as_before_with_the_flag():
    want = json.load(open(GOLDEN))
    for name, S in (("flat1", ocp.flat1()), ("flat3", ocp.flat3()), ("flat2b", ocp.flat2b())):
        lw = LoweredModel(S["model"], S["query"], S["dirty"], own_star=True)
        assert _describe(lw) == want[name], name
        assert lw.own_star == {} and lw.indexed == {}


# ---- the refusals -----------------------------------------------------------------------------------------------------------
def _program(build, cols, dirty=None, own_star=True, params=4):
    m = Model()
    o = m.add_class("Obs")
    o.param("pa", ProportionsParameter(1.0))
    for j in range(params + 2):
        o.param(f"t{j}", IndexedProportionsParameter(1.0))
    build(m, o)
    q = Query(m, "Obs", cols)
    return LoweredModel(m, q, dirty or {c: ["alpha", None] for c in cols}, own_star=own_star)


def _star(ka_words, deps, head_obs=1, extra=None):
    def build(m, o):
        with o.block():
            o.choice("a", ChooseProportionally(ka_words, "pa"))
            for j, w in enumerate(deps):
                o.choice(f"b{j}", ChooseProportionally(w, f"t{j}", index="a"))
            for k in range(head_obs):
                o.choice(f"x{k}", AddTypos("a"))
            for j in range(len(deps)):
                o.choice(f"y{j}", AddTypos(f"b{j}"))
            if extra:
                extra(m, o)
    cols = {f"X{k}": ("a", f"x{k}") for k in range(head_obs)}
    cols.update({f"Y{j}": (f"b{j}", f"y{j}") for j in range(len(deps))})
    return build, cols


def test_flag_off_gives_the_pinned_message():
    build, cols = _star(WORDS, [WORDS, WORDS])
    with pytest.raises(NotImplementedError, match=r"Obs\.b1: a already indexes b0; two dependents on one index are not lowered"):
        _program(build, cols, own_star=False)
    assert _program(build, cols).own_star == {(0, 0): [1, 2]}


def test_refusals_by_name():
    big = [f"w{k}" for k in range(OWN_STAR_MAX_K + 1)]
    build, cols = _star(WORDS, [WORDS] * (OWN_STAR_MAX_ARMS + 1))
    with pytest.raises(NotImplementedError, match=r"Obs\.a: 5 dependents on one index \(b0, b1, b2, b3, b4\); a star holds at most 4"):
        _program(build, cols)
    assert len(_program(*_star(WORDS, [WORDS] * OWN_STAR_MAX_ARMS)).own_star[(0, 0)]) == 4

    build, cols = _star(big, [WORDS[:2], WORDS[:2]])
    with pytest.raises(NotImplementedError, match=r"Obs\.a: 4097 options; the index and the dependents of a star hold at most 4096"):
        _program(build, cols)
    build, cols = _star(WORDS[:2], [WORDS[:2], big])
    with pytest.raises(NotImplementedError, match=r"Obs\.b1: 4097 options; the index and the dependents of a star hold at most 4096"):
        _program(build, cols)

    build, cols = _star(big[:4096], [WORDS[:2], big[:65]])
    with pytest.raises(NotImplementedError, match=rf"Obs\.b1: the product with a has 4096 x 65 = {4096 * 65} options, more than the "
                                                  rf"{OWN_MAX_OPTIONS} an own option list holds"):
        _program(build, cols)

    # the cached values: 4 head terms of 4096 values, S(a) and its chunk sums exceed the LDS of a workgroup
    build, cols = _star(big[:4096], [WORDS[:2], WORDS[:2]], head_obs=4)
    need = 8 * (4 * 4096 + 2 + 2 + 4096 + 64)
    assert need > OWN_STAR_LDS_MAX >= 8 * (3 * 4096 + 2 + 2 + 4096 + 64)
    with pytest.raises(NotImplementedError, match=rf"Obs\.a: the star with b0, b1 caches {need} bytes of term values, more than the "
                                                  rf"{OWN_STAR_LDS_MAX} of a workgroup's LDS"):
        _program(build, cols)
    assert _program(*_star(big[:4096], [WORDS[:2], WORDS[:2]], head_obs=3)).own_star

    build, cols = _star(WORDS, [WORDS, WORDS], head_obs=_lib.MAX_TERMS - 1)
    with pytest.raises(NotImplementedError, match=rf"Obs\.a: the star with b0, b1 carries more than {_lib.MAX_TERMS} terms"):
        _program(build, cols)

    def chain(m, o):
        with o.block():
            o.choice("a", ChooseProportionally(WORDS, "pa"))
            o.choice("b", ChooseProportionally(WORDS, "t0", index="a"))
            o.choice("c", ChooseProportionally(WORDS, "t1", index="b"))
            o.choice("y", AddTypos("c"))
    with pytest.raises(NotImplementedError, match=r"Obs\.c: the index b is itself indexed"):
        _program(chain, {"Y": ("c", "y")})

    def uniform(m, o):
        with o.block():
            o.choice("a", ChooseUniformly(WORDS))
            o.choice("b", ChooseProportionally(WORDS, "t0", index="a"))
            o.choice("c", ChooseProportionally(WORDS, "t1", index="a"))
            o.choice("y", AddTypos("b"))
    with pytest.raises(NotImplementedError, match=r"Obs\.b: an indexed choice among the observed class's own choices is not "
                                                  r"lowered when its index \(a\) is a ChooseUniformly choice"):
        _program(uniform, {"Y": ("b", "y")})

    def keyed(m, o):
        with o.block():
            o.choice("a", Unmodeled())
            o.choice("b", ChooseProportionally(WORDS, "t0", index="a"))
            o.choice("c", ChooseProportionally(WORDS, "t1", index="a"))
            o.choice("y", AddTypos("b"))
    with pytest.raises(NotImplementedError, match=r"Obs\.b: the index a is observed directly and is not a choice \(the keyed form\)"):
        _program(keyed, {"Y": ("b", "y"), "A": "a"}, {"Y": ["alpha", None], "A": ["x", "y"]})

    def other_block(m, o):
        with o.block():
            o.choice("a", ChooseProportionally(WORDS, "pa"))
            o.choice("b", ChooseProportionally(WORDS, "t0", index="a"))
            o.choice("x", AddTypos("a"))
        with o.block():
            o.choice("c", ChooseProportionally(WORDS, "t1", index="a"))
            o.choice("y", AddTypos("c"))
    with pytest.raises(NotImplementedError, match=r"Obs\.c: the index a is declared in another block"):
        _program(other_block, {"X": ("a", "x"), "Y": ("c", "y")})

    def between(m, o):
        with o.block():
            o.choice("a", ChooseProportionally(WORDS, "pa"))
            o.choice("b", ChooseProportionally(WORDS, "t0", index="a"))
            o.choice("x", AddTypos("a"))
            o.choice("c", ChooseProportionally(WORDS, "t1", index="a"))
            o.choice("y", AddTypos("c"))
    with pytest.raises(NotImplementedError, match=r"Obs\.c: x, declared between the index a and the choice, reads the index"):
        _program(between, {"X": ("a", "x"), "Y": ("c", "y")})

    def gauss(m, o):
        o.param("avg", IndexedMeanParameter(0.0, 10.0))
        with o.block():
            o.choice("a", ChooseProportionally(WORDS, "pa"))
            o.choice("b", ChooseProportionally(WORDS, "t0", index="a"))
            o.choice("c", ChooseProportionally(WORDS, "t1", index="a"))
            o.julia("base", IndexedLookup("avg"), ["a"])
            o.choice("x", AddNoise("base", 1.0))
    with pytest.raises(NotImplementedError, match=r"Obs\.a: a factor of a Gaussian observation that is itself indexed, or that "
                                                  r"indexes a sibling choice, is not lowered"):
        _program(gauss, {"A": "a", "X": "x"}, {"A": ["alpha", "bravo"], "X": [1.0, 2.0]})


def test_several_ranks_and_prior_proposals_are_refused_before_the_device_is_touched():
    S = osp.starp(3, (4, 2), long_run=False)
    lw, _ = osp.lower(S)
    tr = Trace(lw, S["n_rows"], 0)
    eng = object.__new__(Engine)
    eng.lw = lw
    with pytest.raises(NotImplementedError, match="use_dd_proposals=False"):
        eng.sweep_own(tr, InferenceConfig(1, 2, use_dd_proposals=False), 1, 0)
    eng._dev_comm = True
    with pytest.raises(NotImplementedError, match="several ranks"):
        eng.sweep_own(tr, InferenceConfig(1, 2), 1, 0)


# ---- Trace.own and the counts -------------------------------------------------------------------------------------------------
def test_counts_from_host_arrays_equal_a_literal_tally():
    S = osp.starp(5, (3, 4), long_run=False)
    lw, _ = osp.lower(S)
    n = S["n_rows"]
    tr = Trace(lw, n, 0)
    rng = np.random.default_rng(0)
    own = np.stack([rng.integers(5, size=n), rng.integers(3, size=n), rng.integers(4, size=n)]).astype(np.int32)
    own[:, ::7] = -1
    tr.own = own.copy()
    tr.refresh_own_counts()
    pa, t0, t1 = np.zeros(5, np.int64), np.zeros((5, 3), np.int64), np.zeros((5, 4), np.int64)
    for i in range(n):
        if own[0, i] >= 0:
            pa[own[0, i]] += 1
            t0[own[0, i], own[1, i]] += 1
            t1[own[0, i], own[2, i]] += 1
    assert np.array_equal(tr.params[("Obs", "pa")].counts, pa)
    assert np.array_equal(tr.params[("Obs", "theta0")].counts, t0) and np.array_equal(tr.params[("Obs", "theta1")].counts, t1)
    assert np.array_equal(tr.own_counts(1), t0) and np.array_equal(tr.own_counts(0), pa)
    tr.check_consistency()
    tr.params[("Obs", "theta1")].counts[0, 0] += 1
    with pytest.raises(AssertionError, match=r"Obs\.b1: Dirichlet counts out of sync"):
        tr.check_consistency()


def test_a_partly_set_row_of_a_star_is_refused():
    S = osp.starp(5, (3, 4), long_run=False)
    lw, _ = osp.lower(S)
    tr = Trace(lw, S["n_rows"], 0)
    own = np.zeros((3, S["n_rows"]), dtype=np.int32)
    own[:, 3] = -1  # (all unset: fine)
    tr.own = own.copy()
    own[2, 6] = -1
    with pytest.raises(ValueError, match=r"row 6: only some of the own choices a, b0, b1 of one star are set \(a, b0\)"):
        tr.own = own


# ---- the contract in float64 --------------------------------------------------------------------------------------------------
def _fixw(d):
    """pclean_fixw in plain float64 (math.exp in place of the library's exp: the bound below covers the difference)"""
    return 0 if not d >= -28.5 else (1 << 40 if d >= 0 else int(math.exp(d) * 2.0 ** 40))


def _contract(H, T):
    """the contract of the star on float64 factors: (lse, {(a, b_1 .. b_D) option indices: probability})"""
    ka = len(H)
    S, vs, Vs = np.array(H, dtype=np.float64), [], []
    for t in T:
        M = t.max(axis=1)
        v = [[0 if M[a] == -math.inf else _fixw(float(x - M[a])) for x in t[a]] for a in range(ka)]
        V = [sum(r) for r in v]
        S = S + np.array([M[a] + math.log(V[a] * 2.0 ** -40) if V[a] else -math.inf for a in range(ka)])
        vs.append(v)
        Vs.append(V)
    m = S.max()
    u = [_fixw(float(s - m)) for s in S]
    U = sum(u)
    lse = m + math.log(U * 2.0 ** -40)
    probs = {}
    for a in range(ka):
        if not u[a]:
            continue
        for bs in itertools.product(*[range(t.shape[1]) for t in T]):
            p = u[a] / U
            for j, b in enumerate(bs):
                p *= vs[j][a][b] / Vs[j][a]
            probs[(a,) + bs] = p
    return lse, probs


def test_the_contract_restated_in_float64_meets_the_exact_joint_conditional():
    """lse and every joint probability (u_a / U) prod_j v_j(a, b_j) / V_j(a) against exact_scores (mpmath when it imports).

    Bound.  A fixed-point weight floor(exp(d) 2^40) lies at most 2^-40 below exp(d) in units of the maximum weight 2^40 = 1,
    so with w_j = exp(t_j - M_j): |V_j 2^-40 - sum_b w_j| <= K_j 2^-40 against a sum >= 1 (the maximum's weight is exactly
    1), and L_j, the exact log-sum-exp's restatement, is off by at most K_j 2^-40 (|log(1 + x)| <= |x| (1 + |x|)) plus the
    roundings of exp, log and the additions, a few 1e-16 relative.  S(a) adds D such errors: |S(a) - S*(a)| <= E =
    sum_j K_j 2^-40 + 1e-12.  u_a = floor(exp(S(a) - m) 2^40): U 2^-40 is a sum >= 1 whose terms are off by the factor
    exp(+-2E) (both S(a) and m move) and by 2^-40 each, so |lse - lse*| <= 2 E + K_a 2^-40, within
    (K_a + 2 sum_j K_j) 2^-40 + 1e-12 (1 + |lse*|).  A probability p = (u_a / U) prod_j v_j / V_j <= 1: each ratio x / X has
    X >= 2^40, |dx| <= 1 unit + the shift, |dX| <= K units, so its absolute error is at most (K + 1) 2^-40 (+ 2E for u_a / U),
    and a product of factors <= 1 moves by at most the sum of its factors' errors: |p - p*| <= (K_a + 1 + 2 sum_j K_j) 2^-40
    + sum_j (K_j + 1) 2^-40 + 1e-12 <= (K_a + 3 sum_j K_j + D + 1) 2^-40 + 1e-12.  The device is not involved: this shows the
    definition itself meets the exact conditional."""
    worst_l, worst_p = 0.0, 0.0
    for ka, ks, variant in [(3, (2, 2), False), (4, (5, 3), False), (5, (3, 2), True)]:
        S = osp.starp(ka, ks, seed=9, long_run=False, variant=variant, runs=(1,))
        pa, ths = osp.draw_params(S, 12)
        seen = set()
        for i in range(S["n_rows"]):
            key = tuple(S["dirty"][c][i] for c in S["dirty"])
            if key in seen or len(seen) >= 40:
                continue
            seen.add(key)
            H, T = osp.exact_parts(S, pa, ths, i)
            lse, probs = _contract(H, T)
            sc = osp.exact_scores(S, pa, ths, i)
            z, pi = pe.log_marginal(sc), pe.normalise(sc)
            bl = (ka + 2 * sum(ks)) * 2.0 ** -40 + 1e-12 * (1 + abs(z))
            bp = (ka + 3 * sum(ks) + len(ks) + 1) * 2.0 ** -40 + 1e-12
            worst_l = max(worst_l, abs(lse - z) / bl)
            for idx in itertools.product(range(ka), *[range(k) for k in ks]):
                name = (S["A"][idx[0]],) + tuple(S["Bs"][j][b] for j, b in enumerate(idx[1:]))
                worst_p = max(worst_p, abs(probs.get(idx, 0.0) - pi.get(name, 0.0)) / bp)
    print(f"\n[star contract] lse error / bound {worst_l:.3g}, probability error / bound {worst_p:.3g}")
    assert worst_l <= 1.0 and worst_p <= 1.0


# ---- the grid rule under sanitizers ---------------------------------------------------------------------------------------------
def test_grid_rule_of_the_link_under_sanitizers(tmp_path):
    exe = str(tmp_path / "own_star_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert lines[-1] == "all cases passed" and "ok 1x7" in lines and "ok 7x1" in lines and "ok 1x1" in lines, lines[-5:]
