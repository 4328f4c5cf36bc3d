"""Flat programs with an own choice indexed by a sibling own choice (TEST INFRASTRUCTURE).

  FLATP(na, nb)   a ~ ChooseProportionally(A, pa);  b ~ ChooseProportionally(B, theta, index="a");
                  a_obs ~ AddTypos(a);  b_obs ~ AddTypos(b)        — one own block, ONE product leaf over a * |B| + b
  variant         + b_obs2 ~ AddTypos(b, 2);  a_fmt ~ FormatName(a);  `a` itself in the query (observed directly on some rows)
  TWIN            indexed_program.product_model over the same words and the same rows: the pair behind a slot `d ~ Doc`.  Its
                  new-row product leaf (block 0, node 1) is what the parent code computes, through pclean_score_node.

Words and the first rows are indexed_program.product_shape_program's (each observation exact, with a typo or missing, every
combination); then runs of RUNS identical rows and one run of LONG_RUN rows (beyond own_block.hip's OWN_RUN_SPLIT = 2048).
exact_scores() restates the joint conditional log pa[a] + log theta[a][b] + the terms from oracle/literal.py's densities on
the strings: nothing of the lowering's option order, value columns or fixed-point arithmetic."""
import math

import numpy as np

import indexed_program as ip
import posterior_exact as pe
from posterior_exact import lit
from pclean_amd.model import (AddTypos, ChooseProportionally, FormatName, IndexedProportionsParameter, LoweredModel, Model,
                              ProportionsParameter, Query)

RUNS = (1, 2, 64, 65, 300)
LONG_RUN = 2100


def model(A, B, variant=False):
    m = Model()
    o = m.add_class("Obs")
    o.param("pa", ProportionsParameter(1.0))
    o.param("theta", IndexedProportionsParameter(1.0))
    with o.block():
        o.choice("a", ChooseProportionally(A, "pa"))
        o.choice("b", ChooseProportionally(B, "theta", index="a"))
        o.choice("a_obs", AddTypos("a"))
        o.choice("b_obs", AddTypos("b"))
        if variant:
            o.choice("b_obs2", AddTypos("b", 2))
            o.choice("a_fmt", FormatName("a"))
    cols = {"Degree": ("a", "a_obs"), "Spec": ("b", "b_obs")}
    if variant:
        cols.update({"Spec2": ("b", "b_obs2"), "Fmt": ("a", "a_fmt"), "A": "a"})
    return m, Query(m, "Obs", cols)


def flatp(na, nb, seed=0, n_rows=64, long_run=True, variant=False):
    """the program, its rows and what exact_scores needs: terms {choice: [(query column, kind, max_typos)]} in declaration
    order, direct {choice: query column}"""
    P = ip.product_shape_program(na, nb, n_rows=n_rows, seed=seed)
    A, B = P["A"], P["B"]
    rng = np.random.default_rng(seed + 1000)
    dirty = {"Degree": list(P["dirty"]["Degree"]), "Spec": list(P["dirty"]["Spec"])}
    for r in RUNS + ((LONG_RUN,) if long_run else ()):
        a, b = A[int(rng.integers(na))], B[int(rng.integers(nb))]
        oa, ob = (a if r % 2 else pe._typo(rng, a)), pe._typo(rng, b) + "z" * (r % 7)  # (a tuple no other row holds)
        dirty["Degree"] += [oa] * r
        dirty["Spec"] += [ob] * r
    n = len(dirty["Degree"])
    perm = rng.permutation(n)
    dirty = {k: [v[i] for i in perm] for k, v in dirty.items()}
    terms = {"a": [("Degree", "typos", None)], "b": [("Spec", "typos", None)]}
    direct = {}
    if variant:
        pick = rng.integers(na, size=n)
        truth = [A[int(k)] for k in pick]
        # the further observations follow a hidden `a` of the row where the first ones are missing or agree with it
        dirty["Spec2"] = [None if i % 5 == 1 else (pe._typo(rng, B[int(rng.integers(nb))]) if i % 2 else B[int(rng.integers(nb))])
                          for i in range(n)]
        dirty["Fmt"] = [None if i % 3 == 2 else (truth[i].upper() if i % 2 else truth[i][0] + ".") for i in range(n)]
        dirty["A"] = [truth[i] if i % 6 == 0 else None for i in range(n)]
        terms = {"a": [("Degree", "typos", None), ("Fmt", "format", None)], "b": [("Spec", "typos", None), ("Spec2", "typos", 2)]}
        direct = {"a": "A"}
    m, q = model(A, B, variant)
    return dict(model=m, query=q, dirty=dirty, A=A, B=B, n_rows=n, terms=terms, direct=direct, variant=variant)


def lower(S):
    lw = LoweredModel(S["model"], S["query"], S["dirty"])
    return lw, lw.encode_observations(S["dirty"])


def twin(S):
    """indexed_program.product_model over the same words and rows (the plain FLATP only): (lowered, observations, leaf)"""
    assert not S["variant"]
    m = ip.product_model(degrees=S["A"], specs=S["B"])
    lw = LoweredModel(m, ip.product_query(m), S["dirty"])
    return lw, lw.encode_observations(S["dirty"]), (0, 1)


def draw_params(S, seed):
    """(pa [na], theta [na][nb]) with unequal vectors per index value"""
    rng = np.random.default_rng(seed)
    na, nb = len(S["A"]), len(S["B"])
    return rng.dirichlet(np.ones(na)), rng.dirichlet(np.full(nb, 0.7), size=na)


def exact_scores(S, pa, theta, i):
    """{(a, b): log pa[a] + log theta[a][b] + the log densities of row i's observations}, on the strings"""
    d = S["dirty"]
    ta = [sum(lit.add_typos_logpdf(d[c][i], a, mt) if kind == "typos" else lit.format_name_logpdf(d[c][i], a)
              for c, kind, mt in S["terms"]["a"]) for a in S["A"]]
    tb = [sum(lit.add_typos_logpdf(d[c][i], b, mt) if kind == "typos" else lit.format_name_logpdf(d[c][i], b)
              for c, kind, mt in S["terms"]["b"]) for b in S["B"]]
    out = {}
    for ka, a in enumerate(S["A"]):
        for kb, b in enumerate(S["B"]):
            s = math.log(pa[ka]) + math.log(theta[ka][kb]) + ta[ka] + tb[kb]
            for ch, col in S["direct"].items():
                if d[col][i] is not None and d[col][i] != (a if ch == "a" else b):
                    s = -math.inf
            out[(a, b)] = s
    return out


def exact_matrix(S, pa, theta, rows):
    """exact_scores of `rows` as float64 [len(rows)][na * nb] in the grid's order a * nb + b, one evaluation per distinct
    observed tuple"""
    cols = list(S["dirty"])
    memo, out = {}, np.empty((len(rows), len(S["A"]) * len(S["B"])))
    for t, i in enumerate(rows):
        key = tuple(S["dirty"][c][i] for c in cols)
        if key not in memo:
            sc = exact_scores(S, pa, theta, i)
            memo[key] = np.array([sc[(a, b)] for a in S["A"] for b in S["B"]])
        out[t] = memo[key]
    return out


def planted(n_rows=1200, na=20, nb=4, seed=7):
    """b is a function of a (b = B[index of a mod nb]); every a has n_rows / na rows; on every tenth row OF EACH a b's
    observation is missing and a's is clean (`hidden`); the other rows observe both, clean or with one typo.  Words of 14-17
    letters, pairwise far apart."""
    rng = np.random.default_rng(seed)
    A = pe._words(rng, na, 14, 18)
    B = pe._words(rng, nb, 14, 18, taken=A)
    perm = rng.permutation(n_rows)
    ka = (np.arange(n_rows) % na)[perm]
    hidden = ((np.arange(n_rows) // na) % 10 == 0)[perm]
    truth_a = [A[int(k)] for k in ka]
    truth_b = [B[int(k) % nb] for k in ka]
    dirty = {"Degree": [], "Spec": []}
    for i in range(n_rows):
        if hidden[i]:
            dirty["Degree"].append(truth_a[i])
            dirty["Spec"].append(None)
        else:
            dirty["Degree"].append(truth_a[i] if rng.random() < 0.6 else pe._typo(rng, truth_a[i]))
            dirty["Spec"].append(truth_b[i] if rng.random() < 0.6 else pe._typo(rng, truth_b[i]))
    m, q = model(A, B)
    return dict(model=m, query=q, dirty=dirty, A=A, B=B, n_rows=n_rows, truth={"Degree": truth_a, "Spec": truth_b},
                hidden=hidden, variant=False, terms={"a": [("Degree", "typos", None)], "b": [("Spec", "typos", None)]}, direct={})
