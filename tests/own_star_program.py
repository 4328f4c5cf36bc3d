"""Flat programs with SEVERAL own choices indexed by one sibling own choice: a star (TEST INFRASTRUCTURE).

  STARP(ka, (k1 .. kD))   a ~ ChooseProportionally(A, pa);  b_j ~ ChooseProportionally(B_j, theta_j, index="a");
                          a_obs ~ AddTypos(a);  b_j_obs ~ AddTypos(b_j)     — one own block, lowered with own_star=True to a
                          head node and D arm nodes
  variant                 + b0_obs2 ~ AddTypos(b0, 2);  a_fmt ~ FormatName(a);  `a` itself in the query (observed directly on
                          some rows);  the LAST arm has no observation at all
  HEAD TWIN               the same `a` with its observations and no dependents: a plain option list whose scores are
                          H(a) = log pa[a] + the head's terms, the part of S(a) the device never reports on its own

Words lie pairwise far apart (pe._words); the first rows hold every combination of exact / one typo / missing per
observation; then runs of RUNS identical rows and one of LONG_RUN rows (beyond own_block.hip's OWN_RUN_SPLIT = 2048).
exact_parts() restates the factors of the joint conditional from oracle/literal.py's densities on the strings;
definition() restates the contract of the star (include/pclean_hip.h) on the device's fp64 scores."""
import itertools
import json
import math
import os
import sys

import numpy as np

if __name__ == "__main__":  # (the child of the skip test: started as a script)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import posterior_exact as pe
from posterior_exact import lit
from pclean_amd.model import (AddTypos, ChooseProportionally, FormatName, IndexedProportionsParameter, LoweredModel, Model,
                              ProportionsParameter, Query)

RUNS = (1, 2, 64, 65, 300)
LONG_RUN = 2100
TWO_M40 = 9.094947017729282379150390625e-13  # 2^-40


def model(A, Bs, variant=False, dependents=True):
    m = Model()
    o = m.add_class("Obs")
    o.param("pa", ProportionsParameter(1.0))
    D = len(Bs) if dependents else 0
    for j in range(D):
        o.param(f"theta{j}", IndexedProportionsParameter(1.0))
    observed = [j for j in range(D) if not (variant and j == D - 1)]
    with o.block():
        o.choice("a", ChooseProportionally(A, "pa"))
        for j in range(D):
            o.choice(f"b{j}", ChooseProportionally(Bs[j], f"theta{j}", index="a"))
        o.choice("a_obs", AddTypos("a"))
        for j in observed:
            o.choice(f"b{j}_obs", AddTypos(f"b{j}"))
        if variant:
            if D:
                o.choice("b0_obs2", AddTypos("b0", 2))
            o.choice("a_fmt", FormatName("a"))
    cols = {"Ca": ("a", "a_obs")}
    for j in observed:
        cols[f"C{j}"] = (f"b{j}", f"b{j}_obs")
    if variant:
        if D:
            cols["C0x"] = ("b0", "b0_obs2")
        cols.update({"Fmt": ("a", "a_fmt"), "A": "a"})
    return m, Query(m, "Obs", cols)


def starp(ka, ks, seed=0, long_run=True, variant=False, runs=RUNS):
    """the program, its rows and what exact_parts needs: terms {choice: [(query column, kind, max_typos)]} in declaration
    order, direct {choice: query column}"""
    rng = np.random.default_rng(seed)
    D = len(ks)
    A = pe._words(rng, ka, 10, 14)
    Bs, taken = [], list(A)
    for k in ks:
        Bs.append(pe._words(rng, k, 10, 14, taken=taken))
        taken += Bs[-1]
    observed = [j for j in range(D) if not (variant and j == D - 1)]
    cols = ["Ca"] + [f"C{j}" for j in observed]
    dirty = {c: [] for c in cols}
    words = {"Ca": A, **{f"C{j}": Bs[j] for j in observed}}
    for combo in itertools.product((0, 1, 2), repeat=len(cols)):  # exact / one typo / missing, every combination
        for c, how in zip(cols, combo):
            w = words[c][int(rng.integers(len(words[c])))]
            dirty[c].append(w if how == 0 else pe._typo(rng, w) if how == 1 else None)
    for r in tuple(runs) + ((LONG_RUN,) if long_run else ()):
        for c in cols:
            w = words[c][int(rng.integers(len(words[c])))]
            dirty[c] += [(w if r % 2 and c == "Ca" else pe._typo(rng, w)) + ("z" * (r % 7) if c != "Ca" else "")] * r
    n = len(dirty["Ca"])
    perm = rng.permutation(n)
    dirty = {k: [v[i] for i in perm] for k, v in dirty.items()}
    terms = {"a": [("Ca", "typos", None)], **{f"b{j}": ([(f"C{j}", "typos", None)] if j in observed else []) for j in range(D)}}
    direct = {}
    if variant:
        truth = [A[int(k)] for k in rng.integers(ka, size=n)]
        dirty["C0x"] = [None if i % 5 == 1 else (pe._typo(rng, Bs[0][int(rng.integers(ks[0]))]) if i % 2 else Bs[0][int(rng.integers(ks[0]))])
                        for i in range(n)]
        dirty["Fmt"] = [None if i % 3 == 2 else (truth[i].upper() if i % 2 else truth[i][0] + ".") for i in range(n)]
        dirty["A"] = [truth[i] if i % 6 == 0 else None for i in range(n)]
        terms["a"] = [("Ca", "typos", None), ("Fmt", "format", None)]
        terms["b0"] = [("C0", "typos", None), ("C0x", "typos", 2)]
        direct = {"a": "A"}
    m, q = model(A, Bs, variant)
    return dict(model=m, query=q, dirty=dirty, A=A, Bs=Bs, n_rows=n, terms=terms, direct=direct, variant=variant)


def lower(S, own_star=True):
    lw = LoweredModel(S["model"], S["query"], S["dirty"], own_star=own_star)
    return lw, lw.encode_observations(S["dirty"])


def head_twin(S):
    """the index alone, with its observations: (lowered, observations); its one leaf scores H(a)"""
    m, q = model(S["A"], S["Bs"], S["variant"], dependents=False)
    dirty = {c: v for c, v in S["dirty"].items() if c in q.obsmap}
    lw = LoweredModel(m, q, dirty)
    return lw, lw.encode_observations(dirty)


def draw_params(S, seed):
    """(pa [ka], [theta_j [ka][kj]]) with unequal vectors per index value"""
    rng = np.random.default_rng(seed)
    ka = len(S["A"])
    return rng.dirichlet(np.ones(ka)), [rng.dirichlet(np.full(len(B), 0.7), size=ka) for B in S["Bs"]]


def _term(kind, obs, val, mt):
    return lit.add_typos_logpdf(obs, val, mt) if kind == "typos" else lit.format_name_logpdf(obs, val)


def exact_parts(S, pa, thetas, i):
    """(H [ka], [T_j [ka][kj]]) of row i on the strings: H(a) = log pa[a] + the log densities of the observations of a (-inf
    where a directly observed a differs), T_j(a, b) = log theta_j[a][b] + those of b_j.  The joint conditional of
    (a, b_1 .. b_D) is H(a) + sum_j T_j(a, b_j)."""
    d = S["dirty"]
    H = np.array([math.log(pa[k]) + sum(_term(kind, d[c][i], a, mt) for c, kind, mt in S["terms"]["a"]) for k, a in enumerate(S["A"])])
    col = S["direct"].get("a")
    if col is not None and d[col][i] is not None:
        H[[k for k, a in enumerate(S["A"]) if a != d[col][i]]] = -math.inf
    T = []
    for j, B in enumerate(S["Bs"]):
        tb = np.array([sum(_term(kind, d[c][i], b, mt) for c, kind, mt in S["terms"][f"b{j}"]) for b in B])
        with np.errstate(divide="ignore"):
            T.append(np.log(np.asarray(thetas[j], dtype=np.float64)) + tb[None, :])
    return H, T


def exact_scores(S, pa, thetas, i):
    """{(a, b_1 .. b_D): joint log score} of row i on the strings (small shapes)"""
    H, T = exact_parts(S, pa, thetas, i)
    out = {}
    for k, a in enumerate(S["A"]):
        for bs in itertools.product(*[range(len(B)) for B in S["Bs"]]):
            out[(a,) + tuple(S["Bs"][j][b] for j, b in enumerate(bs))] = float(H[k] + sum(T[j][k, b] for j, b in enumerate(bs)))
    return out


def _lse_fix(hip, M, V):
    """pclean_lse_from_fix on arrays: M + log(V 2^-40) through the device's own log, -inf where V == 0"""
    V = np.asarray(V, dtype=np.float64)
    x = np.where(V > 0, V * TWO_M40, 1.0)
    lg = hip.debug_detmath(np.ascontiguousarray(x).ravel())[1].reshape(x.shape)
    with np.errstate(invalid="ignore"):
        return np.where(V > 0, M + lg, -np.inf)


def _fixw(hip, d):
    d = np.asarray(d, dtype=np.float64)
    return hip.debug_detmath(np.ascontiguousarray(d).ravel())[2].reshape(d.shape)


def definition(hip, H, ts, rows, seed, sweep, n_draws, sites):
    """The star's contract on fp64 scores of ONE observed tuple: H [ka] (the head's own part), ts [t_j [ka][kj]].  Returns
    dict(S [ka], lse, L [D][ka], u [ka] uint64, U int, v [D] of [ka][kj] uint64, V [D] of [ka] Python ints,
    a [len(rows)][n_draws], b [D][len(rows)][n_draws]) — fixw and log through the device's pclean_detmath, sums and the 128-bit
    products in Python integers."""
    ka, D = len(H), len(ts)
    S = np.array(H, dtype=np.float64)
    Ls, vs, Vs = [], [], []
    for t in ts:
        M = t.max(axis=1)
        with np.errstate(invalid="ignore"):
            v = np.where(np.isneginf(M)[:, None], np.uint64(0), _fixw(hip, t - M[:, None]))
        V = [sum(row.tolist()) for row in v]
        L = _lse_fix(hip, M, V)
        S = S + L  # (arm order)
        Ls.append(L)
        vs.append(v)
        Vs.append(V)
    m = S.max()
    with np.errstate(invalid="ignore"):
        u = np.zeros(ka, dtype=np.uint64) if np.isneginf(m) else _fixw(hip, S - m)
    U = sum(u.tolist())
    lse = float(_lse_fix(hip, np.array([m]), [U])[0])
    cum = np.cumsum(u, dtype=np.uint64)
    a_out = np.full((len(rows), n_draws), ka - 1, dtype=np.int64)
    b_out = [np.full((len(rows), n_draws), t.shape[1] - 1, dtype=np.int64) for t in ts]
    for p in range(n_draws):
        R = hip.debug_rand64(seed, np.asarray(rows, dtype=np.uint32), sites[0], p, sweep)
        Rj = [hip.debug_rand64(seed, np.asarray(rows, dtype=np.uint32), sites[1 + j], p, sweep) for j in range(D)]
        for r in range(len(rows)):
            if not U:
                continue
            a = int(np.searchsorted(cum, np.uint64((int(R[r]) * U) >> 64), side="right"))
            a_out[r, p] = a
            for j in range(D):
                cj = np.cumsum(vs[j][a], dtype=np.uint64)
                b_out[j][r, p] = int(np.searchsorted(cj, np.uint64((int(Rj[j][r]) * Vs[j][a]) >> 64), side="right"))
    return dict(S=S, lse=lse, L=Ls, u=u, U=U, v=vs, V=Vs, a=a_out, b=b_out)


def planted(n_rows=1200, ka=20, ks=(4, 5), seed=7):
    """b_j is a function of a (b_j = B_j[index of a mod k_j]); every a has n_rows / ka rows; on every tenth row OF EACH a one
    or both dependents' observations are missing and a's is clean (`hidden` [D][n]); the other rows observe everything, clean
    or with one typo.  Words of 14-17 letters, pairwise far apart."""
    rng = np.random.default_rng(seed)
    A = pe._words(rng, ka, 14, 18)
    Bs, taken = [], list(A)
    for k in ks:
        Bs.append(pe._words(rng, k, 14, 18, taken=taken))
        taken += Bs[-1]
    perm = rng.permutation(n_rows)
    ia = (np.arange(n_rows) % ka)[perm]
    tenth = ((np.arange(n_rows) // ka) % 10 == 0)[perm]
    which = ((np.arange(n_rows) // (10 * ka)) % 3)[perm]  # 0: the first is hidden, 1: the second, 2: both
    hidden = np.array([tenth & (which != 1), tenth & (which != 0)])
    truth = {"Ca": [A[int(k)] for k in ia], **{f"C{j}": [Bs[j][int(k) % ks[j]] for k in ia] for j in range(2)}}
    dirty = {c: [] for c in truth}
    for i in range(n_rows):
        for c in truth:
            w = truth[c][i]
            if c != "Ca" and hidden[int(c[1]), i]:
                dirty[c].append(None)
            elif tenth[i]:
                dirty[c].append(w)
            else:
                dirty[c].append(w if rng.random() < 0.6 else pe._typo(rng, w))
    m, q = model(A, Bs)
    return dict(model=m, query=q, dirty=dirty, A=A, Bs=Bs, n_rows=n_rows, truth=truth, hidden=hidden, variant=False,
                terms={"a": [("Ca", "typos", None)], "b0": [("C0", "typos", None)], "b1": [("C1", "typos", None)]}, direct={})


def skip_case(seed=3):
    """SKIP: 40 index values, arms of 6 and 5.  Three rows of interest — `far`: every observation exact (the head's string is
    far from all but one a: most a are skipped); `none`: every observation missing (B(a) - S(a) <= log 6 + log 5, nothing
    is skipped); `loose`: the head's observation missing and arm 0's exact at B_0[2], with theta_0[5] moved onto b = 0 but for
    e^-36 on b = 2 — S(5) lies more than 31 below m while its bound (the row maximum of theta_0[5], near 0) stays within a few
    nats of m: it is weighed and its weight is 0."""
    rng = np.random.default_rng(seed)
    S = starp(40, (6, 5), seed=seed, long_run=False, runs=(3,))
    A, Bs = S["A"], S["Bs"]
    for c, w in (("Ca", [A[3], None, None]), ("C0", [Bs[0][1], None, Bs[0][2]]), ("C1", [Bs[1][4], None, None])):
        S["dirty"][c] += w
    n = S["n_rows"]
    S["n_rows"] = n + 3
    S["model"], S["query"] = model(A, Bs)
    pa = rng.uniform(0.5, 1.5, size=40)
    pa /= pa.sum()
    ths = [rng.dirichlet(np.full(len(B), 5.0), size=40) for B in Bs]
    ths[0][5] = 0.0
    ths[0][5][2] = math.exp(-36.0)
    ths[0][5][0] = 1.0 - ths[0][5][2]
    return S, pa, ths, dict(far=n, none=n + 1, loose=n + 2)


def run_skip_case():
    """the skip case on the device: probes of the three rows (head without scores, every arm) and one sweep of all rows;
    JSON-serialisable, doubles as their bit patterns"""
    from pclean_amd.engine import Engine, InferenceConfig
    from pclean_amd.trace import Trace
    S, pa, ths, rows = skip_case()
    lw, obs = lower(S)
    eng = Engine(lw, obs, dist_mode=1)
    try:
        tr = Trace(lw, S["n_rows"], 0)
        tr.params[("Obs", "pa")].value = pa
        for j, th in enumerate(ths):
            tr.params[("Obs", f"theta{j}")].value = th
        eng.upload_trace(tr)
        eng.hip.set_active_rows(0, S["n_rows"])
        out = {}
        for name, r in rows.items():
            q = np.array([r], dtype=np.int32)
            lse, _, dr = eng.hip.score_own(0, 0, q, seed=17, sweep=2, n_draws=3)
            st = eng.hip.get_own_stats()
            res = dict(lse=[int(x) for x in lse.view(np.uint64)], a=dr.tolist(), weighed=int(st.star_weighed),
                       skipped=int(st.star_skipped), variants=int(st.variants))
            for j in range(len(ths)):
                lj, _, bj = eng.hip.score_own(0, 1 + j, q, seed=17, sweep=2, n_draws=3)
                res[f"lse{j}"] = [int(x) for x in lj.view(np.uint64)]
                res[f"b{j}"] = bj.tolist()
            out[name] = res
        chosen, logml = eng.sweep_own(tr, InferenceConfig(1, 3), 23, 1)
        st = eng.hip.get_own_stats()
        out["sweep"] = dict(vals=tr.own.tolist(), logml=[int(x) for x in logml.view(np.uint64)], chosen=chosen.tolist(),
                            skipped=int(st.star_skipped), weighed=int(st.star_weighed))
        return out
    finally:
        eng.close()


if __name__ == "__main__":
    print("RESULT " + json.dumps(run_skip_case()))
