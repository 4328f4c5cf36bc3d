"""Flat programs — observed classes all of whose blocks are own blocks — and their exact conditionals (TEST INFRASTRUCTURE).

  FLAT1   city ~ ChooseProportionally(words, p);  y ~ AddTypos(city)
  FLAT3   name ~ ChooseProportionally(names, p);  a ~ AddTypos(name);  b ~ AddTypos(name, 2);  c ~ FormatName(name);
          and `name` itself in the query: a direct observation on some rows.  Every term is missing in some rows, all of
          them in some.
  FLAT2B  block 0: city ~ ChooseProportionally, state ~ ChooseUniformly, one AddTypos observation each (two separable
          choices); block 1: cond ~ ChooseProportionally; cond_obs ~ AddTypos(cond, 3)
  TWIN    the same choice moved into a one-attribute latent class behind a slot: `A: x ~ ChooseProportionally(..)`,
          `Obs: r ~ A; <the same observations of r.x>` — its new-row leaf (block 0, node 1) is what the parent code
          computes for the same rows.

Data: seeded NumPy strings in the style of posterior_exact._words / _typo.  exact_scores() builds the conditional
pi(o) ~ lp[o] + sum of the terms from oracle/literal.py's densities on the strings: nothing of the product's lowering."""
import math

import numpy as np

import posterior_exact as pe
from posterior_exact import lit
from pclean_amd.model import (AddTypos, ChooseProportionally, ChooseUniformly, FormatName, LoweredModel, Model,
                              ProportionsParameter, Query)

RUNS = (1, 2, 64, 65, 300)  # rows that share one observed tuple (the lengths of the static runs the kernel groups)


def _shuffled(rng, cols):
    n = len(next(iter(cols.values())))
    perm = rng.permutation(n)
    return {k: [v[i] for i in perm] for k, v in cols.items()}


def _spec(model, query, dirty, choices, terms, direct=None):
    """choices {own choice: options}; terms {own choice: [(query column, kind, max_typos)]} in declaration order;
    direct {own choice: query column of its direct observation}"""
    return dict(model=model, query=query, dirty=dirty, choices=choices, terms=terms, direct=direct or {},
                n_rows=len(next(iter(dirty.values()))))


def flat1(K=40, seed=0, filler=40, wl=(6, 10)):
    """one choice over K words, one AddTypos observation; the rows hold runs of RUNS identical observations, `filler` rows
    with an observation of their own (clean or with a typo) and two rows without one"""
    rng = np.random.default_rng(seed)
    words = pe._words(rng, K, *wl)
    col = []
    for r in RUNS:
        col += [pe._typo(rng, words[int(rng.integers(K))])] * r
    seen = set(col)
    while len(col) < sum(RUNS) + filler:
        w = words[int(rng.integers(K))]
        o = w if rng.random() < 0.5 else pe._typo(rng, w)
        if o not in seen:
            seen.add(o)
            col.append(o)
    col += [None, None]
    dirty = _shuffled(rng, {"Y": col})
    m = Model()
    o = m.add_class("Obs")
    o.param("p", ProportionsParameter(1.0))
    with o.block():
        o.choice("city", ChooseProportionally(words, "p"))
        o.choice("y", AddTypos("city"))
    q = Query(m, "Obs", {"Y": ("city", "y")})
    return _spec(m, q, dirty, {"city": words}, {"city": [("Y", "typos", None)]})


def twin1(S):
    """TWIN of flat1(..): the same words, the same rows"""
    words = S["choices"]["city"]
    m = Model()
    a = m.add_class("A")
    a.param("p", ProportionsParameter(1.0))
    a.choice("x", ChooseProportionally(words, "p"))
    o = m.add_class("Obs")
    o.fk("r", "A")
    o.choice("y", AddTypos("r.x"))
    return dict(model=m, query=Query(m, "Obs", {"Y": ("r.x", "y")}), dirty=S["dirty"], n_rows=S["n_rows"], leaf=(0, 1))


def _flat3_data(K, seed, n_free, wl):
    rng = np.random.default_rng(seed)
    names = [w.capitalize() for w in pe._words(rng, K, *wl)]

    def row(kind):
        t = int(rng.integers(K))
        w = names[t]
        a = w if rng.random() < 0.5 else pe._typo(rng, w)
        b = pe._typo(rng, w) if rng.random() < 0.7 else pe._typo(rng, pe._typo(rng, pe._typo(rng, w)))
        c = [w, w.upper(), w[0] + ".", w[0].lower() + ".", pe._typo(rng, w)][int(rng.integers(5))]
        d = w if kind == "direct" else None
        if kind == "none":
            a = b = c = None
        elif kind == "a":
            b = c = None
        elif kind == "b":
            a = c = None
        elif kind == "c":
            a = b = None
        elif kind == "ab":
            c = None
        return a, b, c, d

    rows = []
    for r in RUNS:
        rows += [row("abc")] * r
    kinds = ["abc", "abc", "ab", "a", "b", "c", "none", "direct"]
    for i in range(n_free):
        rows.append(row(kinds[i % len(kinds)]))
    cols = {"A": [r[0] for r in rows], "B": [r[1] for r in rows], "C": [r[2] for r in rows], "Name": [r[3] for r in rows]}
    return names, _shuffled(rng, cols)


def flat3(K=30, seed=1, n_free=64, wl=(5, 9)):
    names, dirty = _flat3_data(K, seed, n_free, wl)
    m = Model()
    o = m.add_class("Obs")
    o.param("p", ProportionsParameter(1.0))
    with o.block():
        o.choice("name", ChooseProportionally(names, "p"))
        o.choice("a", AddTypos("name"))
        o.choice("b", AddTypos("name", 2))
        o.choice("c", FormatName("name"))
    q = Query(m, "Obs", {"A": ("name", "a"), "B": ("name", "b"), "C": ("name", "c"), "Name": "name"})
    return _spec(m, q, dirty, {"name": names},
                 {"name": [("A", "typos", None), ("B", "typos", 2), ("C", "format", None)]}, direct={"name": "Name"})


def twin3(S):
    names = S["choices"]["name"]
    m = Model()
    a = m.add_class("A")
    a.param("p", ProportionsParameter(1.0))
    a.choice("x", ChooseProportionally(names, "p"))
    o = m.add_class("Obs")
    o.fk("r", "A")
    o.choice("a", AddTypos("r.x"))
    o.choice("b", AddTypos("r.x", 2))
    o.choice("c", FormatName("r.x"))
    q = Query(m, "Obs", {"A": ("r.x", "a"), "B": ("r.x", "b"), "C": ("r.x", "c"), "Name": "r.x"})
    return dict(model=m, query=q, dirty=S["dirty"], n_rows=S["n_rows"], leaf=(0, 1))


def flat2b(n_rows=400, seed=2, kc=25, ks=6, kd=12, planted=False):
    """two own blocks, the first with two separable choices.  planted: every observation is the clean string or one typo
    away from it, so that (with words of 14-17 letters, pairwise far apart) the true option takes all of the mass"""
    rng = np.random.default_rng(seed)
    lo, hi = (14, 18) if planted else (6, 10)
    cities = pe._words(rng, kc, lo, hi)
    states = pe._words(rng, ks, lo, hi, taken=cities)
    conds = pe._words(rng, kd, lo, hi, taken=cities + states)
    truth = dict(city=[cities[int(i)] for i in rng.integers(kc, size=n_rows)],
                 state=[states[int(i)] for i in rng.integers(ks, size=n_rows)],
                 cond=[conds[int(i)] for i in rng.integers(kd, size=n_rows)])

    def noisy(w, p_missing):
        u = rng.random()
        if u < p_missing:
            return None
        return w if u < 0.6 else pe._typo(rng, w)
    pm = 0.0 if planted else 0.08
    dirty = {"City": [noisy(w, pm) for w in truth["city"]], "State": [noisy(w, pm) for w in truth["state"]],
             "Cond": [noisy(w, pm) for w in truth["cond"]]}
    m = Model()
    o = m.add_class("Obs")
    o.param("city_p", ProportionsParameter(1.0))
    o.param("cond_p", ProportionsParameter(2.0))
    with o.block():
        o.choice("city", ChooseProportionally(cities, "city_p"))
        o.choice("state", ChooseUniformly(states))
        o.choice("city_obs", AddTypos("city"))
        o.choice("state_obs", AddTypos("state"))
    with o.block():
        o.choice("cond", ChooseProportionally(conds, "cond_p"))
        o.choice("cond_obs", AddTypos("cond", 3))
    q = Query(m, "Obs", {"City": ("city", "city_obs"), "State": ("state", "state_obs"), "Cond": ("cond", "cond_obs")})
    S = _spec(m, q, dirty, {"city": cities, "state": states, "cond": conds},
              {"city": [("City", "typos", None)], "state": [("State", "typos", None)], "cond": [("Cond", "typos", 3)]})
    S["truth"] = {"City": truth["city"], "State": truth["state"], "Cond": truth["cond"]}
    return S


def lower(S):
    lw = LoweredModel(S["model"], S["query"], S["dirty"])
    obs = lw.encode_observations(S["dirty"])
    return lw, obs


def param_of(S, choice):
    """name of the ProportionsParameter behind an own choice, None for ChooseUniformly"""
    d = S["model"].classes[S["query"].cls].attr(choice).dist
    return d.param if isinstance(d, ChooseProportionally) else None


def exact_scores(S, params, choice, i):
    """{option: log prior + log likelihood of row i's observations} of one own choice, from the literal interpreter's
    densities on the strings; params {parameter name: probability vector}"""
    cls = S["query"].cls
    attr = S["model"].classes[cls].attr(choice)
    lt = lit.LitTrace(S["model"])
    for k, v in params.items():
        lt.params[(cls, k)] = list(v)
    options, lps, _ = lit.discrete_proposal(lt, cls, attr)
    out = {}
    seen = S["direct"].get(choice)
    for o, lp in zip(options, lps):
        s = lp
        for col, kind, mt in S["terms"][choice]:
            x = S["dirty"][col][i]
            s += lit.add_typos_logpdf(x, o, mt) if kind == "typos" else lit.format_name_logpdf(x, o)
        if seen is not None and S["dirty"][seen][i] is not None and S["dirty"][seen][i] != o:
            s = -math.inf
        out[o] = s
    return out


def exact_pi(S, params, choice, i):
    return pe.normalise(exact_scores(S, params, choice, i))


# ---- the exact-distribution case (tests/test_gpu_own_choice.py) and the sampler its power is measured with ---------------
def dist_case(seed=5, K=12):
    """FLAT3 over short names (3-4 letters: several options within a typo or two of most observations), a fixed parameter
    vector, the exact conditional of every row and a current value per row drawn from it"""
    S = flat3(K=K, seed=seed, n_free=96, wl=(3, 5))
    rng = np.random.default_rng(seed + 100)
    params = {"p": rng.dirichlet(np.full(K, 1.0))}
    memo, pis, scores = {}, [], []
    for i in range(S["n_rows"]):
        key = tuple(S["dirty"][c][i] for c in ("A", "B", "C", "Name"))
        if key not in memo:
            sc = exact_scores(S, params, "name", i)
            memo[key] = (sc, pe.normalise(sc))
        scores.append(memo[key][0])
        pis.append(memo[key][1])
    names = S["choices"]["name"]
    cur = [names[int(rng.choice(K, p=[pis[i].get(o, 0.0) for o in names]))] for i in range(S["n_rows"])]
    return S, params, scores, pis, cur


def expected_output(pi, s, P, mh):
    """output distribution of one sweep for a row of a flat class: every particle carries the same weight"""
    if s is None:
        return dict(pi)
    return pe.mh_one_block(pi, s) if mh else pe.pg_one_block(pi, s, P)


def sample_rows(rng, dists, n):
    """n draws per row from dists [{candidate: probability}] -> [{candidate: count}]"""
    out = []
    for d in dists:
        keys = list(d)
        p = np.array([d[k] for k in keys], dtype=np.float64)
        cnt = rng.multinomial(n, p / p.sum())
        out.append({k: int(c) for k, c in zip(keys, cnt) if c})
    return out


# ---- a plain-NumPy sequential restatement of the sampler for a flat class (the end-to-end test's other side) ----------
def sequential_flat(vocab, dirty, clean, n_iters, P, seed, rejuv=50, concentration=1.0):
    """The reference's schedule for one own block per column (experiments.flat_model), row by row in float64: the row's
    value is drawn from its exact conditional theta[o] exp(loglik[o]) (initialisation: always; a sweep: kept with 1/P, the
    retained particle of equally weighted particles), the counts follow, and every `rejuv` rows every parameter is drawn
    from Dirichlet(concentration + counts).  Returns the cell accuracy of the final table."""
    rng = np.random.default_rng(seed)
    cols = list(vocab)
    n = len(dirty[cols[0]])
    lik, code = {}, {}
    for c in cols:
        seen = list(dict.fromkeys(dirty[c]))
        idx = {v: j for j, v in enumerate(seen)}
        code[c] = np.array([idx[v] for v in dirty[c]])
        lik[c] = np.exp(np.array([[lit.add_typos_logpdf(v, o) for o in vocab[c]] for v in seen]))
    theta = {c: rng.dirichlet(np.full(len(vocab[c]), concentration)) for c in cols}
    counts = {c: np.zeros(len(vocab[c]), dtype=np.int64) for c in cols}
    val = {c: np.full(n, -1) for c in cols}

    def move():
        for c in cols:
            theta[c] = rng.dirichlet(concentration + counts[c])

    def draw(c, i):
        w = theta[c] * lik[c][code[c][i]]
        cdf = np.cumsum(w)
        return int(np.searchsorted(cdf, rng.random() * cdf[-1], side="right"))

    for sweep in range(n_iters + 1):
        for i in range(n):
            if sweep and i and i % rejuv == 0:
                move()
            if sweep == 0 or rng.random() >= 1.0 / P:
                for c in cols:
                    k = min(draw(c, i), len(vocab[c]) - 1)
                    if val[c][i] >= 0:
                        counts[c][val[c][i]] -= 1
                    val[c][i] = k
                    counts[c][k] += 1
            if sweep == 0 and (i + 1) % rejuv == 0:
                move()
    hit = sum(vocab[c][val[c][i]] == clean[c][i] for c in cols for i in range(n))
    return hit / float(n * len(cols))
