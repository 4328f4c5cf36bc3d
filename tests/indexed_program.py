"""A small provider program written with the indexed proportions and the number-code prior, and a pure-Python restatement
of its conditionals from the strings.

    Doc:  @learned theta :: Dict{String, ProportionsParameter{1.0}}
          npi   ~ NumberCodePrior()                      (number_code_prior.jl:10-14; Unmodeled() in the twin)
          state ~ Unmodeled()
          city  ~ ChooseProportionally(CITIES, theta[state])
    Obs:  d ~ Doc;   d.npi and d.state observed directly;   city_obs ~ AddTypos(d.city)

The frozen oracle layers do not know these priors, so the tests carry this restatement (as tests/tabulated_program.py does
for its terms): CRP masses, -log(code), log theta[state string][city] and the AddTypos density of oracle/literal.py on the
strings themselves — nothing of the lowering's option order, key columns or fixed-point arithmetic."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
import literal as lit  # noqa: E402

from pclean_amd.model import (AddTypos, ChooseProportionally, IndexedProportionsParameter, LoweredModel, Model,  # noqa: E402
                              NumberCodePrior, Query, Unmodeled)
from pclean_amd.trace import Trace  # noqa: E402

STATES = ["CA", "NY", "TX", "WA"]
CITIES = ["sacramento", "albany", "austin", "olympia", "fresno", "buffalo", "houston"]
CODES = ["1", "3", "7", "42", "1234567", "1234567893"]


def model(code_prior=True, concentration=1.0):
    m = Model()
    d = m.add_class("Doc")
    d.param("theta", IndexedProportionsParameter(concentration))
    with d.block():
        d.choice("npi", NumberCodePrior() if code_prior else Unmodeled())
        d.choice("state", Unmodeled())
        d.choice("city", ChooseProportionally(CITIES, "theta", index="state"))
    o = m.add_class("Obs")
    with o.block():
        o.fk("d", "Doc")
        o.choice("city_obs", AddTypos("d.city"))
    return m


def query(m):
    return Query(m, "Obs", {"NPI": "d.npi", "State": "d.state", "City": ("d.city", "city_obs")})


def _typo(rng, w):
    j = int(rng.integers(len(w)))
    return w[:j] + "q" + w[j + 1:]


def draw_program(seed=0, code_prior=True, n_ent=36, missing=False):
    """36 Doc rows with 1-4 references each and about 90 observed rows: the city observed exactly, with a typo, or not at
    all; npi and state always observed; with `missing` npi and the city are each missing on every seventh row, at
    different offsets, and both on row 0 (the state never: the keyed form needs every row's key).  Entities share codes and states, so that an observed (npi, state) fits
    several rows; codes span 1 .. 1234567893: below a small code a new row competes with the existing ones, below a large
    one it does not.  A few rows observe a city that none of the fitting entities holds."""
    rng = np.random.default_rng(seed)
    ents = [(CODES[k % len(CODES)], STATES[(k // 2) % len(STATES)], CITIES[(k * 5 + k // 7) % len(CITIES)]) for k in range(n_ent)]
    rows = []
    for e, (npi, st, city) in enumerate(ents):
        for j in range(1 + e % 4):
            u = (e + j) % 4
            rows.append((e, npi, st, city if u == 0 else (_typo(rng, city) if u == 1 else (None if u == 2 else CITIES[(e + 1) % len(CITIES)]))))
    n = len(rows)
    dirty = {"NPI": [r[1] for r in rows], "State": [r[2] for r in rows], "City": [r[3] for r in rows]}
    if missing:
        for c, col in enumerate(("NPI", "City")):
            for i in range(c, n, 7):
                dirty[col][i] = None
            dirty[col][0] = None
    m = model(code_prior)
    q = query(m)
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    tr = Trace(lw, n, seed)
    t = tr.tables["Doc"]
    ci = lw.colidx["Doc"]
    for e, (npi, st, city) in enumerate(ents):
        v = np.zeros(len(ci), np.int32)
        v[ci["npi"]] = lw.latent_dom[("Doc", "npi")].index_of(npi)
        v[ci["state"]] = lw.latent_dom[("Doc", "state")].index_of(st)
        v[ci["city"]] = lw.latent_dom[("Doc", "city")].index_of(city)
        assert tr.insert_row("Doc", v) == e
    for i, r in enumerate(rows):
        tr.cur[0, i] = r[0]
        t.counts[r[0]] += 1
    tr.resample_parameters()  # theta | counts: unequal vectors per state
    return dict(lw=lw, trace=tr, obs=obs, query=q, dirty=dirty, model=m, ents=ents, rows=rows, code_prior=code_prior)


# ---- the restatement --------------------------------------------------------------------------------------------------
def theta_by_string(S, shift=0):
    """{state string: {city string: probability}} of the trace's parameter; shift != 0: every state reads the vector of
    the state `shift` places further in the domain (the wrong-key twin of the power self-test)"""
    lw, tr = S["lw"], S["trace"]
    kdom = lw.latent_dom[("Doc", "state")]
    val = tr.params[("Doc", "theta")].value
    return {kdom.string(k): dict(zip(CITIES, val[(k + shift) % len(kdom)])) for k in range(len(kdom))}


def doc_rows(S):
    """{row id: (npi, state, city, count)} of the live Doc rows, as strings"""
    lw, tr = S["lw"], S["trace"]
    t, ci = tr.tables["Doc"], lw.colidx["Doc"]
    out = {}
    for r in np.flatnonzero(t.live[:t.n]):
        out[int(r)] = tuple(lw.latent_dom[("Doc", a)].string(int(t.cols[ci[a], r])) for a in ("npi", "state", "city")) + (int(t.counts[r]),)
    return out


def code_logp(S, s):
    return -math.log(int(s)) if S["code_prior"] else 0.0


def _eq(observed, value):
    return 0.0 if observed is None or observed == value else -math.inf


def _typos(observed, word):
    return 0.0 if observed is None else lit.add_typos_logpdf(observed, word, None, False)


def block_scores(S, i, theta=None):
    """{row id | ('NEW', city): log score} of observed row i (npi and state observed), its own reference removed first,
    and the block's log-marginal.  The new row's mass is split over its city: the nested conditional of the new-row branch."""
    theta = theta or theta_by_string(S)
    tr = S["trace"]
    npi, st, city = (S["dirty"][c][i] for c in ("NPI", "State", "City"))
    assert npi is not None and st is not None
    docs = doc_rows(S)
    cur = int(tr.cur[0, i])
    if cur >= 0:
        a, b, c, n = docs[cur]
        if n == 1:
            del docs[cur]
        else:
            docs[cur] = (a, b, c, n - 1)
    t = tr.tables["Doc"]
    s, d = t.strength, t.discount
    total = sum(v[3] for v in docs.values())
    sc = {}
    for r, (a, b, c, n) in docs.items():
        sc[r] = (math.log(n - d) - math.log(total + s)) + _eq(npi, a) + _eq(st, b) + _typos(city, c)
    new = math.log(s + d * len(docs)) - math.log(total + s) + code_logp(S, npi)
    for c in CITIES:
        sc[("NEW", c)] = new + math.log(theta[st][c]) + _typos(city, c)
    return sc


def latent_city_scores(S, ev_obs, theta=None):
    """{(state, city): log score} of a Doc row's city under the evidence rows' observations [(npi, state, city_obs)]:
    theta[state][city], the state every observing evidence row names, every AddTypos observation"""
    theta = theta or theta_by_string(S)
    sc = {}
    for st in theta:
        for c in CITIES:
            sc[(st, c)] = math.log(theta[st][c]) + sum(_eq(o[1], st) + _typos(o[2], c) for o in ev_obs)
    return sc


# ---- a larger synthetic program: strongly state-dependent cities ------------------------------------------------------
def synthetic(n_rows=300, seed=1, n_ent=60):
    """n_rows observed rows of n_ent providers; every state has one dominant city (90 %), the city is observed with a typo
    on every third row and missing on every eleventh"""
    rng = np.random.default_rng(seed)
    ents = []
    for e in range(n_ent):
        st = STATES[int(rng.integers(len(STATES)))]
        city = CITIES[STATES.index(st)] if rng.random() < 0.9 else CITIES[int(rng.integers(len(CITIES)))]
        ents.append((str(1000 + e), st, city))
    dirty = {"NPI": [], "State": [], "City": []}
    for i in range(n_rows):
        npi, st, city = ents[int(rng.integers(n_ent))]
        dirty["NPI"].append(npi)
        dirty["State"].append(st)
        dirty["City"].append(None if i % 11 == 5 else (_typo(rng, city) if i % 3 == 0 else city))
    m = model()
    q = query(m)
    lw = LoweredModel(m, q, dirty)
    return dict(lw=lw, obs=lw.encode_observations(dirty), dirty=dirty, model=m, query=q, ents=ents)


# ---- the sibling-choice index: a product leaf ---------------------------------------------------------------------------
DEGREES = ["medical", "osteopathy", "nursing"]
SPECS = ["cardiology", "dermatology", "pediatrics", "oncology"]


def product_model(uniform_index=False, degrees=None, specs=None):
    """Doc: degree ~ ChooseProportionally(DEGREES, deg_p) (or ChooseUniformly); spec ~ ChooseProportionally(SPECS,
    theta[degree]), one block.  Obs: d ~ Doc; deg_obs ~ AddTypos(d.degree); spec_obs ~ AddTypos(d.spec)"""
    from pclean_amd.model import ChooseUniformly, ProportionsParameter
    m = Model()
    d = m.add_class("Doc")
    d.py_strength = 20.0  # (a new row takes a share of every posterior that the draws can resolve)
    d.param("deg_p", ProportionsParameter(1.0))
    d.param("theta", IndexedProportionsParameter(1.0))
    with d.block():
        degrees, specs = degrees or DEGREES, specs or SPECS
        d.choice("degree", ChooseUniformly(degrees) if uniform_index else ChooseProportionally(degrees, "deg_p"))
        d.choice("spec", ChooseProportionally(specs, "theta", index="degree"))
    o = m.add_class("Obs")
    with o.block():
        o.fk("d", "Doc")
        o.choice("deg_obs", AddTypos("d.degree"))
        o.choice("spec_obs", AddTypos("d.spec"))
    return m


def product_query(m):
    return Query(m, "Obs", {"Degree": ("d.degree", "deg_obs"), "Spec": ("d.spec", "spec_obs")})


def product_program(seed=0, uniform_index=False, n_ent=24, free_every=0):
    """24 Doc rows with 1-4 references whose speciality goes with the degree (every sixth holds the fourth one), so that
    theta differs strongly between the degrees; deg_obs / spec_obs exact, with a typo or missing in every combination
    (both missing on some rows).  free_every: every k-th observed row has no current referent, and twelve more rows
    without a referent observe the degree alone or the speciality alone: the new row's share (Pitman-Yor strength 20: about
    a quarter) is split over the missing half by theta."""
    rng = np.random.default_rng(seed)
    ents = [(DEGREES[k % 3], SPECS[3] if k % 6 == 5 else SPECS[k % 3]) for k in range(n_ent)]
    rows = []
    for e, (dg, sp) in enumerate(ents):
        for j in range(1 + e % 4):
            u, w = (e + j) % 3, (e // 3 + j) % 3
            rows.append((e, dg if u == 0 else (_typo(rng, dg) if u == 1 else None), sp if w == 0 else (_typo(rng, sp) if w == 1 else None)))
    if free_every:
        rows += [(-1, DEGREES[k % 3] if k % 2 == 0 else None, SPECS[k % 4] if k % 2 else None) for k in range(12)]
    n = len(rows)
    dirty = {"Degree": [r[1] for r in rows], "Spec": [r[2] for r in rows]}
    m = product_model(uniform_index)
    q = product_query(m)
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    tr = Trace(lw, n, seed)
    t, ci = tr.tables["Doc"], lw.colidx["Doc"]
    for e, (dg, sp) in enumerate(ents):
        v = np.zeros(len(ci), np.int32)
        v[ci["degree"]] = lw.latent_dom[("Doc", "degree")].index_of(dg)
        v[ci["spec"]] = lw.latent_dom[("Doc", "spec")].index_of(sp)
        assert tr.insert_row("Doc", v) == e
    for i, r in enumerate(rows):
        if r[0] < 0 or (free_every and i % free_every == 1 and i > 0 and rows[i - 1][0] == r[0]):
            continue  # (never the entity's first row: the entity stays alive)
        tr.cur[0, i] = r[0]
        t.counts[r[0]] += 1
    tr.resample_parameters()
    return dict(lw=lw, trace=tr, obs=obs, query=q, dirty=dirty, model=m, ents=ents, rows=rows, uniform_index=uniform_index)


def product_priors(S, shift=0):
    """({degree: log p}, {degree: {spec: log theta}}) from the strings; shift: theta read `shift` degrees further"""
    tr = S["trace"]
    th = tr.params[("Doc", "theta")].value
    pa = np.full(len(DEGREES), 1.0 / len(DEGREES)) if S["uniform_index"] else tr.params[("Doc", "deg_p")].value
    return ({a: math.log(pa[k]) for k, a in enumerate(DEGREES)},
            {a: {b: math.log(th[(k + shift) % len(DEGREES)][j]) for j, b in enumerate(SPECS)} for k, a in enumerate(DEGREES)})


def product_block_scores(S, i, shift=0):
    """{row id | ('NEW', (degree, spec)): log score} of observed row i, its own reference removed first"""
    lw, tr = S["lw"], S["trace"]
    la, lt = product_priors(S, shift)
    dg_o, sp_o = S["dirty"]["Degree"][i], S["dirty"]["Spec"][i]
    t, ci = tr.tables["Doc"], lw.colidx["Doc"]
    docs = {}
    for r in np.flatnonzero(t.live[:t.n]):
        docs[int(r)] = [lw.latent_dom[("Doc", "degree")].string(int(t.cols[ci["degree"], r])),
                        lw.latent_dom[("Doc", "spec")].string(int(t.cols[ci["spec"], r])), int(t.counts[r])]
    cur = int(tr.cur[0, i])
    if cur >= 0:
        docs[cur][2] -= 1
        if docs[cur][2] == 0:
            del docs[cur]
    s, d = t.strength, t.discount
    total = sum(v[2] for v in docs.values())
    sc = {r: (math.log(n - d) - math.log(total + s)) + _typos(dg_o, a) + _typos(sp_o, b) for r, (a, b, n) in docs.items()}
    new = math.log(s + d * len(docs)) - math.log(total + s)
    for a in DEGREES:
        for b in SPECS:
            sc[("NEW", (a, b))] = new + la[a] + lt[a][b] + _typos(dg_o, a) + _typos(sp_o, b)
    return sc


def product_latent_scores(S, ev_obs, shift=0):
    """{(degree, spec): log score} of a Doc row's pair under its evidence rows' observations [(deg_obs, spec_obs)]"""
    la, lt = product_priors(S, shift)
    return {(a, b): la[a] + lt[a][b] + sum(_typos(o[0], a) + _typos(o[1], b) for o in ev_obs) for a in DEGREES for b in SPECS}


def product_synthetic(n_rows=300, seed=2, n_ent=50):
    """n_rows observed rows of n_ent providers whose speciality depends strongly on the degree (90 % one speciality per
    degree); typos on every third observation, each column missing on every ninth row"""
    rng = np.random.default_rng(seed)
    ents = []
    for e in range(n_ent):
        dg = DEGREES[int(rng.integers(3))]
        ents.append((dg, SPECS[DEGREES.index(dg)] if rng.random() < 0.9 else SPECS[int(rng.integers(4))]))
    dirty = {"Degree": [], "Spec": []}
    for i in range(n_rows):
        dg, sp = ents[int(rng.integers(n_ent))]
        dirty["Degree"].append(None if i % 9 == 2 else (_typo(rng, dg) if i % 3 == 0 else dg))
        dirty["Spec"].append(None if i % 9 == 5 else (_typo(rng, sp) if i % 3 == 1 else sp))
    m = product_model()
    q = product_query(m)
    lw = LoweredModel(m, q, dirty)
    return dict(lw=lw, obs=lw.encode_observations(dirty), dirty=dirty, model=m, query=q, ents=ents)


def product_shape_program(na, nb, n_rows=64, seed=0):
    """a product leaf of na x nb options over made-up words, n_rows observed rows that all start without a referent (an
    empty Doc table: every row takes the new-row branch); each observation exact, with a typo or missing"""
    rng = np.random.default_rng(seed)

    def words(n, taken):
        out = []
        while len(out) < n:
            w = "".join(rng.choice(list("abcdefghijklmnop"), size=int(rng.integers(6, 11))))
            if w not in taken:
                taken.add(w)
                out.append(w)
        return out
    taken = set()
    A, B = words(na, taken), words(nb, taken)
    dirty = {"Degree": [], "Spec": []}
    for i in range(n_rows):
        a, b = A[int(rng.integers(na))], B[int(rng.integers(nb))]
        dirty["Degree"].append(None if i % 4 == 1 or i % 8 == 3 else (_typo(rng, a) if i % 3 == 0 else a))
        dirty["Spec"].append(None if i % 4 == 2 or i % 8 == 3 else (_typo(rng, b) if i % 5 == 0 else b))
    m = product_model(degrees=A, specs=B)
    q = product_query(m)
    lw = LoweredModel(m, q, dirty)
    tr = Trace(lw, n_rows, seed)
    return dict(lw=lw, trace=tr, obs=lw.encode_observations(dirty), dirty=dirty, model=m, query=q, A=A, B=B)
