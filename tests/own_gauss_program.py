"""Flat programs with Gaussian observations in an own block, and their exact conditionals (TEST INFRASTRUCTURE).

    room ~ ChooseProportionally(rooms, p)            (na rooms; na = 0: no string factor)
    room_obs ~ AddTypos(room)                        (typos=True)        or `room` in the query (direct=True), or both
    unit ~ ChooseUniformly(units)                    (nb units; nb = 0: AddNoise, no unit)
    rent ~ TransformedGaussian(avg[room], SIGMA, unit)   /   AddNoise(avg[room], SIGMA)
    fee  ~ AddNoise(avg2[room], SIGMA2)              (second="room"),  AddNoise(avg2[], SIGMA2)  (second="const")

The leaf's options are the grid k = a * nb + b.  exact_scores() restates the conditional of a row in float64 from
oracle/literal.py's densities (add_typos_logpdf on the strings, normal_logpdf on the numbers) in the order the contract
names: log p(a) + log p(b); the string terms in declaration order, the equality of a direct observation last; then per
present number  += logpdf, -= log|deriv|.  Nothing of the product's lowering is used."""
import math

import numpy as np

import posterior_exact as pe
from posterior_exact import lit
from pclean_amd.model import (AddNoise, AddTypos, ChooseProportionally, ChooseUniformly, IndexedLookup, IndexedMeanParameter,
                              LoweredModel, Model, ProportionsParameter, Query, Transformation, TransformedGaussian)

SIGMA, SIGMA2 = 150.0, 4.0


def make_units(nb, nonlinear=False):
    """nb Transformations: the identity, x / 1000 (thousands), x / 12 (per year -> per month) — linear — and, last when
    nonlinear, forward(b) = b^2 / 1000 (backward and log|deriv| then differ from row to row: derived columns)"""
    lin = [Transformation(lambda x: x, lambda x: x, lambda x: 1.0),
           Transformation(lambda x: x / 1000.0, lambda x: x * 1000.0, lambda x: 1.0 / 1000.0),
           Transformation(lambda x: x * 12.0, lambda x: x / 12.0, lambda x: 12.0),
           Transformation(lambda x: x / 7.0, lambda x: x * 7.0, lambda x: 1.0 / 7.0)]
    sq = Transformation(lambda b: b * b / 1000.0, lambda x: math.sqrt(1000.0 * x), lambda b: 2.0 * b / 1000.0)
    us = lin[:nb]
    if nonlinear and nb:
        us[-1] = sq
    return us


def gauss_case(na, nb, n_rows=320, seed=0, typos=True, direct=False, second=None, nonlinear=False, long_run=0, pool=None,
               wl=(4, 7), spread=None, wrong_unit=None, room_missing=0.0):
    """A program, its rows and what generated them.  A fifth of the rows lack the number, a tenth the string observation,
    some both (and the second number); long_run: that many rows share one string observation.  pool: the string
    observations are drawn from that many distinct strings (keeps the restatement of a large grid cheap).  spread: the means
    of the rooms lie that many SIGMA apart (default: close, so that the conditionals are not point masses); wrong_unit: the
    share of rows stated in a unit other than the first (default: uniform over the units) — such a case has no missing cells
    but a share room_missing of the directly observed rooms."""
    rng = np.random.default_rng(seed)
    rooms = pe._words(rng, na, *wl) if na else []
    units = make_units(nb, nonlinear)
    step = SIGMA * (spread if spread is not None else 0.7)
    mu = 1500.0 + step * np.arange(max(na, 1))
    mu2 = 40.0 + 3.0 * np.arange(max(na, 1)) if second == "room" else np.array([40.0])
    p = rng.dirichlet(np.ones(na) * 2.0) if na else np.zeros(0)
    obs_pool = None
    if pool and na:
        obs_pool = [pe._typo(rng, rooms[int(rng.integers(na))]) for _ in range(pool)]
    cols = {"Room": [], "RoomObs": [], "Rent": [], "Fee": []}
    truth = []
    shared = None
    for i in range(n_rows):
        a = int(rng.choice(na, p=p)) if na else 0
        if nb and wrong_unit is not None:
            b = 0 if rng.random() >= wrong_unit else int(rng.integers(1, nb)) if nb > 1 else 0
        else:
            b = int(rng.integers(nb)) if nb else 0
        base = float(rng.normal(mu[a], SIGMA))
        x = float(units[b].forward(base)) if nb else base
        fee = float(rng.normal(mu2[a if second == "room" else 0], SIGMA2))
        ro = None
        if na:
            if obs_pool is not None:
                ro = obs_pool[int(rng.integers(len(obs_pool)))]
            else:
                ro = rooms[a] if rng.random() < 0.6 else pe._typo(rng, rooms[a])
        kind = i % 10 if wrong_unit is None else -1
        if kind == 3 or kind == 7:
            x = None
        if kind == 5:
            ro = None
        if kind == 7 and i % 20 == 7:
            ro, fee = None, None  # (a row with nothing observed)
        if kind == 4:
            fee = None
        if na and i < long_run:  # (one string observation for all of them: one tuple run)
            shared = shared or ro or rooms[a]
            ro = shared
        seen = na and direct and kind not in (5, 6) and not (wrong_unit is not None and rng.random() < room_missing)
        cols["Room"].append(rooms[a] if seen else None)
        cols["RoomObs"].append(ro)
        cols["Rent"].append(x)
        cols["Fee"].append(fee)
        truth.append((a, b))
    m = Model()
    o = m.add_class("Obs")
    o.param("p", ProportionsParameter(1.0))
    o.param("avg", IndexedMeanParameter(1500.0, 1000.0))
    o.param("avg2", IndexedMeanParameter(40.0, 30.0))
    bind = {}
    with o.block():
        if na:
            o.choice("room", ChooseProportionally(rooms, "p"))
            if typos:
                o.choice("room_obs", AddTypos("room"))
        if nb:
            o.choice("unit", ChooseUniformly(units))
        o.julia("base", IndexedLookup("avg"), ["room"] if na else [])
        if nb:
            o.choice("rent", TransformedGaussian("base", SIGMA, "unit"))
            o.julia("corrected", lambda unit, rent: round(unit.backward(rent)), ["unit", "rent"])
        else:
            o.choice("rent", AddNoise("base", SIGMA))
            o.julia("corrected", lambda rent: round(rent), ["rent"])
        if second:
            o.julia("base2", IndexedLookup("avg2"), ["room"] if second == "room" else [])
            o.choice("fee", AddNoise("base2", SIGMA2))
            o.julia("fee_clean", lambda fee: round(fee), ["fee"])
    if na and typos:
        bind["RoomObs"] = ("room", "room_obs")
    if na and direct:
        bind["Room"] = "room"
    bind["Rent"] = ("corrected", "rent")
    if second:
        bind["Fee"] = ("fee_clean", "fee")
    dirty = {c: cols[c] for c in bind}
    return dict(model=m, query=Query(m, "Obs", bind), dirty=dirty, n_rows=n_rows, rooms=rooms, units=units, na=na, nb=nb,
                typos=typos, direct=direct, second=second, mu=mu, mu2=mu2, p=p, truth=truth, K=max(na, 1) * max(nb, 1))


def lower(S):
    lw = LoweredModel(S["model"], S["query"], S["dirty"])
    return lw, lw.encode_observations(S["dirty"])


def set_params(S, tr):
    """the generating parameters into a Trace"""
    if S["na"]:
        tr.params[("Obs", "p")].value = np.asarray(S["p"], dtype=np.float64)
    tr.mean_params[0].value = np.asarray(S["mu"], dtype=np.float64).copy()
    if S["second"]:
        tr.mean_params[1].value = np.asarray(S["mu2"], dtype=np.float64).copy()


def exact_scores(S, i, p=None, mu=None, mu2=None):
    """(scores float64 [K], sum of the absolute terms [K]) of row i over the grid k = a * nb + b"""
    na, nb = max(S["na"], 1), max(S["nb"], 1)
    p = S["p"] if p is None else p
    mu = S["mu"] if mu is None else mu
    mu2 = S["mu2"] if mu2 is None else mu2
    d = S["dirty"]
    with np.errstate(divide="ignore"):
        lpa = np.log(np.asarray(p, dtype=np.float64)) if S["na"] else np.zeros(1)
    lpb = np.full(nb, -math.log(nb)) if S["nb"] else np.zeros(1)
    if S["na"] and S["nb"]:
        s = (lpa[:, None] + lpb[None, :]).reshape(-1)
    else:
        s = (lpa if S["na"] else lpb).copy()
    mag = np.abs(s)
    a_of = np.repeat(np.arange(na), nb)
    b_of = np.tile(np.arange(nb), na)
    if S["na"] and S["typos"]:
        t = np.array([lit.add_typos_logpdf(d["RoomObs"][i], w) for w in S["rooms"]])
        s = s + t[a_of]
        mag = mag + np.abs(t)[a_of]
    if S["na"] and S["direct"] and d["Room"][i] is not None:
        s = np.where(np.array(S["rooms"], dtype=object)[a_of] == d["Room"][i], s, -math.inf)
    x = d["Rent"][i]
    if x is not None:
        if S["nb"]:
            bx = np.array([float(u.backward(x)) for u in S["units"]])
            lad = np.array([math.log(abs(float(u.deriv(float(u.backward(x)))))) for u in S["units"]])
        else:
            bx, lad = np.array([x * 1.0]), np.array([0.0])
        lp = lit.normal_logpdf(bx[b_of], np.asarray(mu, dtype=np.float64)[a_of if S["na"] else np.zeros_like(a_of)], SIGMA)
        s = s + lp
        s = s - lad[b_of]
        mag = mag + np.abs(lp) + np.abs(lad[b_of])
    if S["second"] and d["Fee"][i] is not None:
        m2 = np.asarray(mu2, dtype=np.float64)[a_of if S["second"] == "room" else np.zeros_like(a_of)]
        lp = lit.normal_logpdf(d["Fee"][i] * 1.0, m2, SIGMA2)
        s = s + lp
        s = s - 0.0
        mag = mag + np.abs(lp)
    return s, mag


def exact_pi(S, i, **kw):
    """{k: probability} of row i's exact joint conditional"""
    s, _ = exact_scores(S, i, **kw)
    return pe.normalise({k: float(v) for k, v in enumerate(s)})


def numpy_stats(S, lw, vals, g, e):
    """count / qsum of Gaussian term g over the joint values vals, the NumPy restatement: rint(bx * 2^e) in int64"""
    spec = lw.gauss_specs[g]
    nb = max(S["nb"], 1)
    x = lw.xnum[spec["x_col"]]
    rows = np.flatnonzero((vals >= 0) & ~np.isnan(x))
    a, b = vals[rows] // nb, vals[rows] % nb
    idx = (a if spec["dims"] else np.zeros_like(a)).astype(np.int64)
    unit = b if spec["t_local"] is not None else np.zeros_like(b)
    bx = lw.gauss_backward(rows, unit, g)
    ok = np.isfinite(bx)
    q = np.rint(bx[ok] * 2.0 ** e).astype(np.int64)
    count = np.bincount(idx[ok], minlength=spec["n_mean"]).astype(np.int64)
    qsum = np.zeros(spec["n_mean"], dtype=np.int64)
    np.add.at(qsum, idx[ok], q)
    return count, qsum


# ---- the exact-distribution case (device test) and the draws its power is checked with on the CPU ------------------------
DIST = dict(na=3, nb=2, n_rows=60, seed=8, spread=0.5)
S_DRAWS, DIST_SEED = pe.S_GPU, 4100


def dist_case():
    """close means (the conditionals spread over several options), and the exact joint conditional of every row"""
    S = gauss_case(**DIST)
    return S, [exact_pi(S, i) for i in range(S["n_rows"])]
