"""The rents County/Obs program (tests/addnoise_program.py) with a SECOND numeric observation in the same block: a deposit
the module synthesises itself, `deposit ~ AddNoise(deposit_base, 80.0)` on its own IndexedMeanParameter.  Both numbers
depend on the same referent and share the block's own choices (br, unit), which the proposal enumerates once
(proposal_compiler.jl:55-129 adds the logdensity of every observed choice of the block inside that enumeration).

The C++ oracle and oracle/literal.py know one Gaussian observation per block, so the tests of these programs carry their
own float64 restatement of the score (`gauss_part` below)."""
import numpy as np

import addnoise_program as ap
from pclean_amd import experiments as ex
from pclean_amd.model import (AddNoise, ChooseUniformly, IndexedLookup, IndexedMeanParameter, LoweredModel, Query,
                              Transformation, TransformedGaussian)
from pclean_amd.trace import Trace

DEPOSIT_STD = 80.0
RENT_STD = 150.0


def rents_units():
    """the two Transformations of experiments/rents/run.jl: dollars, and thousands of dollars"""
    return [Transformation(lambda x: x, lambda x: x, lambda x: 1.0),
            Transformation(lambda x: x / 1000.0, lambda x: x * 1000.0, lambda x: 1 / 1000.0)]


def _rent(o, index):
    o.julia("rent_base", IndexedLookup("avg_rent"), list(index))
    o.choice("rent", AddNoise("rent_base", RENT_STD))
    o.julia("corrected", lambda rent: round(rent), ["rent"])


def _deposit(o, index):
    o.param("avg_deposit", IndexedMeanParameter(2000, 1000))
    o.julia("deposit_base", IndexedLookup("avg_deposit"), list(index))
    o.choice("deposit", AddNoise("deposit_base", DEPOSIT_STD))
    o.julia("deposit_corrected", lambda deposit: round(deposit), ["deposit"])


FULL = ("county.state", "county.countykey", "br")
CAND = ("county.state", "county.countykey")


def two_model(dirty):
    """rent and deposit, both indexed by (county.state, county.countykey, br)"""
    m, o = ap._county_and_obs(dirty)
    _rent(o, FULL)
    _deposit(o, FULL)
    return m


def two_model_swapped(dirty):
    """the same two observations declared in the other order"""
    m, o = ap._county_and_obs(dirty)
    _deposit(o, FULL)
    _rent(o, FULL)
    return m


def two_candidate_model(dirty):
    """no br: candidate-side indices only, nothing own is enumerated"""
    m, o = ap._county_and_obs(dirty, with_br=False)
    _rent(o, CAND)
    _deposit(o, CAND)
    return m


def mixed_model(dirty):
    """rent as the rents program's TransformedGaussian (own choices br and unit), deposit as AddNoise (indexes br alone)"""
    m, o = ap._county_and_obs(dirty)
    o.choice("unit", ChooseUniformly(rents_units()))
    o.julia("rent_base", IndexedLookup("avg_rent"), list(FULL))
    o.choice("rent", TransformedGaussian("rent_base", RENT_STD, "unit"))
    o.julia("corrected", lambda unit, rent: round(unit.backward(rent)), ["unit", "rent"])
    _deposit(o, FULL)
    return m


def base_model(dirty):
    """no numeric observation at all: what the scores of the others hold besides their Gaussian part"""
    m, o = ap._county_and_obs(dirty)
    return m


def base_candidate_model(dirty):
    m, o = ap._county_and_obs(dirty, with_br=False)
    return m


def all_missing(model_fn):
    """model_fn with the Deposit column entirely missing (setup() reads the mark)"""
    def fn(dirty):
        return model_fn(dirty)
    fn.deposit_all_missing = True
    fn.__name__ = "all_missing_" + model_fn.__name__
    return fn


def query(m):
    attrs = {a.name for a in m.classes["Obs"].attrs}
    cols = {"CountyKey": "county.countykey", "County": ("county.name", "county_name"), "State": "county.state"}
    if "br" in attrs:
        cols["Room Type"] = "br"
    if "rent" in attrs:
        cols["Monthly Rent"] = ("corrected", "rent")
    if "deposit" in attrs:
        cols["Deposit"] = ("deposit_corrected", "deposit")
    return Query(m, "Obs", cols)


def with_deposit(dirty, clean, seed=11, all_missing_=False):
    """Deposit = d[state, countykey, br] + N(0, 80) from the CLEAN values (d drawn once per cell from N(2000, 600)),
    rounded to whole dollars; about 10 % of the dirty column is missing (None).  The rents data never misses a rent, so
    about 5 % of the dirty rents are blanked as well — except with all_missing_, whose rent column stays that of
    tests/addnoise_program.py."""
    rng = np.random.default_rng(seed)
    n = len(dirty["County"])
    cell = {}
    dep = []
    for i in range(n):
        key = tuple((clean[c][i] if clean[c][i] is not None else dirty[c][i]) for c in ("State", "County", "Room Type"))
        key = (key[0], dirty["CountyKey"][i], key[2])
        if key not in cell:
            cell[key] = rng.normal(2000.0, 600.0)
        dep.append(float(np.round(cell[key] + rng.normal(0.0, DEPOSIT_STD))))
    gone = rng.random(n) < 0.10
    dirty = dict(dirty)
    clean = dict(clean)
    clean["Deposit"] = list(dep)
    dirty["Deposit"] = [None if (gone[i] or all_missing_) else dep[i] for i in range(n)]
    no_rent = rng.random(n) < 0.05
    if not all_missing_:
        dirty["Monthly Rent"] = [None if no_rent[i] else v for i, v in enumerate(dirty["Monthly Rent"])]
    return dirty, clean


def setup(model_fn, n_rows=600, seed=3, data=None, query_fn=None):
    """model_fn(dirty) on the first n_rows rows of rents + Deposit, latent state from the clean values (the state of
    tests/addnoise_program.py: setup).  data: (dirty, clean) to use instead.  query_fn: the Query of a model with other
    columns than this module's (default: query)."""
    if data is None:
        dirty, clean = ex.rents_data()
        dirty = {c: v[:n_rows] for c, v in dirty.items()}
        clean = {c: v[:n_rows] for c, v in clean.items()}
        dirty, clean = with_deposit(dirty, clean, all_missing_=getattr(model_fn, "deposit_all_missing", False))
    else:
        dirty, clean = data
    m = model_fn(dirty)
    q = (query_fn or query)(m)
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    n = obs.shape[1]
    name_dom, state_dom = lw.latent_dom[("County", "name")], lw.latent_dom[("County", "state")]
    names = [c if (c is not None and name_dom.get(c) >= 0) else d for c, d in zip(clean["County"], dirty["County"])]
    states = []
    for i in range(n):
        v = clean["State"][i] if clean["State"][i] is not None and state_dom.get(clean["State"][i]) >= 0 else dirty["State"][i]
        states.append(v if v is not None else state_dom.string(0))
    tr = Trace.from_clean_values(lw, {0: {"countykey": list(dirty["CountyKey"]), "name": names, "state": states}}, n, seed)
    return dict(dirty=dirty, clean=clean, model=m, query=q, lw=lw, obs=obs, trace=tr)


def seed_means(S, seed=5):
    """both mean tables set to seeded arrays around the data (rent ~ 1500 +- 600, deposit ~ 2000 +- 600), by attribute"""
    centre = {"rent": (0, 1500.0), "deposit": (1, 2000.0)}
    for spec, mp in zip(S["lw"].gauss_specs, S["trace"].mean_params):
        stream, mean = centre[spec["gauss_attr"]]
        mp.value = np.random.default_rng([seed, stream]).normal(mean, 600.0, size=spec["n_mean"])


def normal_logpdf(x, mean, std):
    """logpdf(Normal(mean, std), x), written out (add_noise.jl:7, transformed_gaussian.jl:15)"""
    z = (x - mean) / std
    return -0.5 * z * z - np.log(std) - 0.5 * np.log(2 * np.pi)


def term_value(S, g, i, index_values, local_values):
    """N_g - lad_g of row i for term g, or None when the number is missing.  index_values: {candidate-side path: value id},
    local_values: the block's own choices by slot (lw.locals[0] order)."""
    lw = S["lw"]
    spec = lw.gauss_specs[g]
    x = lw.xnum[spec["x_col"], i]
    if x != x:
        return None
    idx = 0
    for d, st in zip(spec["dims"], spec["strides"]):
        idx += st * (index_values[d[1]] if d[0] == "cand" else local_values[d[1]])
    u = 0 if spec["t_local"] is None else local_values[spec["t_local"]]
    unit = spec["units"][u]
    bx = float(unit.backward(float(x)))
    lad = float(np.log(abs(float(unit.deriv(bx)))))
    return normal_logpdf(bx, S["trace"].mean_params[g].value[idx], spec["sigma"]) - lad


def gauss_part(S, i, index_values):
    """The Gaussian part of row i's score for a candidate with the given candidate-side index values, in float64:
    log-sum-exp over the unobserved own choices of  sum lp + sum_g (N_g - lad_g),  missing terms skipped, 0.0 when
    every term is missing.  Returns (value, number of combinations)."""
    lw = S["lw"]
    specs = lw.gauss_specs
    if all(lw.xnum[sp["x_col"], i] != lw.xnum[sp["x_col"], i] for sp in specs):
        return 0.0, 1
    spec = specs[0]
    ranges, lp = [], 0.0
    for l, (n, oc) in enumerate(zip(spec["local_n"], spec["local_obs"])):
        o = S["obs"][oc, i] if oc >= 0 else -1
        ranges.append([int(o)] if o >= 0 else list(range(n)))
        lp += -np.log(float(n))
    combos = [[]]
    for r in ranges:
        combos = [c + [v] for c in combos for v in r]
    vals = []
    for c in combos:
        s = lp
        for g in range(len(specs)):
            t = term_value(S, g, i, index_values, c)
            if t is not None:
                s += t
        vals.append(s)
    vals = np.array(vals)
    m = vals.max()
    return float(m + np.log(np.sum(np.exp(vals - m)))) if len(vals) > 1 else float(vals[0]), len(vals)
