"""The rents program (experiments/rents/run.jl) with its monthly rent observed through AddNoise (add_noise.jl:1-7) instead
of a TransformedGaussian: `rent ~ AddNoise(rent_base, 150.0)`, no unit choice.  Its twin, `identity_unit_model`, keeps the
TransformedGaussian but lets `unit` choose among ONE Transformation, the identity: ChooseUniformly over one option has
log-density -log(1) = -0.0, the identity's backward(x) is x * 1.0 and its log|deriv| 0.0, so every score of the twin is
the AddNoise program's score, operation for operation — the C++ oracle and the kernels must give both the same bits."""
import numpy as np

from pclean_amd import experiments as ex
from pclean_amd.model import (AddNoise, AddTypos, ChooseProportionally, ChooseUniformly, IndexedLookup, IndexedMeanParameter,
                              LoweredModel, Model, ProportionsParameter, Query, StringPrior, Transformation,
                              TransformedGaussian, Unmodeled)
from pclean_amd.trace import Trace

ROOM_TYPES = ["studio", "1br", "2br", "3br", "4br"]


def identity():
    return Transformation(lambda x: x, lambda x: x, lambda x: 1.0)


def _county_and_obs(dirty, with_br=True):
    poss = {}
    for k, c in zip(dirty["CountyKey"], dirty["County"]):
        poss.setdefault(k, [])
        if c not in poss[k]:
            poss[k].append(c)
    states = list(dict.fromkeys(v for v in dirty["State"] if v is not None))
    m = Model()
    c = m.add_class("County")
    c.param("state_pops", ProportionsParameter())
    c.choice("countykey", Unmodeled())
    c.choice("name", StringPrior(10, 35, poss, keyed_by="countykey"))
    c.choice("state", ChooseProportionally(states, "state_pops"))
    o = m.add_class("Obs")
    o.param("avg_rent", IndexedMeanParameter(1500, 1000))
    o.fk("county", "County")
    o.choice("county_name", AddTypos("county.name", 2))
    if with_br:
        o.choice("br", ChooseUniformly(ROOM_TYPES))
    return m, o


def addnoise_model(dirty, index=("county.state", "county.countykey", "br")):
    m, o = _county_and_obs(dirty)
    o.julia("rent_base", IndexedLookup("avg_rent"), list(index))
    o.choice("rent", AddNoise("rent_base", 150.0))
    o.julia("corrected", lambda rent: round(rent), ["rent"])
    return m


def candidate_mean_model(dirty):
    """AddNoise whose mean is indexed by the referent's values alone: nothing own is enumerated per candidate"""
    m, o = _county_and_obs(dirty, with_br=False)
    o.julia("rent_base", IndexedLookup("avg_rent"), ["county.state", "county.countykey"])
    o.choice("rent", AddNoise("rent_base", 150.0))
    o.julia("corrected", lambda rent: round(rent), ["rent"])
    return m


def identity_unit_model(dirty, with_br=True):
    m, o = _county_and_obs(dirty, with_br)
    o.choice("unit", ChooseUniformly([identity()]))
    o.julia("rent_base", IndexedLookup("avg_rent"), ["county.state", "county.countykey"] + (["br"] if with_br else []))
    o.choice("rent", TransformedGaussian("rent_base", 150.0, "unit"))
    o.julia("corrected", lambda unit, rent: round(unit.backward(rent)), ["unit", "rent"])
    return m


def identity_unit_candidate_model(dirty):
    """candidate_mean_model's twin: -log(1) + 0.0 for the one-option unit is the 0.0 of no own choice at all"""
    return identity_unit_model(dirty, with_br=False)


def query(m):
    cols = {"CountyKey": "county.countykey", "County": ("county.name", "county_name"), "State": "county.state",
            "Room Type": "br", "Monthly Rent": ("corrected", "rent")}
    if not any(a.name == "br" for a in m.classes["Obs"].attrs):
        del cols["Room Type"]
    return Query(m, "Obs", cols)


def setup(model_fn, n_rows=600, seed=3):
    """model_fn(dirty) on the first n_rows rows of rents, latent state from the clean values — the state
    tests/helpers.py: rents_setup builds for the rents program itself."""
    dirty, clean = ex.rents_data()
    dirty = {c: v[:n_rows] for c, v in dirty.items()}
    clean = {c: v[:n_rows] for c, v in clean.items()}
    m = model_fn(dirty)
    q = query(m)
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


def addnoise_logpdf(x, mean, std):
    """add_noise.jl:7, logpdf(Normal(mean, std), x), written out"""
    z = (x - mean) / std
    return -0.5 * z * z - np.log(std) - 0.5 * np.log(2 * np.pi)
