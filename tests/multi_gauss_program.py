"""Programs with THREE and FOUR numeric observations in one block (PCLEAN_MAX_GAUSS = 4), and programs whose own choices
fill the 16 combinations a candidate branch may enumerate (8 x 2, 4 x 4).  They extend tests/two_gauss_program.py: the
numbers besides the rent are synthesised here (with_numbers), every model has a `base` twin — the same program with every
numeric column missing — and the float64 restatement is two_gauss_program.term_value / gauss_part, which loop over
lw.gauss_specs and so restate any number of terms.

The C++ oracle, oracle/literal.py and the CPU oracle engine know ONE Gaussian observation per block.  What stands in for
them here: the restatement (checked against a long-double sum in tests/test_multi_gauss.py), the power preconditions
below (each way a kernel could misread a term moves the restatement by far more than the tests' tolerance), and the
chain `four terms with two missing == two terms == one term == oracle`, bit for bit (tests/test_gpu_multi_gauss.py)."""
import math
import types

import numpy as np

import addnoise_program as ap
import two_gauss_program as tg
from pclean_amd import experiments as ex
from pclean_amd.model import (AddNoise, ChooseUniformly, IndexedLookup, IndexedMeanParameter, Query, Transformation,
                              TransformedGaussian)

# attribute -> (observed column, sigma, prior mean of its IndexedMeanParameter, seed stream): four distinct sigmas
TERMS = {"rent": ("Monthly Rent", 150.0, 1500.0, 0), "deposit": ("Deposit", 80.0, 2000.0, 1),
         "fee": ("Fee", 25.0, 300.0, 2), "util": ("Util", 40.0, 400.0, 3)}
NUMERIC = ["Monthly Rent", "Deposit", "Fee", "Util"]  # the first k of them are a program's numeric columns
PRIOR_STD = 1000.0
# the synthetic numbers: (centre, spread) of the cell means, drawn once per cell, and whether the own choice names the cell too
SYNTH = {"Deposit": (2000.0, 600.0, True), "Fee": (300.0, 100.0, False), "Util": (400.0, 120.0, True)}
TIER = "Tier"


def tier_names(n):
    return [f"t{v}" for v in range(n)]


def four_units():
    """dollars, thousands of dollars and hundreds of dollars (linear: t_scale 1, 1000 and 100, so option 2 reads a scale
    and a log|deriv| that are neither option 0's nor option 1's), and one Transformation that is not linear —
    backward(x) = 1500 log(x) / log(1500): backward(x) and log|deriv| are derived columns, t_x_col / t_lad_col of option 3.
    It keeps a number near 1500 at its scale."""
    c = math.log(1500.0) / 1500.0
    return tg.rents_units() + [
        Transformation(lambda x: x / 100.0, lambda x: x * 100.0, lambda x: 1 / 100.0),
        Transformation(lambda v: math.exp(c * v), lambda x: math.log(max(x, 1.0)) / c, lambda v: c * math.exp(c * v))]


LINEAR_SCALES = [1.0, 1000.0, 100.0, 10.0]


def four_linear_units():
    """four linear Transformations with four distinct scales: every t_scale / t_logabsderiv slot is read, no derived column"""
    def unit(c):
        return Transformation(lambda x: x / c, lambda x: x * c, lambda x: 1 / c)
    return [unit(c) for c in LINEAR_SCALES]


# ---- data ----------------------------------------------------------------------------------------------------------------
def presence_patterns(n, k, seed):
    """pattern[i] in [0, 2^k): bit g set = numeric column g of row i is present.  Every run of 2^k consecutive rows holds
    every pattern once, in a seeded order — no coin flips, so no pattern can come out empty"""
    rng = np.random.default_rng([seed, 101])
    m = 1 << k
    return np.concatenate([rng.permutation(m) for _ in range((n + m - 1) // m)])[:n]


def with_numbers(dirty, clean, k, seed=11, tiers=0, units=None):
    """The first k of NUMERIC as dirty / clean columns.  Deposit, Fee and Util are synthesised the way
    two_gauss_program.with_deposit does: a mean per (state, countykey[, own choice]) cell drawn once, plus N(0, sigma),
    rounded; the cell is that of the CLEAN values.  Presence follows presence_patterns (the rent is blanked too).

    The own choice: Room Type — additionally blanked in every fourth run of 2^k rows, so every presence pattern occurs
    with the room type missing — or, with tiers > 0, a synthetic column Tier of that many values, observed in every
    other run of 2^k rows.

    units: Transformations; the dirty rent and deposit of row i are then written in unit i % len(units) (forward of the
    dollar value, not rounded), so that every option is the one that explains the numbers of a share of the rows."""
    n = len(dirty["County"])
    dirty, clean = dict(dirty), dict(clean)
    run = np.arange(n) >> k
    if tiers:
        t = np.random.default_rng(seed).integers(0, tiers, n)
        clean[TIER] = [tier_names(tiers)[v] for v in t]
        dirty[TIER] = [clean[TIER][i] if run[i] % 2 == 0 else None for i in range(n)]
        own = clean[TIER]
    else:
        dirty["Room Type"] = [None if run[i] % 4 == 3 else v for i, v in enumerate(dirty["Room Type"])]
        own = [c if c is not None else d for c, d in zip(clean["Room Type"], dirty["Room Type"])]
    state = [c if c is not None else d for c, d in zip(clean["State"], dirty["State"])]
    pat = presence_patterns(n, k, seed)
    for g, col in enumerate(NUMERIC[:k]):
        if g == 0:
            vals = list(dirty[col])
        else:
            centre, spread, by_own = SYNTH[col]
            crng, cell, vals = np.random.default_rng([seed, g]), {}, []
            for i in range(n):
                key = (state[i], dirty["CountyKey"][i]) + ((own[i],) if by_own else ())
                if key not in cell:
                    cell[key] = crng.normal(centre, spread)
                vals.append(float(np.round(cell[key] + crng.normal(0.0, TERMS[col.lower()][1]))))
            clean[col] = list(vals)
        if units is not None and g < 2:
            vals = [float(units[i % len(units)].forward(float(v))) for i, v in enumerate(vals)]
        dirty[col] = [vals[i] if (pat[i] >> g) & 1 else None for i in range(n)]
    return dirty, clean


# ---- models --------------------------------------------------------------------------------------------------------------
def _term(o, name, index, unit=None):
    col, sigma, prior_mean, _ = TERMS[name]
    if name != "rent":  # (avg_rent is declared by addnoise_program._county_and_obs)
        o.param(f"avg_{name}", IndexedMeanParameter(prior_mean, PRIOR_STD))
    o.julia(f"{name}_base", IndexedLookup(f"avg_{name}"), list(index))
    if unit is None:
        o.choice(name, AddNoise(f"{name}_base", sigma))
        o.julia(f"{name}_corrected", lambda x: round(x), [name])
    else:
        o.choice(name, TransformedGaussian(f"{name}_base", sigma, unit))
        o.julia(f"{name}_corrected", lambda u, x: round(u.backward(x)), [unit, name])


def _model(k, tiers=0, units=None):
    """marks a model function with the data it is written for: its first k numeric columns, its Tier column, the units its
    rent and deposit are written in"""
    def mark(fn):
        fn.k, fn.tiers, fn.units = k, tiers, units
        return fn
    return mark


@_model(3)
def three_model(dirty):
    """three AddNoise terms, all indexed by (county.state, county.countykey, br)"""
    m, o = ap._county_and_obs(dirty)
    for name in ("rent", "deposit", "fee"):
        _term(o, name, tg.FULL)
    return m


@_model(4)
def four_model(dirty):
    """four AddNoise terms of the same shape, four distinct sigmas"""
    m, o = ap._county_and_obs(dirty)
    for name in ("rent", "deposit", "fee", "util"):
        _term(o, name, tg.FULL)
    return m


@_model(4)
def four_model_permuted(dirty):
    """four_model declared in another order"""
    m, o = ap._county_and_obs(dirty)
    for name in ("util", "rent", "fee", "deposit"):
        _term(o, name, tg.FULL)
    return m


@_model(4)
def four_mixed_model(dirty):
    """rent as the rents program's TransformedGaussian (own choices br and unit), deposit and util as AddNoise on
    (state, countykey, br), fee as AddNoise on the candidate-side values alone: strides [850, 5, 1] and [170, 1]"""
    m, o = ap._county_and_obs(dirty)
    o.choice("unit", ChooseUniformly(tg.rents_units()))
    _term(o, "rent", tg.FULL, unit="unit")
    _term(o, "deposit", tg.FULL)
    _term(o, "fee", tg.CAND)
    _term(o, "util", tg.FULL)
    return m


TIERED = ("county.state", "county.countykey", "tier")


@_model(3, tiers=8)
def sixteen_8x2(dirty):
    """8 tiers x 2 units = 16 combinations; three terms"""
    m, o = ap._county_and_obs(dirty, with_br=False)
    o.choice("tier", ChooseUniformly(tier_names(8)))
    o.choice("unit", ChooseUniformly(tg.rents_units()))
    _term(o, "rent", TIERED, unit="unit")
    _term(o, "deposit", TIERED)
    _term(o, "fee", tg.CAND)
    return m


def _four_by_four(dirty, units):
    m, o = ap._county_and_obs(dirty, with_br=False)
    o.choice("tier", ChooseUniformly(tier_names(4)))
    o.choice("unit", ChooseUniformly(units))
    _term(o, "rent", TIERED, unit="unit")
    _term(o, "deposit", TIERED, unit="unit")
    _term(o, "fee", tg.CAND)
    return m


@_model(3, tiers=4, units=four_units)
def sixteen_4x4(dirty):
    """4 tiers x 4 Transformations = 16 combinations: rent and deposit both choose among four_units() (three linear
    scales, the derived columns of option 3 per term), fee is an AddNoise on the candidate-side values"""
    return _four_by_four(dirty, four_units())


@_model(3, tiers=4, units=four_linear_units)
def sixteen_4x4_linear(dirty):
    """sixteen_4x4 with four_linear_units(): all four t_scale and t_logabsderiv slots hold distinct values"""
    return _four_by_four(dirty, four_linear_units())


def query(m):
    attrs = {a.name for a in m.classes["Obs"].attrs}
    cols = {"CountyKey": "county.countykey", "County": ("county.name", "county_name"), "State": "county.state"}
    if "br" in attrs:
        cols["Room Type"] = "br"
    if "tier" in attrs:
        cols[TIER] = "tier"
    for name, (col, _, _, _) in TERMS.items():
        if name in attrs:
            cols[col] = (f"{name}_corrected", name)
    return Query(m, "Obs", cols)


def data(model_fn, n_rows=600, missing=()):
    """(dirty, clean) of the first n_rows rents rows for model_fn; the columns named in `missing` entirely None"""
    dirty, clean = ex.rents_data()
    dirty = {c: v[:n_rows] for c, v in dirty.items()}
    clean = {c: v[:n_rows] for c, v in clean.items()}
    dirty, clean = with_numbers(dirty, clean, model_fn.k, tiers=model_fn.tiers,
                                units=model_fn.units() if model_fn.units else None)
    for col in missing:
        dirty[col] = [None] * n_rows
    return dirty, clean


def setup(model_fn, n_rows=600, seed=3, missing=(), base=False, given=None):
    """two_gauss_program.setup on this module's data and query.  base: the model's twin — the same program with every
    numeric column missing (the lowering accepts it: each term is lowered, no row ever scores one).  given: (dirty, clean)
    to use instead of data(model_fn, ...)."""
    if base:
        missing = NUMERIC[:model_fn.k]
    return tg.setup(model_fn, seed=seed, data=data(model_fn, n_rows, missing) if given is None else given, query_fn=query)


def seed_means(S, spread_sigmas, seed=5):
    """every term's mean table from its own stream (named by the attribute, so a permuted declaration order keeps the
    tables): centred at the attribute's data scale, spread spread_sigmas times that term's sigma"""
    for spec, mp in zip(S["lw"].gauss_specs, S["trace"].mean_params):
        _, sigma, centre, stream = TERMS[spec["gauss_attr"]]
        mp.value = np.random.default_rng([seed, stream]).normal(centre, spread_sigmas * sigma, size=spec["n_mean"])


def fix_locals(S):
    """own choices of every row: the observed first one where there is one, a fixed pattern elsewhere; the second one
    cycling through its options"""
    lw, tr = S["lw"], S["trace"]
    spec = lw.gauss_specs[0]
    n = tr.cur.shape[1]
    for l, (nl, oc) in enumerate(zip(spec["local_n"], spec["local_obs"])):
        o = S["obs"][oc] if oc >= 0 else np.full(n, -1)
        tr.locals[0][:, l] = np.where(o >= 0, o, (np.arange(n) + l) % nl)


# ---- the restatement's parts ---------------------------------------------------------------------------------------------
def presence(S):
    """[k][n_rows] bool: term g's number is present"""
    lw = S["lw"]
    return np.stack([~np.isnan(lw.xnum[sp["x_col"]]) for sp in lw.gauss_specs])


def own_observed(S):
    """[n_rows] bool: the first own choice is observed"""
    oc = S["lw"].gauss_specs[0]["local_obs"][0]
    return S["obs"][oc] >= 0


def referent_values(S, k):
    """candidate-side index values of County row k"""
    lw, t = S["lw"], S["trace"].tables["County"]
    return {"state": int(t.cols[lw.colidx["County"]["state"], k]), "countykey": int(t.cols[lw.colidx["County"]["countykey"], k])}


def combo_scores(S, i, index_values):
    """([(l0, l1) or (l0,)], scores): the score of every combination of the unobserved own choices of row i that
    two_gauss_program.gauss_part marginalises, in the enumeration's order.  Every number missing: the combinations the
    observed own choices allow, all 0.0 (they follow their uniform priors)."""
    lw = S["lw"]
    spec = lw.gauss_specs[0]
    ranges, lp = [], 0.0
    for n, oc in zip(spec["local_n"], spec["local_obs"]):
        o = S["obs"][oc, i] if oc >= 0 else -1
        ranges.append([int(o)] if o >= 0 else list(range(n)))
        lp += -np.log(float(n))
    combos = [[]]
    for r in ranges:
        combos = [c + [v] for c in combos for v in r]
    any_present = presence(S)[:, i].any()
    vals = []
    for c in combos:
        s = lp if any_present else 0.0
        for g in range(len(lw.gauss_specs)):
            t = tg.term_value(S, g, i, index_values, c)
            if t is not None:
                s += t
        vals.append(s)
    return [tuple(c) for c in combos], np.array(vals)


def rows_visited(S, per_kind=2):
    """the rows the score tests visit: of every presence pattern x (first own choice observed, missing), the first few"""
    pres, own = presence(S), own_observed(S)
    pat = (pres * (1 << np.arange(len(pres)))[:, None]).sum(axis=0)
    rows = []
    for p in range(1 << len(pres)):
        for o in (True, False):
            sel = np.flatnonzero((pat == p) & (own == o))
            assert len(sel) >= per_kind, (p, o)
            rows.extend(sel[:per_kind])
    return np.array(sorted(int(r) for r in rows), dtype=np.int32), pat


def perturbed(S, drop=None, swap_sigma=None, table_from=None, swap_strides=None, option_alias=False):
    """S as a kernel that misreads one thing would see it (for the power preconditions; lw and trace are views that hold
    what term_value / gauss_part read):
      drop = g                 term g is never added
      swap_sigma = (g, h)      the two terms' sigmas exchanged
      table_from = (g, h)      term g reads its mean from term h's table
      swap_strides = (g, a, b) the strides of term g's index dimensions a and b exchanged
      option_alias             Transformation option u read as option u & 1 (only two slots filled, or copied)
    An index that leaves the table it is read from wraps around (a device would read whatever lies there)."""
    lw, tr = S["lw"], S["trace"]
    specs = [dict(sp) for sp in lw.gauss_specs]
    tables = [mp.value for mp in tr.mean_params]
    if swap_sigma is not None:
        g, h = swap_sigma
        specs[g]["sigma"], specs[h]["sigma"] = specs[h]["sigma"], specs[g]["sigma"]
    if table_from is not None:
        g, h = table_from
        tables[g] = tables[h]
    if swap_strides is not None:
        g, a, b = swap_strides
        st = list(specs[g]["strides"])
        st[a], st[b] = st[b], st[a]
        specs[g]["strides"] = st
    if option_alias:
        for sp in specs:
            sp["units"] = [sp["units"][u & 1] for u in range(len(sp["units"]))]
    if drop is not None:
        del specs[drop], tables[drop]

    class Wrapped:
        def __init__(self, v):
            self.value = v

        def __getitem__(self, idx):
            return self.value[idx % len(self.value)]
    mean_params = [types.SimpleNamespace(value=Wrapped(v)) for v in tables]
    return dict(S, lw=types.SimpleNamespace(gauss_specs=specs, xnum=lw.xnum),
                trace=types.SimpleNamespace(mean_params=mean_params))


def perturbations(S):
    """{name: keyword arguments of perturbed()}: every single term dropped, every pair of sigmas exchanged, every term
    reading every other table, every pair of index strides of every term exchanged"""
    k = len(S["lw"].gauss_specs)
    out = {}
    for g in range(k):
        out[f"drop term {g}"] = dict(drop=g)
        for h in range(k):
            if h > g:
                out[f"sigmas of {g} and {h} exchanged"] = dict(swap_sigma=(g, h))
            if h != g:
                out[f"term {g} reads table {h}"] = dict(table_from=(g, h))
        nd = len(S["lw"].gauss_specs[g]["dims"])
        for a in range(nd):
            for b in range(a + 1, nd):
                out[f"strides {a} and {b} of term {g} exchanged"] = dict(swap_strides=(g, a, b))
    if any(len(sp["units"]) > 2 for sp in S["lw"].gauss_specs):
        out["Transformation option u read as u & 1"] = dict(option_alias=True)
    return out


# what a score holds besides its Gaussian part: the one AddTypos observation, at worst -1e5 for a name beyond max_typos
# (add_typos.jl:34), and the name's prior, the state's and the referent's count, a few hundred at the very most
SCORE_REST = 1.0e5 + 1000.0


def score_tolerance(n_comb, want, score=None):
    """the tolerance of the candidate and new-row score tests: the fixed-point log-sum-exp bound plus 1e-12 relative to the
    score.  Without a score (CPU: the preconditions) the score's size is bounded by |want| + SCORE_REST."""
    import posterior_exact
    mag = abs(score) if score is not None else abs(want) + SCORE_REST
    return posterior_exact.logml_bound(n_comb, want) + 1e-12 * max(1.0, mag)


# ---- the chosen particle's own choices -----------------------------------------------------------------------------------
FIX_CUTOFF = 28.5  # pclean_fixw(d) == 0 for d < -28.5 (include/pclean_detmath.h): such a combination is never drawn
SCORE_SPREAD = 6.0     # mean spread (in sigmas) of the score tests
DECIDED_SPREAD = 40.0  # ... of the own-choice test: wide enough that one combination usually outweighs all others


def decided(S, i, index_values):
    """(combinations, scores, index of the best, decided): decided when the runner-up lies more than FIX_CUTOFF below the
    best, so that every other combination's fixed-point weight is exactly 0 and the draw must be the best one"""
    combos, sc = combo_scores(S, i, index_values)
    best = int(np.argmax(sc))
    rest = np.delete(sc, best)
    return combos, sc, best, bool(len(rest) == 0 or rest.max() < sc[best] - FIX_CUTOFF)
