"""Latent sweeps that weigh chosen ProposalDummyValues of KEYED choices (TimePrior under MaybeSwap, keyed StringPrior under
AddTypos): the float64 restatement and the closed forms of tests/latent_time_program.py have to earn their place before the
device is compared with them (tests/test_gpu_latent_time.py), and the host side is checked where no GPU is needed.

  * the oracle's sampler returns the 1440 times the closed forms enumerate, uniformly;
  * the restatement: c(placeholder) is the dummy mass alone, and the three cases of a drawn time move it by what
    maybe_swap.jl:13-28 says;
  * the weights program holds every case in at least W_MIN_CASE slots, and every misreading a kernel could commit — another
    key's dummy mass, another key's number of options, another evidence row's error probability, membership by id instead
    of by string, a missing observation skipped — moves at least a dozen slots by 1000 tolerances or more;
  * the closed forms are distributions, the MECHANISM follows them, and at the device test's draw count the uncorrected
    kernel (every weight equal) is rejected with p < 1e-6;
  * host logic: which choices are served, the `excl` convention per key, the per-row dummy options, and the recorded
    origin -> resample_dummies gives the row the time its weight was computed with."""
import math
import types

import numpy as np
import pytest

import latent_time_program as lt
import posterior_exact as pe

N_DRAWS = lt.DIST_ROWS * lt.DIST_SWEEPS


@pytest.fixture(scope="module")
def wprog(oracle):
    return lt.weights_program(oracle)


def test_sampler_returns_the_enumerated_times(oracle):
    from pclean_amd import sampling
    keys = [sampling.dummy_seed(5, 3, p, 0) for p in range(1, 41)]
    got = [lt.time_at(oracle, k, e) for k in keys for e in range(50)]
    assert len(lt.ALL_TIMES) == 1440 == len(set(lt.ALL_TIMES))
    assert all(s in set(lt.ALL_TIMES) for s in got)
    # element `elem` of the stream of `key` is one draw, whatever the length of the call that made it
    ro = oracle.RandomOracle()
    whole = ro.random_time_prior(50, int(keys[0]), 0)
    assert [lt.render(int(h), int(m), int(a)) for h, m, a in whole] == got[:50]
    hours = {}
    for s in got:
        hours[s.split(":")[0]] = hours.get(s.split(":")[0], 0) + 1
    assert pe.gof([(0, {str(h): 1.0 / 12 for h in range(1, 13)}, hours)])["p"] > pe.ALPHA
    # minutes are not padded: the pattern of time_prior.jl:10 rejects a sixth of what the sampler returns
    assert sum(1 for s in lt.ALL_TIMES if not lt.lit._TIME_RE.match(s)) == 12 * 9 * 2


def test_the_restatement_on_hand_made_rows():
    atoms = {"ka": ["1:5 a.m."], "kb": ["10:10 a.m.", "3:30 p.m."], "kc": []}
    trips = [{"key": "kb", "dep": "**:** p.m."}, {"key": "ka", "dep": "**:** p.m."}]
    rows = [dict(trip=0, src="s0", dep="7:15 a.m."), dict(trip=0, src="s0", dep="7:15 a.m."), dict(trip=0, src="s1", dep="8:8 p.m."),
            dict(trip=1, src="s2"), dict(trip=1, src="s2"), dict(trip=1, src="s3", dep="6:6 a.m.")]
    S = lt.trip_program(trips, rows, atoms)
    ph = lt.dist_of(S, "dep").dummy_value()
    prob = {s: float(S["trace"].prob_table()[S["trace"].prob_index()[i]]) for i, s in ((0, "s0"), (2, "s1"), (3, "s2"), (5, "s3"))}
    assert len(set(prob.values())) == 4
    md_kb = math.log1p(-2.0 / 1440.0)
    assert abs(lt.dummy_mass_log(S, "dep", "kb") - md_kb) <= 1e-15 and lt.dummy_mass_log(S, "dep", "ka") == 0.0
    assert lt.dummy_mass_log(S, "dep", "kc") == 0.0
    # the placeholder and (i): the likelihood terms cancel exactly
    for v in (ph, "2:2 a.m."):
        c, tol = lt.slot_correction(S, "dep", 0, v)
        assert abs(c + md_kb) <= tol and lt.slot_case(S, "dep", 0, v) == {"i"}
    assert lt.evidence_of(S, "dep", 0) == [("7:15 a.m.", prob["s0"], 2), ("8:8 p.m.", prob["s1"], 1)]
    # (ii): the two entries that repeat v move by log1p(-p) - log p + log n each
    c, _ = lt.slot_correction(S, "dep", 0, "7:15 a.m.")
    want = -md_kb + 2 * (math.log1p(-prob["s0"]) - math.log(prob["s0"]) + math.log(2))
    assert abs(c - want) <= 1e-12 and lt.slot_case(S, "dep", 0, "7:15 a.m.") == {"ii"}
    # (iii) with missing observations: v is the option, the two missing entries score 0 where the placeholder scores -1000
    c, _ = lt.slot_correction(S, "dep", 1, "1:5 a.m.")
    assert c == 2000.0 and lt.slot_case(S, "dep", 1, "1:5 a.m.") == {"iii-missing"}
    # ... an atom of ANOTHER key is no option of this row's key
    c, _ = lt.slot_correction(S, "dep", 1, "10:10 a.m.")
    assert c == 0.0 and lt.slot_case(S, "dep", 1, "10:10 a.m.") == {"i"}


def _slots(S, draws):
    """every slot the weights program can have: (sweep, row, particle, value); particle 0 = the retained drawn times"""
    out = [(sw, t, p, v) for (sw, t, p), v in draws.items()]
    out += [(sw, t, 0, v) for sw in range(len(lt.PARTICLES)) for t, (_, v) in lt.W_HELD.items()]
    return out


def test_every_case_occurs_in_the_weights_program(wprog):
    S, draws = wprog
    n = {"i": 0, "ii": 0, "iii-missing": 0, "iii": 0}
    rows = {k: set() for k in n}
    for (sw, t, p), v in draws.items():
        if t in lt.W_EXPLAINED:
            continue
        for c in lt.slot_case(S, "dep", t, v):
            n[c] += 1
            rows[c].add(t)
    held = len(lt.W_HELD) * len(lt.PARTICLES)
    print(f"cases among the fresh particles' times: {n}; retained drawn times: {held}")
    assert n["i"] >= lt.W_MIN_CASE, "case (i): add a row whose observations repeat no drawn time"
    assert n["ii"] >= lt.W_MIN_CASE, "case (ii): observe a drawn time of the row's own particles that is no atom of its key"
    assert n["iii-missing"] >= lt.W_MIN_CASE, ("case (iii): make a drawn time of a row with a missing observation an atom of "
                                               "its key (one the time pattern rejects, or the dummy is never drawn)")
    assert held >= lt.W_MIN_CASE, "retained drawn times: add a row to W_HELD"
    assert rows["ii"] >= set(lt.W_ENTRIES), "every lane-stride shape should hold an observed drawn time"
    # three keys with different atom counts, one with none; the shapes of the lane stride
    counts = {k: len(lt.atoms_of(S, "dep", k)) for k in lt.KEYS}
    assert counts["kc"] == 0 and len(set(counts.values())) == 3
    shapes = {t: len(lt.evidence_of(S, "dep", t)) for t in range(lt.W_N_TRIPS)}
    assert {0, 1, 63, 64, 65, 130} <= set(shapes.values()) and shapes[0] == 0
    # the held times are no options of their rows' keys, and the rows hold them under drawn-value ids
    lw = S["lw"]
    for t, (key, v) in lt.W_HELD.items():
        assert v not in lt.atoms_of(S, "dep", key)
        assert int(S["trace"].tables["Trip"].cols[lw.colidx["Trip"]["dep"], t]) == lw.latent_dom[("Trip", "dep")].extra[v]


def _misread(S, trip, v, kind):
    """c(v) of (trip, dep) as a kernel that commits misreading `kind` would compute it"""
    key = S["trips"][trip]["key"]
    other = {"ka": "kb", "kb": "ka", "kc": "kb"}[key]
    ph = lt.dist_of(S, "dep").dummy_value()
    ev = lt.evidence_of(S, "dep", trip)
    terms = [-lt.dummy_mass_log(S, "dep", other if kind == "mass" else key)]
    probs = sorted({p for _, p, _ in ev})
    for o, prob, n in ev:
        kw = {}
        if kind == "n_options":
            kw = dict(n_options=len(lt.atoms_of(S, "dep", other)))
        if kind == "prob" and len(probs) > 1:
            prob = probs[(probs.index(prob) + 1) % len(probs)]
        if kind == "missing" and o is None:
            continue
        if kind == "by_id":
            kw = dict(options=[], n_options=len(lt.atoms_of(S, "dep", key)))  # a drawn time has no id among the options
        terms.append(n * lt.density(S, "dep", key, o, prob, v, **kw))
        terms.append(-n * lt.density(S, "dep", key, o, prob, ph, **({} if kind == "by_id" else kw)))
    return math.fsum(terms)


@pytest.mark.parametrize("kind", ["mass", "n_options", "prob", "by_id", "missing"])
def test_misreadings_move_a_dozen_slots(wprog, kind):
    S, draws = wprog
    moved = 0
    for sw, t, p, v in _slots(S, draws):
        c, tol = lt.slot_correction(S, "dep", t, v)
        tol = max(tol, 2.0 ** -1000)
        if abs(_misread(S, t, v, kind) - c) >= 1000.0 * tol:
            moved += 1
    print(f"{kind}: {moved} slots move by 1000 tolerances or more")
    assert moved >= 12, kind


@pytest.mark.parametrize("name,mh,atoms_id,state", lt.DIST_CASES, ids=[c[0] for c in lt.DIST_CASES])
def test_closed_forms_and_power(name, mh, atoms_id, state):
    S = lt.dist_program(atoms_id, state)
    ev, atoms = lt.dist_evidence(S), lt.DIST_ATOMS[atoms_id]
    assert sum(n for _, _, n in ev) == len(lt.DIST_OBS)
    exact = lt.kernel(atoms, ev, state, mh)
    assert abs(math.fsum(exact.values()) - 1.0) <= 1e-12
    rng = np.random.default_rng(11)
    ok = pe.gof([(0, exact, lt.simulate(atoms, ev, state, mh, N_DRAWS, rng))])
    bad = pe.gof([(0, exact, lt.simulate(atoms, ev, state, mh, N_DRAWS, rng, corrected=False))])
    print(f"{name}: mechanism {pe.describe(ok)}\n{name}: uncorrected {pe.describe(bad)}; pooled mass "
          f"{pe.pooled_mass([exact], N_DRAWS):.4f}")
    assert ok["p"] > pe.ALPHA, pe.describe(ok)
    assert bad["p"] < 1e-6, pe.describe(bad)
    flat = lt.kernel(atoms, ev, state, mh, corrected=False)
    again = pe.gof([(0, flat, lt.simulate(atoms, ev, state, mh, N_DRAWS, rng, corrected=False))])
    assert again["p"] > pe.ALPHA, pe.describe(again)


# ---- host logic --------------------------------------------------------------------------------------------------
def _served(lw, cname, keyed=True):
    from pclean_amd.engine import Engine
    return Engine.latent_dummy_served(types.SimpleNamespace(lw=lw, latent_dummy_keyed=keyed), cname)


def test_served_choices_are_reported(wprog):
    import helpers
    F = helpers.flights_setup()
    # keyed choices are served while the engine's switch is on (latent_sweep turns it on); off, as before
    assert _served(F["lw"], "Flight", keyed=False) == [] and _served(wprog[0]["lw"], "Trip", keyed=False) == ["label"]
    assert _served(F["lw"], "Flight") == ["sdt", "sat", "adt", "aat"]  # (flight_id: an equality term, as before)
    assert _served(F["lw"], "TrackingWebsite") == []
    R = helpers.rents_setup(n_rows=200)
    assert _served(R["lw"], "County") == ["name"]
    S, _ = wprog
    assert _served(S["lw"], "Trip") == ["dep", "label"] and _served(S["lw"], "Src") == []
    assert _served(lt.keyed_string_program()["lw"], "Trip") == ["name"]


def test_excl_and_dummy_options_go_by_the_rows_key():
    from pclean_amd.engine import Engine, InferenceConfig
    from pclean_amd.inference import latent_current_choices
    T = lt.keyed_string_program()
    lw, tr = T["lw"], T["trace"]
    rows = np.arange(len(T["trips"]))
    cfg = InferenceConfig(1, 2)
    pl = lw.latent_plans["Trip"]
    r_name = pl["root_attr"].index("name")
    assert (latent_current_choices(lw, tr, "Trip", rows, cfg) == -1).all()  # flag off: as before
    excl = latent_current_choices(lw, tr, "Trip", rows, cfg, ["name"])
    dom = lw.latent_dom[("Trip", "name")]
    for t in rows:
        key, v = T["trips"][t]["key"], T["trips"][t]["name"]
        if t in T["held"]:  # "qqqqq" under kb is ka's atom: no option of kb
            assert excl[r_name, t] == lt.value_id(T, "name", key, v) >= 0, t
        else:
            assert excl[r_name, t] == -1, t
    assert dom.string(int(excl[r_name, sorted(T["held"])[1]])) == "qqqqq"
    assert (np.delete(excl, r_name, axis=0) == -1).all()
    # the dummy option of every row's key
    eng = types.SimpleNamespace(lw=lw, latent_dummy_served=lambda c: ["name"])
    dk = Engine.latent_dummy_options(eng, tr, "Trip", rows)
    vals, keys = lw.option_values[("Trip", "name")], lw.option_keycol[("Trip", "name")]
    kdom = lw.latent_dom[("Trip", "key")]
    dummy = dom.get(lt.dist_of(T, "name").dummy_value())
    for t in rows:
        k = int(dk[r_name, t])
        assert vals[k] == dummy and kdom.string(int(keys[k])) == T["trips"][t]["key"]
    assert (np.delete(dk, r_name, axis=0) == -1).all()
    assert Engine.latent_dummy_options(types.SimpleNamespace(lw=lw, latent_dummy_served=lambda c: []), tr, "Trip", rows) is None


class _StubEngine:
    """what resample_dummies asks of an engine, with the oracle's samplers"""

    def __init__(self, oracle, S):
        self.oracle, self.lw, self.obs = oracle, S["lw"], S["obs"]

    def latent_dummy_served(self, cname):
        return _served(self.lw, cname)

    def sample_prior_strings(self, dist, n, seed, stream):
        from pclean_amd import sampling
        from pclean_amd.model import TimePrior
        ro = self.oracle.RandomOracle()
        if isinstance(dist, TimePrior):
            return sampling.random_time_prior(ro, n, seed=seed, stream=stream)
        return sampling.random_string_prior(ro, n, dist.min_len, dist.max_len, seed=seed, stream=stream)

    def sample_prior_strings_at(self, dist, seeds, elems):
        from pclean_amd import sampling
        from pclean_amd.model import TimePrior
        if isinstance(dist, TimePrior):
            return [lt.time_at(self.oracle, k, e) for k, e in zip(seeds, elems)]
        return sampling.random_string_prior_at(self.oracle.RandomOracle(), seeds, elems, dist.min_len, dist.max_len)

    def reload(self):
        pass


def test_latent_sweep_turns_keyed_serving_on():
    """latent_sweep(dummy_correction=True) fills excl by key and has the engine name the rows' dummy options: it turns the
    switch on before it asks what is served; without the flag it leaves the switch alone"""
    from pclean_amd.engine import InferenceConfig
    from pclean_amd.inference import latent_sweep
    T = lt.keyed_string_program()
    asked = []

    def served(cname):
        asked.append(eng.latent_dummy_keyed)
        raise KeyboardInterrupt  # (far enough)

    eng = types.SimpleNamespace(lw=T["lw"], latent_dummy_keyed=False, latent_dummy_served=served)
    with pytest.raises(KeyboardInterrupt):
        latent_sweep(eng, T["trace"], "Trip", InferenceConfig(1, 2), 1, 0, dummy_correction=True)
    assert asked == [True]


def test_a_committed_dummy_gets_the_time_of_its_recorded_origin(oracle):
    from pclean_amd.inference import commit_latent, resample_dummies
    S, draws = lt.weights_program(oracle)
    lw, tr = S["lw"], S["trace"]
    pl = lw.latent_plans["Trip"]
    nn = len(pl["nodes"])
    root = {a: pl["roots"][pl["root_attr"].index(a)] for a in ("key", "dep", "label")}
    vals_d, keys_d = lw.option_values[("Trip", "dep")], lw.option_keycol[("Trip", "dep")]
    dom, kdom = lw.latent_dom[("Trip", "dep")], lw.latent_dom[("Trip", "key")]
    dummy = dom.get(lt.dist_of(S, "dep").dummy_value())
    live = np.arange(lt.W_N_TRIPS)
    chosen = np.zeros(len(live), dtype=np.int32)
    vals = np.full((len(live), nn), -2, dtype=np.int32)
    sweep = len(lt.PARTICLES) - 1
    picked = {3: 17, 8: 40, 12: 5}  # row -> chosen particle; each takes the dummy of its key
    t_tab = tr.tables["Trip"]
    for t in live:
        key_id = int(t_tab.cols[lw.colidx["Trip"]["key"], t])
        vals[t, root["key"]] = int(np.flatnonzero(lw.option_values[("Trip", "key")] == key_id)[0])
        vals[t, root["label"]] = 0
        vals[t, root["dep"]] = int(np.flatnonzero((vals_d == dummy) & (keys_d == key_id))[0])
        chosen[t] = picked.get(int(t), 0)
    commit_latent(lw, tr, "Trip", live, chosen, vals, (["dep", "label"], sweep))
    assert {k: v for k, v in tr.row_origin.items()} == {("Trip", t): (t, p, sweep, pl["block_id"]) for t, p in picked.items()}
    assert resample_dummies(_StubEngine(oracle, S), tr, lt.SEED, 1) > 0
    dom = lw.latent_dom[("Trip", "dep")]
    for t, p in picked.items():
        now = dom.string(int(tr.tables["Trip"].cols[lw.colidx["Trip"]["dep"], t]))
        assert now == draws[(sweep, t, p)], (t, p, now, draws[(sweep, t, p)])
    # a drawn time that is an atom of the row's key is held as that option, anything else as a drawn value
    for t, p in picked.items():
        vid = int(tr.tables["Trip"].cols[lw.colidx["Trip"]["dep"], t])
        assert (vid < dummy) == (draws[(sweep, t, p)] in lt.atoms_of(S, "dep", S["trips"][t]["key"]))
    assert not (tr.tables["Trip"].cols[lw.colidx["Trip"]["dep"], :lt.W_N_TRIPS] == dummy).any()  # no placeholder left
