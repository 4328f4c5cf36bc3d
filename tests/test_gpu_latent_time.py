"""Latent sweeps with dummy_correction on the device for KEYED choices — TimePrior under MaybeSwap evidence (flights' Flight)
and keyed StringPrior under AddTypos evidence (rents' County) — against the float64 restatement and the closed forms of
tests/latent_time_program.py (values from the oracle's C++ samplers, densities from oracle/literal.py;
tests/test_latent_time_cpu.py shows what those are worth).

Weights: pclean_get_latent_weights for every (row, particle) of latent_time_program.weights_program — rows with 0, 1, 63,
64, 65 and 130 aggregated evidence entries, five error probabilities, three keys (no atoms, pattern atoms, atoms the time
pattern rejects), missing observations, rows that hold drawn times, an unkeyed StringPrior choice served in the same call
(string slots and time slots together, the string slots cut into arena slices) — and of the keyed-StringPrior twin; P = 2
(MH), 2, 64.  The tolerance of a slot is 4 k 2^-53 sum |summand| over the k summands of its restatement
(tests/test_gpu_latent_dummy.py derives it); a particle without a slot weighs exactly 0.  A fresh particle's weight is
checked exactly where the sweep returns its draws (the chosen particle) and as one of the sums over a subset of its served
choices elsewhere.

Measured on an MI355X: the weights program — 980 fresh particles with slots (499 time slots told from "no slot", 776 string
slots; cases (i) 387, (ii) 73, (iii) with a missing observation 28, (iii) 11), 12 retained slots, the worst 0.064 of its
tolerance; the twin — 578 and 9, the worst 0.024; the four distribution cases at 10 240 draws each: p = 0.055, 0.18, 0.67,
0.39 (the bar is posterior_exact.ALPHA = 1e-4; the uncorrected kernel: p < 1e-12 on the CPU twin)."""
import itertools
import os

import numpy as np
import pytest

import latent_time_program as lt
import posterior_exact as pe
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import build_evidence, latent_current_choices

pytestmark = pytest.mark.gpu

SEED = lt.SEED


def _engine(S):
    """an engine that serves keyed choices (what inference.latent_sweep turns on)"""
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    eng.latent_dummy_keyed = True
    return eng


def _setup(S, eng, served=None):
    lw, tr = S["lw"], S["trace"]
    eng.upload_trace(tr)
    live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "Trip")
    served = eng.latent_dummy_served("Trip") if served is None else served
    excl = latent_current_choices(lw, tr, "Trip", live, InferenceConfig(1, 2), served)
    return live, ev_off, ev_rows, ev_ctx, excl


def _sweep(eng, S, args, P, mh, sweep_idx, on):
    live, ev_off, ev_rows, ev_ctx, excl = args
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
    if not on:
        excl = np.full_like(excl, -1)
    chosen, vals = eng.sweep_latent(S["trace"], "Trip", cfg, SEED, sweep_idx, live, ev_off, ev_rows, ev_ctx, excl,
                                    dummy_correction=on)
    return chosen.copy(), vals.copy(), (eng.latent_weights() if on else None)


def test_keyed_time_sampler_equals_the_oracle(hip, oracle):
    from pclean_amd import sampling
    seeds = [sampling.dummy_seed(SEED, (3 << 16) | 1, p, s) for p in range(1, 65) for s in range(3)]
    elems = [(7 * i) % 300 for i in range(len(seeds))]
    got = sampling.random_time_prior_at(hip, seeds, elems)
    assert got == [lt.time_at(oracle, k, e) for k, e in zip(seeds, elems)]
    assert sampling.random_time_prior_at(hip, [], []) == []
    # stream 0 of the unkeyed sampler at the same key is the same stream
    assert sampling.random_time_prior(hip, 40, seed=seeds[0], stream=0) == sampling.random_time_prior_at(hip, [seeds[0]] * 40,
                                                                                                        list(range(40)))


def _check_weights(oracle, S, eng, args, P, mh, sweep_idx, memo, restricted=False):
    """one corrected sweep against the restatement; returns (weights, chosen, vals, statistics)"""
    lw = S["lw"]
    pl = lw.latent_plans["Trip"]
    live, ev_off, ev_rows, ev_ctx, excl = args
    chosen, vals, w = _sweep(eng, S, args, P, mh, sweep_idx, True)
    n = len(live)
    assert w.shape == (n, P)
    attrs = eng.latent_dummy_served("Trip")
    roots = {a: pl["roots"][pl["root_attr"].index(a)] for a in attrs}
    ridx = {a: pl["root_attr"].index(a) for a in attrs}
    dummy_opt = {a: lw.latent_dom[("Trip", a)].get(lt.dist_of(S, a).dummy_value()) for a in attrs}
    drawn = {}
    for a in attrs:
        ps = [p for t in range(n) for p in range(1, P)]
        ks = [int(live[t]) for t in range(n) for p in range(1, P)]
        ss = lt.drawn_values(oracle, S, a, SEED, ps, sweep_idx, ks)
        drawn[a] = {(t, p): s for (t, p), s in zip(((t, p) for t in range(n) for p in range(1, P)), ss)}

    def corr(a, t, v):
        key = (id(S), a, t, v, restricted)
        if key not in memo:
            memo[key] = lt.slot_correction(S, a, int(live[t]), v, restricted)
        return memo[key]

    st = dict(slots=0, exact=0, p0=0, worst=0.0, rows=set(), cases={}, by_attr={a: 0 for a in attrs}, zero=0)
    for t in range(n):
        want, tol, any0 = 0.0, 0.0, False
        for a in attrs:
            v = int(excl[ridx[a], t])
            if v >= 0:
                c, e = corr(a, t, lw.latent_dom[("Trip", a)].string(v))
                want, tol, any0 = want + c, tol + e, True
                st["p0"] += 1
        if not any0:
            assert w[t, 0] == 0.0, (t, w[t, 0])
            st["zero"] += 1
        else:
            assert abs(w[t, 0] - want) <= tol, (t, 0, w[t, 0], want, tol)
            st["worst"] = max(st["worst"], abs(w[t, 0] - want) / tol if tol else 0.0)
        for p in range(1, P):
            cs = [corr(a, t, drawn[a][(t, p)]) for a in attrs]
            if p == chosen[t]:  # its draws came back: which choices took the dummy is known
                took = [lw.option_values[("Trip", a)][vals[t, roots[a]]] == dummy_opt[a] for a in attrs]
                subsets = [tuple(took)]
                st["exact"] += any(took)
                if not any(took):
                    assert w[t, p] == 0.0, (t, p, w[t, p])  # no slot: exactly 0
                    st["zero"] += 1
                    continue
            else:
                subsets = list(itertools.product((False, True), repeat=len(attrs)))
            if w[t, p] == 0.0 and not all(any(sub) for sub in subsets):
                st["zero"] += 1
                continue
            ok = False
            for sub in subsets:
                if not any(sub):
                    continue
                want = sum(c for (c, e), on in zip(cs, sub) if on)
                tol = sum(e for (c, e), on in zip(cs, sub) if on)
                if abs(w[t, p] - want) <= tol:
                    ok = True
                    st["worst"] = max(st["worst"], abs(w[t, p] - want) / tol if tol else 0.0)
                    for a, on in zip(attrs, sub):
                        if on:
                            st["by_attr"][a] += 1
                            if lt.is_time(S, a):
                                for cse in lt.slot_case(S, a, int(live[t]), drawn[a][(t, p)]):
                                    st["cases"][cse] = st["cases"].get(cse, 0) + 1
                    break
            assert ok, (t, p, w[t, p], cs, subsets, [drawn[a][(t, p)] for a in attrs])
            st["slots"] += 1
            st["rows"].add(int(live[t]))
    return w, chosen, vals, st


def _weights_case(oracle, S, arena_slots, lane_cells):
    memo = {}
    eng = _engine(S)
    total = dict(slots=0, exact=0, p0=0, worst=0.0, rows=set(), cases={}, by_attr={}, zero=0, unchanged=0)
    try:
        args = _setup(S, eng)
        for sweep_idx, (P, mh) in enumerate(lt.PARTICLES):
            w, chosen, vals, st = _check_weights(oracle, S, eng, args, P, mh, sweep_idx, memo)
            for k in ("slots", "exact", "p0", "zero"):
                total[k] += st[k]
            total["rows"] |= st["rows"]
            total["worst"] = max(total["worst"], st["worst"])
            for k, v in st["cases"].items():
                total["cases"][k] = total["cases"].get(k, 0) + v
            for k, v in st["by_attr"].items():
                total["by_attr"][k] = total["by_attr"].get(k, 0) + v
            # determinism
            chosen2, vals2, w2 = _sweep(eng, S, args, P, mh, sweep_idx, True)
            assert np.array_equal(w, w2) and np.array_equal(chosen, chosen2) and np.array_equal(vals, vals2)
            # unchanged where nothing applies
            chosen0, vals0, _ = _sweep(eng, S, args, P, mh, sweep_idx, False)
            quiet = np.flatnonzero((w == 0.0).all(axis=1))
            assert np.array_equal(chosen[quiet], chosen0[quiet]) and np.array_equal(vals[quiet], vals0[quiet]), (P, mh)
            total["unchanged"] += len(quiet)
            if P == 64 and arena_slots:  # the string slots of the same call in slices of arena_slots slots
                os.environ["PCLEAN_LATENT_DUMMY_ARENA"] = str(arena_slots * 64 * lane_cells)
                try:
                    chosen3, vals3, w3 = _sweep(eng, S, args, P, mh, sweep_idx, True)
                finally:
                    del os.environ["PCLEAN_LATENT_DUMMY_ARENA"]
                assert np.array_equal(w, w3) and np.array_equal(chosen, chosen3) and np.array_equal(vals, vals3)
                total["string_slots_64"] = sum(v for k, v in st["by_attr"].items() if not lt.is_time(S, k))
    finally:
        eng.close()
    return total


def test_time_weights_equal_the_restatement(oracle):
    """every (row, particle) of the weights program: TimePrior slots and the slots of an unkeyed StringPrior in one call"""
    S, draws = lt.weights_program(oracle)
    lane_cells = (4 + 2) * (lt.W_LABEL_LEN + 2)  # (longest observed label: 4 symbols)
    assert max(len(r["label"]) for r in S["rows"] if r.get("label")) == 4
    total = _weights_case(oracle, S, 4, lane_cells)
    print(f"\n[time] {total['slots']} fresh particles with slots ({total['exact']} through the chosen particle's draws), by "
          f"choice {total['by_attr']}, cases {total['cases']}, {total['p0']} retained slots, worst error "
          f"{total['worst']:.3f} of its tolerance, {total['zero']} particles without a slot, {total['unchanged']} rows "
          f"without a correction")
    assert total["p0"] == len(lt.W_HELD) * len(lt.PARTICLES)
    assert total["rows"] >= {0, 1} | set(lt.W_ENTRIES) | set(lt.W_KA_ROWS) | set(lt.W_HELD), sorted(total["rows"])
    for case in ("i", "ii", "iii-missing"):
        assert total["cases"].get(case, 0) >= lt.W_MIN_CASE, (case, total["cases"])
    # (the seven kb rows that are not explained have 1 + 1 + 63 fresh particles each over the three sweeps, and a kb particle
    # takes the dummy with probability 1440 / 1450: about 450 slots whose correction, -log m_d(kb) at the least, is not 0 and
    # so tells them from "no slot"; the slots of ka and kc weigh exactly 0 in case (i) and are counted with the particles
    # without a slot)
    assert total["by_attr"]["dep"] >= 400 and total["exact"] >= 10 and total["zero"] >= 10
    # one call held string slots and time slots, the string slots in more than one arena slice
    assert total["string_slots_64"] > 4, total["string_slots_64"]


def test_keyed_string_weights_equal_the_restatement(oracle):
    """the keyed-StringPrior twin: the string path with the dummy mass of the row's own key"""
    S = lt.keyed_string_program()
    longest = max(len(r["name"]) for r in S["rows"] if r.get("name"))
    total = _weights_case(oracle, S, 4, (longest + 2) * (5 + 2))
    print(f"\n[keyed strings] {total['slots']} fresh particles with slots ({total['exact']} through the chosen particle's "
          f"draws), {total['p0']} retained slots, worst error {total['worst']:.3f} of its tolerance, {total['zero']} "
          f"particles without a slot")
    assert total["p0"] == len(S["held"]) * len(lt.PARTICLES)
    # rows 1 .. 6: no observed name, then 1 / 63 / 64 / 65 / 130 distinct ones (row 0, of the key without atoms and with no
    # evidence, weighs -log 1 = 0 exactly: it cannot be told from a particle without a slot)
    assert [len(lt.evidence_of(S, "name", t)) for t in range(7)] == [0, 0, 1, 63, 64, 65, 130]
    assert total["rows"] >= set(range(1, 7)) | set(S["held"]), sorted(total["rows"])
    assert {S["trips"][t]["key"] for t in total["rows"]} == set(lt.KEYS)
    assert total["slots"] >= 300 and total["exact"] >= 5 and total["string_slots_64"] > 8


def test_committed_rows_hold_the_times_that_were_weighed(oracle, monkeypatch):
    """latent_sweep(..., dummy_correction=True): every row whose served choice took the dummy holds the value of its recorded
    key, by the oracle's samplers"""
    from pclean_amd import inference as inf
    S, _ = lt.weights_program(oracle)
    lw, tr = S["lw"], S["trace"]
    served = ("dep", "label")
    seen = {}
    real = inf.commit_latent

    def spy(lw_, tr_, cname, live, chosen, vals, *a):
        seen.update(live=np.array(live), chosen=np.array(chosen), vals=np.array(vals),
                    opt={x: lw_.option_values[("Trip", x)].copy() for x in served},
                    dummy={x: lw_.latent_dom[("Trip", x)].get(lt.dist_of(S, x).dummy_value()) for x in served})
        return real(lw_, tr_, cname, live, chosen, vals, *a)

    monkeypatch.setattr(inf, "commit_latent", spy)
    eng = Engine(lw, S["obs"], dist_mode=1)
    try:
        eng.upload_trace(tr)
        assert eng.latent_dummy_served("Trip") == ["label"]  # (latent_sweep turns keyed serving on)
        pl = lw.latent_plans["Trip"]
        block_id, roots = pl["block_id"], {a: pl["roots"][pl["root_attr"].index(a)] for a in served}
        before = {a: [lw.latent_dom[("Trip", a)].string(int(v))
                      for v in tr.tables["Trip"].cols[lw.colidx["Trip"][a], :tr.tables["Trip"].n]] for a in served}
        inf.latent_sweep(eng, tr, "Trip", InferenceConfig(1, 5), SEED, 3, dummy_correction=True)
        assert eng.latent_dummy_served("Trip") == list(served)
        t = tr.tables["Trip"]
        n_checked = {a: 0 for a in served}
        for k, row in enumerate(seen["live"]):
            p = int(seen["chosen"][k])
            for a in served:
                dom = lw.latent_dom[("Trip", a)]
                now = dom.string(int(t.cols[lw.colidx["Trip"][a], row]))
                if p > 0 and seen["opt"][a][seen["vals"][k, roots[a]]] == seen["dummy"][a]:
                    assert tr.row_origin[("Trip", int(row))] == (int(row), p, 3, block_id)
                    want = lt.drawn_values(oracle, S, a, SEED, [p], 3, [int(row)])[0]
                    assert now == want, (row, a, now, want)
                    n_checked[a] += 1
                elif p == 0 and before[a][row] != lt.dist_of(S, a).dummy_value():
                    assert now == before[a][row]  # (a row that held the placeholder gets a draw of the commit's stream)
                assert now != lt.dist_of(S, a).dummy_value()  # no placeholder left
        assert n_checked["dep"] >= 5, n_checked
    finally:
        eng.close()


@pytest.mark.parametrize("name,mh,atoms_id,state", lt.DIST_CASES, ids=[c[0] for c in lt.DIST_CASES])
def test_draws_follow_the_closed_forms(oracle, name, mh, atoms_id, state):
    """DIST_SWEEPS sweeps from a frozen state over DIST_ROWS identical rows against latent_time_program.kernel; the
    uncorrected sweep fails the same test: tests/test_latent_time_cpu.py"""
    S = lt.dist_program(atoms_id, state)
    lw = S["lw"]
    atoms = lt.DIST_ATOMS[atoms_id]
    exact = lt.kernel(atoms, lt.dist_evidence(S), state, mh)
    eng = _engine(S)
    try:
        args = _setup(S, eng)
        live = args[0]
        assert eng.latent_dummy_served("Trip") == ["dep"]
        pl = lw.latent_plans["Trip"]
        r = pl["root_attr"].index("dep")
        root = pl["roots"][r]
        assert ((args[4][r] >= 0).all()) == (state not in atoms)
        opt = lw.option_values[("Trip", "dep")]
        dom = lw.latent_dom[("Trip", "dep")]
        dummy = dom.get(lt.dist_of(S, "dep").dummy_value())
        counts = {}
        for s in range(lt.DIST_SWEEPS):
            chosen, vals, w = _sweep(eng, S, args, 2, mh, s, True)
            fresh = np.flatnonzero(chosen > 0)
            took = fresh[opt[vals[fresh, root]] == dummy]
            times = dict(zip(took.tolist(), lt.drawn_values(oracle, S, "dep", SEED, chosen[took], s, live[took])))
            for t in range(len(live)):
                if chosen[t] == 0:
                    got = state
                elif t in times:
                    got = times[t]
                else:
                    got = dom.string(int(opt[vals[t, root]]))
                counts[got] = counts.get(got, 0) + 1
        res = pe.gof([(0, exact, counts)])
        print(f"\n[{name}] {pe.describe(res)}")
        assert res["n"] == lt.DIST_ROWS * lt.DIST_SWEEPS
        assert res["p"] > pe.ALPHA, pe.describe(res)
    finally:
        eng.close()


@pytest.mark.parametrize("program", ["time", "keyed-string"])
def test_flag_off_and_keyed_serving_off_sweep_to_the_same_bits(program):
    """the flag off, and the flag on with the engine's keyed serving off (latent_dummy_served is empty, no row names a dummy
    option of its key: what the sweeps did before keyed choices were served): the same choices and values, every weight 0"""
    S = lt.dist_program("few", lt.DIST_HELD) if program == "time" else lt.keyed_string_program()
    eng = _engine(S)
    try:
        args = _setup(S, eng)
        assert (args[4] >= 0).any()
        for sweep_idx, (P, mh) in enumerate(lt.PARTICLES):
            off = _sweep(eng, S, args, P, mh, sweep_idx, False)
            on = _sweep(eng, S, args, P, mh, sweep_idx, True)
            assert on[2].any()
            eng.latent_dummy_keyed = False
            try:
                assert eng.latent_dummy_served("Trip") == []
                bare = _setup(S, eng)
                assert (bare[4] == -1).all()
                none = _sweep(eng, S, bare, P, mh, sweep_idx, True)
            finally:
                eng.latent_dummy_keyed = True
            assert none[2].shape == (len(args[0]), P) and not none[2].any()
            assert np.array_equal(none[0], off[0]) and np.array_equal(none[1], off[1])
            again = _sweep(eng, S, args, P, mh, sweep_idx, False)  # (a flagged sweep leaves nothing behind)
            assert np.array_equal(again[0], off[0]) and np.array_equal(again[1], off[1])
    finally:
        eng.close()


def test_flights_serves_its_times_and_stays_consistent():
    """the real flights lowering: the four times are served, and one flagged iteration leaves a consistent trace"""
    import helpers
    from pclean_amd.inference import run_inference
    F = helpers.flights_setup()
    lw, tr = F["lw"], F["trace"]
    eng = Engine(lw, F["obs"], dist_mode=1)
    try:
        assert eng.latent_dummy_served("Flight") == []  # (a bare engine: as before)
        run_inference(eng, tr, InferenceConfig(1, 2, use_mh_instead_of_pg=True, rejuv_frequency=500), SEED,
                      latent_dummy_correction=True)
        assert eng.latent_dummy_served("Flight") == ["sdt", "sat", "adt", "aat"]
        assert eng.latent_dummy_served("TrackingWebsite") == []
        tr.check_consistency()
        for a in ("sdt", "sat", "adt", "aat"):  # no placeholder survives a commit
            d = lw.model.classes["Flight"].attr(a).dist
            t = tr.tables["Flight"]
            col = t.cols[lw.colidx["Flight"][a], :t.n][t.live[:t.n]]
            assert not (col == lw.latent_dom[("Flight", a)].get(d.dummy_value())).any()
    finally:
        eng.close()
