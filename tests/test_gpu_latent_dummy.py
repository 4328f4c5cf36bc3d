"""Latent sweeps with dummy_correction on the device (pclean_set_latent_dummy_correction, csrc/latent.hip) against the
float64 restatement and the closed forms of tests/latent_dummy_program.py (strings from the oracle's C++ sampler,
densities from oracle/literal.py; tests/test_latent_dummy_cpu.py shows what those are worth).

Weights: pclean_get_latent_weights for every (row, particle) of latent_dummy_program.weights_program — rows with 0, 1, 63,
64, 65 and 300 distinct observed values, multiplicities above 1, drawn lengths 1 .. 6, observed lengths 1 .. 40, missing
observations, two terms on one choice (max_typos unset and set), two served choices, rows that hold drawn strings
(particle-0 slots); both distance flavours; P = 2 (MH), 2, 5, 64; a launch cut into arena slices.  The tolerance of a
slot is 4 k 2^-53 sum |summand| over the k summands of its restatement.  A fresh particle's weight is checked against
the corrections of its served choices: exactly, where the sweep returns the particle's draws (the chosen particle), and as
one of the sums over a subset of its choices elsewhere (which draws took the dummy is not returned for the others).

Measured on an MI355X: 621 fresh and 12 retained slots per flavour, the worst 0.040 of its tolerance; 156 (observed,
drawn) pairs on which the two flavours differ; the four distribution cases at 10 240 draws each: p = 0.53, 0.35, 0.075,
0.038 (the bar is posterior_exact.ALPHA = 1e-4; the uncorrected kernel: p < 1e-300 on the CPU twin)."""
import itertools
import os

import numpy as np
import pytest

import latent_dummy_program as ld
import posterior_exact as pe
from pclean_amd import _lib
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import build_evidence, latent_current_choices

pytestmark = pytest.mark.gpu

SEED = 4242
PARTICLES = [(2, True), (2, False), (5, False), (64, False)]


def _setup(S, eng, served=None):
    lw, tr = S["lw"], S["trace"]
    eng.upload_trace(tr)
    live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "Item")
    served = eng.latent_dummy_served("Item") if served is None else served
    excl = latent_current_choices(lw, tr, "Item", live, InferenceConfig(1, 2), served)
    return live, ev_off, ev_rows, ev_ctx, excl


def _sweep(eng, S, args, P, mh, sweep_idx, on):
    live, ev_off, ev_rows, ev_ctx, excl = args
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
    if not on:
        excl = np.full_like(excl, -1)
    chosen, vals = eng.sweep_latent(S["trace"], "Item", cfg, SEED, sweep_idx, live, ev_off, ev_rows, ev_ctx, excl,
                                    dummy_correction=on)
    return chosen.copy(), vals.copy(), (eng.latent_weights() if on else None)


@pytest.fixture(scope="module")
def wprog():
    return ld.weights_program()


@pytest.fixture(scope="module")
def memo():
    return {}


def _check_weights(oracle, S, eng, args, P, mh, sweep_idx, restricted, memo):
    """one corrected sweep against the restatement; returns (weights, chosen, vals, statistics)"""
    lw, tr = S["lw"], S["trace"]
    pl = lw.latent_plans["Item"]
    live, ev_off, ev_rows, ev_ctx, excl = args
    chosen, vals, w = _sweep(eng, S, args, P, mh, sweep_idx, True)
    n = len(live)
    assert w.shape == (n, P)
    attrs = eng.latent_dummy_served("Item")
    roots = {a: pl["roots"][pl["root_attr"].index(a)] for a in attrs}
    ridx = {a: pl["root_attr"].index(a) for a in attrs}
    dummy_opt = {a: lw.latent_dom[("Item", a)].get(lw.model.classes["Item"].attr(a).dist.dummy_value()) for a in attrs}
    # the strings of every fresh particle, from the oracle's sampler
    drawn = {}
    for a in attrs:
        ps = [p for t in range(n) for p in range(1, P)]
        ks = [int(live[t]) for t in range(n) for p in range(1, P)]
        ss = ld.drawn_strings(oracle, lw, a, SEED, pl["block_id"], roots[a], ps, sweep_idx, ks)
        drawn[a] = {(t, p): s for (t, p), s in zip(((t, p) for t in range(n) for p in range(1, P)), ss)}

    def corr(a, t, v):
        key = (a, t, v, restricted)
        if key not in memo:
            memo[key] = ld.slot_correction(S, a, int(live[t]), v, restricted)
        return memo[key]

    st = dict(slots=0, exact=0, p0=0, lens=set(), flavour=0, worst=0.0, items=set())
    for t in range(n):
        # particle 0: the drawn strings the row holds
        want, tol = 0.0, 0.0
        for a in attrs:
            v = int(excl[ridx[a], t])
            if v >= 0:
                c, e = corr(a, t, lw.latent_dom[("Item", a)].string(v))
                want, tol = want + c, tol + e
                st["p0"] += 1
        if tol == 0.0:
            assert w[t, 0] == 0.0, (t, w[t, 0])
        else:
            assert abs(w[t, 0] - want) <= tol, (t, 0, w[t, 0], want, tol)
            st["worst"] = max(st["worst"], abs(w[t, 0] - want) / tol)
        for p in range(1, P):
            cs = [corr(a, t, drawn[a][(t, p)]) for a in attrs]
            if p == chosen[t]:  # its draws came back: which choices took the dummy is known
                took = [lw.option_values[("Item", a)][vals[t, roots[a]]] == dummy_opt[a] for a in attrs]
                subsets = [tuple(took)]
                st["exact"] += any(took)
            else:
                subsets = list(itertools.product((False, True), repeat=len(attrs)))
            if w[t, p] == 0.0 and not all(any(sub) for sub in subsets):
                continue
            ok = False
            for sub in subsets:
                if not any(sub):
                    continue
                want = sum(c for (c, e), on in zip(cs, sub) if on)
                tol = sum(e for (c, e), on in zip(cs, sub) if on)
                if abs(w[t, p] - want) <= tol:
                    ok = True
                    st["worst"] = max(st["worst"], abs(w[t, p] - want) / tol)
                    for a, on in zip(attrs, sub):
                        if on:
                            v = drawn[a][(t, p)]
                            st["lens"].add(len(v))
                            for mt, cnt in ld.evidence_counts(S, a, int(live[t])):
                                st["flavour"] += sum(1 for o in cnt if ld.lit.damerau_levenshtein(o, v, False)
                                                     != ld.lit.damerau_levenshtein(o, v, True))
                    break
            assert ok, (t, p, w[t, p], cs, subsets)
            st["slots"] += 1
            st["items"].add(int(live[t]))
    return w, chosen, vals, st


@pytest.mark.parametrize("dist_mode", [_lib.DIST_DL, _lib.DIST_OSA], ids=["unrestricted", "osa"])
def test_weights_equal_the_restatement(oracle, wprog, memo, dist_mode):
    """every (row, particle) of the weights program, P = 2 (MH), 2, 5, 64, both flavours; items without a correction
    keep the choice and the values of the uncorrected sweep; two runs agree bit for bit; a launch cut into arena slices
    gives the same weights"""
    S = wprog
    restricted = dist_mode == _lib.DIST_OSA
    eng = Engine(S["lw"], S["obs"], dist_mode=dist_mode)
    try:
        args = _setup(S, eng)
        assert eng.latent_dummy_served("Item") == ["name", "tag"]
        assert (args[4] >= 0).sum() == 3  # the drawn strings rows 7 and 8 hold (name twice, tag once)
        total = dict(slots=0, exact=0, p0=0, lens=set(), flavour=0, worst=0.0, unchanged=0, items=set())
        for sweep_idx, (P, mh) in enumerate(PARTICLES):
            w, chosen, vals, st = _check_weights(oracle, S, eng, args, P, mh, sweep_idx, restricted, memo)
            for k in ("slots", "exact", "p0", "flavour"):
                total[k] += st[k]
            total["lens"] |= st["lens"]
            total["items"] |= st["items"]
            total["worst"] = max(total["worst"], st["worst"])
            # determinism
            chosen2, vals2, w2 = _sweep(eng, S, args, P, mh, sweep_idx, True)
            assert np.array_equal(w, w2) and np.array_equal(chosen, chosen2) and np.array_equal(vals, vals2)
            # unchanged where nothing applies
            chosen0, vals0, _ = _sweep(eng, S, args, P, mh, sweep_idx, False)
            quiet = np.flatnonzero((w == 0.0).all(axis=1))
            assert np.array_equal(chosen[quiet], chosen0[quiet]) and np.array_equal(vals[quiet], vals0[quiet]), (P, mh)
            total["unchanged"] += len(quiet)
            if P == 64:  # the same launch in slices of four slots
                lane_cells = (40 + 2) * (ld.W_LEN + 2)
                os.environ["PCLEAN_LATENT_DUMMY_ARENA"] = str(4 * 64 * lane_cells)
                try:
                    chosen3, vals3, w3 = _sweep(eng, S, args, P, mh, sweep_idx, True)
                finally:
                    del os.environ["PCLEAN_LATENT_DUMMY_ARENA"]
                assert np.count_nonzero(w) > 8  # (more than two slices)
                assert np.array_equal(w, w3) and np.array_equal(chosen, chosen3) and np.array_equal(vals, vals3)
        print(f"\n[{'osa' if restricted else 'unrestricted'}] {total['slots']} fresh slots ({total['exact']} through the chosen "
              f"particle's draws), {total['p0']} retained slots, drawn lengths {sorted(total['lens'])}, {total['flavour']} "
              f"(observed, drawn) pairs on which the flavours differ, worst error {total['worst']:.3f} of its tolerance, "
              f"{total['unchanged']} rows without a correction")
        # (the program's atoms explain no observed name, so nearly every fresh particle of rows 0 .. 8 takes the name's
        # dummy: 9 rows x (1 + 1 + 4 + 63) fresh particles = 621 slots; every shape of row must be among them)
        assert total["slots"] >= 500 and total["exact"] >= 10 and total["p0"] == 3 * len(PARTICLES)
        assert total["items"] >= {0, 1} | set(ld.W_DISTINCT) | set(ld.W_STRING_ITEMS), sorted(total["items"])
        assert total["lens"] == set(range(1, ld.W_LEN + 1))
        assert total["flavour"] >= 1, "no fresh slot told the flavours apart: extend latent_dummy_program._observed_words"
        assert total["unchanged"] >= len(PARTICLES) * len(ld.W_EXPLAINED)
    finally:
        eng.close()


def test_committed_rows_hold_the_strings_that_were_weighed(oracle, monkeypatch):
    """latent_sweep(..., dummy_correction=True): every row whose served choice took the dummy holds the string of its
    recorded key, by the oracle's sampler"""
    from pclean_amd import inference as inf
    S = ld.weights_program()
    lw, tr = S["lw"], S["trace"]
    seen = {}
    real = inf.commit_latent

    def spy(lw_, tr_, cname, live, chosen, vals, *a):
        seen.update(live=np.array(live), chosen=np.array(chosen), vals=np.array(vals),
                    opt={x: lw_.option_values[("Item", x)].copy() for x in ("name", "tag")},
                    dummy={x: lw_.latent_dom[("Item", x)].get(lw_.model.classes["Item"].attr(x).dist.dummy_value())
                           for x in ("name", "tag")})
        return real(lw_, tr_, cname, live, chosen, vals, *a)

    monkeypatch.setattr(inf, "commit_latent", spy)
    eng = Engine(lw, S["obs"], dist_mode=1)
    try:
        eng.upload_trace(tr)
        pl = lw.latent_plans["Item"]
        block_id, roots = pl["block_id"], {a: pl["roots"][pl["root_attr"].index(a)] for a in ("name", "tag")}
        before = {a: tr.tables["Item"].cols[lw.colidx["Item"][a], :tr.tables["Item"].n].copy() for a in ("name", "tag")}
        inf.latent_sweep(eng, tr, "Item", InferenceConfig(1, 5), SEED, 3, dummy_correction=True)
        t = tr.tables["Item"]
        n_checked = 0
        for k, row in enumerate(seen["live"]):
            p = int(seen["chosen"][k])
            for a in ("name", "tag"):
                dom = lw.latent_dom[("Item", a)]
                now = dom.string(int(t.cols[lw.colidx["Item"][a], row]))
                if p > 0 and seen["opt"][a][seen["vals"][k, roots[a]]] == seen["dummy"][a]:
                    assert tr.row_origin[("Item", int(row))] == (int(row), p, 3, block_id)
                    want = ld.drawn_string(oracle, lw, a, SEED, block_id, roots[a], p, 3, int(row))
                    assert now == want, (row, a, now, want)
                    n_checked += 1
                elif p == 0:
                    assert int(t.cols[lw.colidx["Item"][a], row]) == int(before[a][row])
                assert now != lw.model.classes["Item"].attr(a).dist.dummy_value()  # no placeholder left
        assert n_checked >= 5
    finally:
        eng.close()


@pytest.mark.parametrize("name,mh,state", ld.DIST_CASES, ids=[c[0] for c in ld.DIST_CASES])
def test_draws_follow_the_closed_forms(oracle, name, mh, state):
    """DIST_SWEEPS sweeps from a frozen state over DIST_ROWS identical rows against latent_dummy_program.kernel; the
    uncorrected sweep (the flag off) fails the same test: tests/test_latent_dummy_cpu.py"""
    S = ld.dist_program(state)
    lw = S["lw"]
    exact = ld.kernel(ld.DIST_ATOMS, ld.DIST_LEN, ld.dist_evidence(), state, mh)
    eng = Engine(lw, S["obs"], dist_mode=1)
    try:
        args = _setup(S, eng)
        live = args[0]
        assert ((args[4] >= 0).all()) == (state not in ld.DIST_ATOMS)
        pl = lw.latent_plans["Item"]
        root = pl["roots"][0]
        opt = lw.option_values[("Item", "name")]
        dom = lw.latent_dom[("Item", "name")]
        dummy = dom.get(lw.model.classes["Item"].attr("name").dist.dummy_value())
        counts = {}
        for s in range(ld.DIST_SWEEPS):
            chosen, vals, w = _sweep(eng, S, args, 2, mh, s, True)
            fresh = np.flatnonzero(chosen > 0)
            took = fresh[opt[vals[fresh, root]] == dummy]
            strings = dict(zip(took.tolist(), ld.drawn_strings(oracle, lw, "name", SEED, pl["block_id"], root,
                                                               chosen[took], s, live[took])))
            for t in range(len(live)):
                if chosen[t] == 0:
                    got = state
                elif t in strings:
                    got = strings[t]
                else:
                    got = dom.string(int(opt[vals[t, root]]))
                counts[got] = counts.get(got, 0) + 1
        res = pe.gof([(0, exact, counts)])
        print(f"\n[{name}] {pe.describe(res)}")
        assert res["n"] == ld.DIST_ROWS * ld.DIST_SWEEPS
        assert res["p"] > pe.ALPHA, pe.describe(res)
    finally:
        eng.close()


@pytest.mark.parametrize("program", ["rents", "flights"])
def test_unserved_classes_are_swept_as_before(program):
    """a keyed StringPrior (rents' County) and TimePrior choices (flights' Flight): nothing is served, every weight is 0 and
    the sweep returns what it returns with the flag off"""
    import helpers
    S = helpers.rents_setup(n_rows=300) if program == "rents" else helpers.flights_setup()
    cname = "County" if program == "rents" else "Flight"
    lw, tr = S["lw"], S["trace"]
    eng = Engine(lw, S["obs"], dist_mode=1)
    try:
        eng.upload_trace(tr)
        assert eng.latent_dummy_served(cname) == []
        live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, cname)
        cfg = InferenceConfig(1, 4)
        excl = latent_current_choices(lw, tr, cname, live, cfg, eng.latent_dummy_served(cname))
        assert np.array_equal(excl, latent_current_choices(lw, tr, cname, live, cfg))
        off = eng.sweep_latent(tr, cname, cfg, SEED, 1, live, ev_off, ev_rows, ev_ctx, excl)
        off = (off[0].copy(), off[1].copy())
        on = eng.sweep_latent(tr, cname, cfg, SEED, 1, live, ev_off, ev_rows, ev_ctx, excl, dummy_correction=True)
        w = eng.latent_weights()
        assert w.shape == (len(live), 4) and not w.any()
        assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    finally:
        eng.close()
