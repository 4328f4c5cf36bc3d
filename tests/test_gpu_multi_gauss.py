"""GPU runs of the programs with three and four Gaussian observations in one block, and of the programs whose own choices
fill all 16 combinations (tests/multi_gauss_program.py).  Every device loop over `more[0 .. n_more)` runs here with
n_more = 2 and 3.  No oracle knows more than one Gaussian per block, so:
  (a) the Gaussian part of candidate scores, new-row options and evidence sets — the program's score minus its all-missing
      twin's — against the float64 restatement two_gauss_program.gauss_part / term_value (its precision and its power are
      asserted on the CPU, tests/test_multi_gauss.py);
  (b) declaration order; (c) a subset of the terms present is the smaller program, bit for bit — which chains the four-term
  path to the two-term path and, through tests/test_gpu_two_gauss.py and test_gpu_addnoise.py, to the oracle;
  (d) prior proposals; (e) the own choices drawn for the chosen particle; (f) windows; (g) the ABI's refusals; (h) end to end.
Each test runs at 600 rows (the last one at 1500)."""
import ctypes as C

import numpy as np
import pytest

import multi_gauss_program as mg
import two_gauss_program as tg
from pclean_amd.engine import Engine, InferenceConfig, make_gauss
from pclean_amd.inference import build_evidence, initialize_trace, run_inference
from pclean_amd.trace import Trace
from test_gpu_two_gauss import _one_latent_and_one_observed_sweep

pytestmark = pytest.mark.gpu

SCORE_CASES = {fn.__name__: fn for fn in (mg.three_model, mg.four_mixed_model, mg.sixteen_8x2, mg.sixteen_4x4,
                                          mg.sixteen_4x4_linear)}
_cache = {}


def _pair(name, spread=mg.SCORE_SPREAD):
    """(program, its all-missing twin), lowered once per module.  The only state a test below changes is the traces' own
    choices (locals, pending_locals); every hand-out sets them anew, so no test sees what another one left behind"""
    if (name, spread) not in _cache:
        fn = getattr(mg, name)
        S, S0 = mg.setup(fn), mg.setup(fn, base=True)
        for s in (S, S0):
            mg.seed_means(s, spread)
        assert np.isnan(S0["lw"].xnum).all() and np.array_equal(S["obs"], S0["obs"])
        assert len(S0["lw"].gauss_more[(0, 0)]) == len(S["lw"].gauss_more[(0, 0)]) >= 2
        _cache[(name, spread)] = (S, S0, S["trace"].cur.copy())
    S, S0, cur = _cache[(name, spread)]
    for s in (S, S0):
        mg.fix_locals(s)
        s["trace"].pending_locals = {}
        assert np.array_equal(s["trace"].cur, cur)
    return S, S0


def _engines(S, S0):
    e, e0 = Engine(S["lw"], S["obs"], dist_mode=1), Engine(S0["lw"], S0["obs"], dist_mode=1)
    e.upload_trace(S["trace"])
    e0.upload_trace(S0["trace"])
    return e, e0


def _check_scores(case, what, S, rows, a, b, values_of, at_least):
    """a - b against gauss_part for every finite (row, candidate); returns the worst error / tolerance"""
    assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.isfinite(a).any()
    n_checked, worst, most = 0, 0.0, 0
    for r, i in enumerate(rows):
        for k in np.flatnonzero(np.isfinite(a[r])):
            want, n_comb = tg.gauss_part(S, int(i), values_of(int(i), int(k)))
            tol = mg.score_tolerance(n_comb, want, a[r, k])
            err = abs((a[r, k] - b[r, k]) - want)
            worst, most = max(worst, err / tol), max(most, n_comb)
            assert abs(b[r, k]) <= mg.SCORE_REST  # (the bound on the rest of a score that the CPU power precondition assumes)
            assert err <= tol, (case, what, int(i), int(k), a[r, k] - b[r, k], want, tol)
            n_checked += 1
    print(f"{case}, {what}: {n_checked} scores, up to {most} combinations, worst error / tolerance {worst:.3g}")
    assert n_checked >= at_least
    return most


@pytest.mark.parametrize("case", sorted(SCORE_CASES))
def test_gaussian_part_of_existing_candidates(case):
    S, S0 = _pair(case)
    e, e0 = _engines(S, S0)
    try:
        tr = S["trace"]
        t = tr.tables["County"]
        rows, pat = mg.rows_visited(S, 4)
        excl = tr.cur[0, rows]
        _, a, _ = e.hip.score_node(0, 0, rows, excl=excl, n_cand=t.n + 1, want_scores=True)
        _, b, _ = e0.hip.score_node(0, 0, rows, excl=excl, n_cand=t.n + 1, want_scores=True)
    finally:
        e.close()
        e0.close()
    a, b = a[:, :t.n], b[:, :t.n]
    # a row's current referent is a candidate unless the row is its only reference (the row's own reference is removed
    # first): many of the pairs of the CPU power precondition are visited here, all of them by the new-row test
    assert np.isfinite(a[np.arange(len(rows)), tr.cur[0, rows]]).sum() >= len(rows) // 4
    most = _check_scores(case, "existing candidates", S, rows, a, b, lambda i, k: mg.referent_values(S, k), 30)
    own = mg.own_observed(S)
    assert set(pat[rows]) == set(range(1 << len(S["lw"].gauss_specs))) and own[rows].any() and (~own[rows]).any()
    if case.startswith("sixteen"):
        assert most == 16


@pytest.mark.parametrize("case", sorted(SCORE_CASES))
def test_gaussian_part_of_the_new_row_branch(case):
    S, S0 = _pair(case)
    lw = S["lw"]
    leaf = next(nid for nid, info in enumerate(lw.blocks[0]["node_info"]) if info["kind"] == "leaf" and info["path"] == "state")
    assert len(lw.gauss_more[(0, leaf)]) == len(lw.gauss_specs) - 1
    opts = lw.option_values[("County", "state")]
    rows, _ = mg.rows_visited(S, 4)
    e, e0 = _engines(S, S0)
    try:
        _, a, _ = e.hip.score_node(0, leaf, rows, n_cand=len(opts), want_scores=True)
        _, b, _ = e0.hip.score_node(0, leaf, rows, n_cand=len(opts), want_scores=True)
    finally:
        e.close()
        e0.close()
    ck = S["obs"][lw.obs_index["county.countykey"]]
    # the pairs of the CPU power precondition — a visited row at its current referent's index values — are all visited
    for r, i in enumerate(rows):
        iv = mg.referent_values(S, int(S["trace"].cur[0, i]))
        assert iv["countykey"] == ck[i] and np.isfinite(a[r, list(opts).index(iv["state"])])
    most = _check_scores(case, "new-row leaf", S, rows, a, b, lambda i, k: {"state": int(opts[k]), "countykey": int(ck[i])},
                         len(rows))
    if case.startswith("sixteen"):
        assert most == 16


@pytest.mark.parametrize("case", sorted(SCORE_CASES))
def test_gaussian_part_of_evidence_sets(case):
    S, S0 = _pair(case)
    lw, tr = S["lw"], S["trace"]
    k = len(lw.gauss_specs)
    pl, pl0 = lw.latent_plans["County"], S0["lw"].latent_plans["County"]
    node = next(nid for nid, info in enumerate(pl["node_info"]) if info["kind"] == "leaf" and info["path"] == "state")
    assert pl0["node_info"][node]["path"] == "state" and len(lw.gauss_more[(pl["block_id"], node)]) == k - 1
    live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "County")
    live0, ev_off0, ev_rows0, ev_ctx0 = build_evidence(S0["lw"], S0["trace"], "County")
    assert np.array_equal(live, live0) and np.array_equal(ev_rows, ev_rows0) and np.array_equal(ev_ctx, ev_ctx0)
    n_lat = 120
    assert len(live) >= n_lat and (np.diff(ev_off[:n_lat + 1]) > 0).all()
    n_ev = int(ev_off[n_lat])
    opts = lw.option_values[("County", "state")]
    e, e0 = _engines(S, S0)
    try:
        e.hip.set_active_rows(0, -1)
        e0.hip.set_active_rows(0, -1)
        _, a, _ = e.hip.score_node_ev(pl["block_id"], node, live[:n_lat], ev_off[:n_lat + 1], ev_rows[:n_ev],
                                      ev_ctx=ev_ctx[:n_ev], n_cand=len(opts), want_scores=True)
        _, b, _ = e0.hip.score_node_ev(pl0["block_id"], node, live[:n_lat], ev_off[:n_lat + 1], ev_rows[:n_ev],
                                       ev_ctx=ev_ctx[:n_ev], n_cand=len(opts), want_scores=True)
    finally:
        e.close()
        e0.close()
    assert np.array_equal(np.isfinite(a), np.isfinite(b))
    ck = S["obs"][lw.obs_index["county.countykey"]]
    n_checked, worst = 0, 0.0
    n_present = np.zeros(k + 1, dtype=int)  # evidence rows by their number of present terms
    units = set()
    for j in range(n_lat):
        for c in np.flatnonzero(np.isfinite(a[j])):
            want, mag = 0.0, 0.0
            for pos in range(ev_off[j], ev_off[j + 1]):
                i = int(ev_rows[pos])
                terms = [tg.term_value(S, g, i, {"state": int(opts[c]), "countykey": int(ck[i])}, [int(v) for v in ev_ctx[pos]])
                         for g in range(k)]
                n_present[sum(x is not None for x in terms)] += 1
                units.add(int(ev_ctx[pos][-1]))
                for x in terms:
                    if x is not None:
                        want += x
                        mag += abs(x)
            tol = 1e-12 * (1.0 + mag)
            err = abs((a[j, c] - b[j, c]) - want)
            worst = max(worst, err / tol)
            assert err <= tol, (case, j, int(c), a[j, c] - b[j, c], want)
            n_checked += 1
    print(f"{case}, evidence sets: {n_checked} scores, evidence rows by present terms {n_present.tolist()}, "
          f"worst error / tolerance {worst:.3g}")
    assert n_checked >= n_lat and (n_present >= 5).all()
    if case.startswith("sixteen_4x4"):  # the evidence rows' Transformations: all four options
        assert units == {0, 1, 2, 3}


def test_declaration_order_does_not_move_the_root_scores():
    """the whole root, NEW column included: four terms against the same four declared in another order"""
    out = []
    rows = np.arange(600, dtype=np.int32)
    for fn in (mg.four_model, mg.four_model_permuted):
        S = mg.setup(fn)
        mg.seed_means(S, mg.SCORE_SPREAD)
        eng = Engine(S["lw"], S["obs"], dist_mode=1)
        try:
            eng.upload_trace(S["trace"])
            t = S["trace"].tables["County"]
            lse, sc, _ = eng.hip.score_node(0, 0, rows, excl=S["trace"].cur[0], n_cand=t.n + 1, want_scores=True)
            out.append((lse, sc, S))
        finally:
            eng.close()
    (la, a, A), (lb, b, B) = out
    # the same tables behind another order of the terms
    assert [sp["gauss_attr"] for sp in B["lw"].gauss_specs] == ["util", "rent", "fee", "deposit"]
    assert np.array_equal(A["trace"].mean_params[0].value, B["trace"].mean_params[1].value)
    assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.isfinite(a[:, -1]).any()
    fin = np.isfinite(a)
    assert (np.abs(a[fin] - b[fin]) <= 1e-12 * np.maximum(1.0, np.abs(a[fin]))).all()
    assert (np.abs(la - lb) <= 1e-12 * np.maximum(1.0, np.abs(la))).all()


def _without(S, cols):
    dirty, clean = dict(S["dirty"]), dict(S["clean"])
    for c in cols:
        del dirty[c], clean[c]
    return dirty, clean


@pytest.mark.parametrize("smaller", ["two_model", "three_model"])
@pytest.mark.parametrize("particles,mh,dd", [(2, True, True), (20, False, True), (6, False, False)])
def test_a_subset_present_is_the_smaller_program_bit_for_bit(particles, mh, dd, smaller):
    """per combination the terms are added in declaration order, a missing one skipped — four terms with the
    last ones missing everywhere perform the additions of the program that never declared them"""
    gone = {"two_model": ["Fee", "Util"], "three_model": ["Util"]}[smaller]
    A = mg.setup(mg.four_model, missing=gone)
    if smaller == "two_model":
        B = tg.setup(tg.two_model, data=_without(A, gone))
    else:
        B = mg.setup(mg.three_model, given=_without(A, gone))
    kb = len(B["lw"].gauss_specs)
    assert np.array_equal(A["obs"], B["obs"]) and np.isnan(A["lw"].xnum[kb:]).all()
    assert np.array_equal(A["lw"].xnum[:kb], B["lw"].xnum, equal_nan=True) and (~np.isnan(B["lw"].xnum)).sum(axis=1).min() > 200
    assert len(A["lw"].gauss_more[(0, 0)]) == 3 and len(B["lw"].gauss_more[(0, 0)]) == kb - 1
    assert [sp["sigma"] for sp in A["lw"].gauss_specs[:kb]] == [sp["sigma"] for sp in B["lw"].gauss_specs]
    mg.seed_means(A, mg.SCORE_SPREAD)
    for g in range(kb):
        B["trace"].mean_params[g].value = A["trace"].mean_params[g].value.copy()
    out = []
    for S in (A, B):
        mg.fix_locals(S)
        out.append(_one_latent_and_one_observed_sweep(S, particles, mh, dd))
    assert np.array_equal(A["trace"].locals[0], B["trace"].locals[0])
    assert sorted(out[0]) == sorted(out[1])
    for key in out[0]:
        assert np.array_equal(out[0][key], out[1][key]), key
    assert (out[0]["logml"] != 0).any()


@pytest.mark.parametrize("case", ["four_mixed_model", "sixteen_4x4", "sixteen_4x4_linear"])
@pytest.mark.parametrize("keep", [True, False])
def test_prior_proposals_score_every_term_at_the_particles_own_choices(case, keep):
    """use_dd_proposals = false, one particle: the retained particle keeps the referent and (keep) the row's own choices, or
    (not keep) draws them; log weight of the program minus that of its all-missing twin = sum of the present terms"""
    S, S0 = _pair(case)
    lw = S["lw"]
    k = len(lw.gauss_specs)
    cfg = InferenceConfig(1, 1, use_mh_instead_of_pg=False, rejuv_frequency=500, use_dd_proposals=False)
    out = []
    for s in (S, S0):
        tr = s["trace"]
        if keep:
            mg.fix_locals(s)
        else:
            tr.locals[0][:] = -1
        eng = Engine(s["lw"], s["obs"], dist_mode=1)
        try:
            eng.upload_trace(tr)
            choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 5, 0)
            out.append((choice.copy(), chosen.copy(), logml.copy(), tr.pending_locals[0].copy()))
        finally:
            eng.close()
            mg.fix_locals(s)
    (choice, chosen, la, loc), (choice0, chosen0, lb, loc0) = out
    cur = S["trace"].cur
    assert np.array_equal(choice, cur) and np.array_equal(choice0, cur) and (chosen == 0).all() and (chosen0 == 0).all()
    assert np.array_equal(loc, loc0)  # the twin's particle draws from the same streams
    spec = lw.gauss_specs[0]
    for l, (nl, oc) in enumerate(zip(spec["local_n"], spec["local_obs"])):
        o = S["obs"][oc] if oc >= 0 else np.full(600, -1)
        assert ((loc[:, l] >= 0) & (loc[:, l] < nl)).all() and (loc[o >= 0, l] == o[o >= 0]).all()
        if not keep:
            # drawn: every option occurs, and not as the pattern fix_locals writes — a uniform draw differs from any fixed
            # value with probability 1 - 1/nl >= 1/2; 0.3 lies 5 standard deviations below that for the fewest rows here
            # (195 with the room type unobserved)
            assert set(loc[o < 0, l]) == set(range(nl))
            assert (o < 0).sum() >= 195 and np.mean(loc[o < 0, l] != S["trace"].locals[0][o < 0, l]) >= 0.3
    if keep:
        assert np.array_equal(loc, S["trace"].locals[0])
    worst, n_all, n_terms = 0.0, 0, 0
    for i in range(600):
        terms = [tg.term_value(S, g, i, mg.referent_values(S, int(cur[0, i])), [int(v) for v in loc[i]]) for g in range(k)]
        terms = [x for x in terms if x is not None]
        tol = 1e-12 * (1.0 + sum(abs(x) for x in terms))
        err = abs((la[i] - lb[i]) - sum(terms))
        worst = max(worst, err / tol)
        assert err <= tol, (case, keep, i, la[i] - lb[i], sum(terms), tol)
        n_all += len(terms) == k
        n_terms += len(terms)
    print(f"{case}, prior proposals, own choices {'kept' if keep else 'drawn'}: 600 rows, {n_terms} terms, {n_all} rows with "
          f"every term, worst error / tolerance {worst:.3g}")
    assert n_all >= 12 and n_terms >= 600


@pytest.mark.parametrize("case", ["four_mixed_model", "sixteen_8x2"])
def test_own_choices_of_the_chosen_particle(case):
    """a data-driven sweep; for every row whose chosen referent exists the combination scores are restated at that referent:
    the drawn combination has a non-zero fixed-point weight, and is the best one wherever every other weighs exactly 0"""
    S, _ = _pair(case, mg.DECIDED_SPREAD)
    lw, tr = S["lw"], S["trace"]
    cfg = InferenceConfig(1, 4, use_mh_instead_of_pg=False, rejuv_frequency=500, use_dd_proposals=True)
    eng = Engine(lw, S["obs"], dist_mode=1)
    try:
        eng.upload_trace(tr)
        choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 5, 0)
        loc = tr.pending_locals[0].copy()
    finally:
        eng.close()
    own = mg.own_observed(S)
    n_rows = n_decided = n_unobserved = 0
    for i in np.flatnonzero(choice[0] >= 0):
        combos, sc, best, dec = mg.decided(S, int(i), mg.referent_values(S, int(choice[0, i])))
        drawn = tuple(int(v) for v in loc[i][:len(combos[0])])
        assert drawn in combos, (case, int(i), drawn)
        assert sc[combos.index(drawn)] >= sc[best] - mg.FIX_CUTOFF, (case, int(i), drawn, sc[combos.index(drawn)], sc[best])
        if dec:
            assert drawn == combos[best], (case, int(i), drawn, combos[best])
            n_decided += 1
            n_unobserved += not own[i]
        n_rows += 1
    print(f"{case}: {n_rows} rows with an existing referent, {n_decided} decided, {n_unobserved} of them with the first own "
          f"choice unobserved")
    assert n_decided >= 100 and n_unobserved >= 30


@pytest.mark.parametrize("dd", [True, False])
def test_windows_equal_one_sweep(dd):
    """24 windows of 25 rows against one sweep of the 600: every window resolves the three further terms of the root and of
    the open leaf anew; draws are keyed by the row and nothing is committed in between"""
    S, _ = _pair("four_mixed_model")
    lw, tr, obs = S["lw"], S["trace"], S["obs"]
    n, W = obs.shape[1], 25
    cfg = InferenceConfig(1, 3, use_mh_instead_of_pg=False, rejuv_frequency=500, use_dd_proposals=dd)
    eng = Engine(lw, obs, dist_mode=1)
    try:
        eng.upload_trace(tr)

        def sweep(lo, hi):
            choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 5, 0, lo=lo, hi=hi)
            rows, vals = new_rows.get(0, (np.zeros(0, np.int32), np.zeros((0, len(lw.blocks[0]["nodes"])), np.int32)))
            order = np.argsort(rows, kind="stable")
            return [choice.copy(), chosen.copy(), logml.copy(), tr.pending_locals[0].copy(), rows[order] + lo, vals[order]]

        whole = sweep(0, n)
        parts = [sweep(lo, min(lo + W, n)) for lo in range(0, n, W)]
    finally:
        eng.close()
        tr.pending_locals = {}
    assert len(parts) == 24
    names = ["choice", "chosen_particle", "logml", "pending_locals", "new rows", "new-row values"]
    for k, name in enumerate(names):
        got = np.concatenate([p[k] for p in parts], axis=1 if name == "choice" else 0)
        assert got.shape == whole[k].shape and np.array_equal(got, whole[k]), name
    assert (whole[2] != 0).any() and (whole[3][:, 0] >= 0).all()


def _refused(eng, fn, block, node, g, status):
    rc = fn(eng.hip.h, C.c_int32(block), C.c_int32(node), C.byref(g))
    msg = eng.hip.lib.pclean_last_error(eng.hip.h).decode()
    assert rc == status, (rc, status, msg)
    assert msg
    return msg


def test_the_abi_refuses_what_the_kernels_cannot_hold_and_keeps_the_plan():
    ERR_ARG, ERR_CAPACITY = -1, -5  # PCLEAN_ERR_ARG, PCLEAN_ERR_CAPACITY (include/pclean_hip.h)
    S, _ = _pair("four_mixed_model")
    lw, tr = S["lw"], S["trace"]
    cfg = InferenceConfig(1, 3, use_mh_instead_of_pg=False, rejuv_frequency=500, use_dd_proposals=True)
    eng = Engine(lw, S["obs"], dist_mode=1)
    try:
        eng.upload_trace(tr)

        def sweep():
            choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 5, 0)
            rows, vals = new_rows.get(0, (np.zeros(0, np.int32), np.zeros((0, 0), np.int32)))
            return [choice.copy(), chosen.copy(), logml.copy(), tr.pending_locals[0].copy(), rows.copy(), vals.copy()]

        before = sweep()
        add, set_ = eng.hip.lib.pclean_add_node_gauss, eng.hip.lib.pclean_set_node_gauss
        more = lw.gauss_more[(0, 0)]
        assert len(more) == 3
        bare = next(nid for nid in range(len(lw.blocks[0]["nodes"])) if (0, nid) not in lw.gauss)
        msgs = [_refused(eng, add, 0, bare, make_gauss(more[0]), ERR_ARG)]  # no first term
        for field, value in (("local_n", (0, 4)), ("local_n", (1, 3)), ("local_obs_col", (0, -1)), ("local_obs_col", (1, 0)),
                             ("n_locals", 1), ("fixed_locals", 1)):  # own choices that are not the first term's
            g = make_gauss(more[0])
            if isinstance(value, tuple):
                assert getattr(g, field)[value[0]] != value[1]
                getattr(g, field)[value[0]] = value[1]
            else:
                assert getattr(g, field) != value
                setattr(g, field, value)
            msgs.append(_refused(eng, add, 0, 0, g, ERR_ARG))
        msgs.append(_refused(eng, add, 0, 0, make_gauss(more[2]), ERR_CAPACITY))  # a fifth term
        for n0, n1 in ((17, 1), (9, 2)):
            g = make_gauss(lw.gauss[(0, 0)])
            g.n_locals, g.local_n[0], g.local_n[1] = (1 if n1 == 1 else 2), n0, n1
            msgs.append(_refused(eng, set_, 0, 0, g, ERR_CAPACITY))
        assert "no Gaussian term yet" in msgs[0] and "share its own choices" in msgs[1] and "more than 4" in msgs[7]
        assert "16 local combinations" in msgs[8] and "16 local combinations" in msgs[9]
        after = sweep()
    finally:
        eng.close()
        tr.pending_locals = {}
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert (before[2] != 0).any()


def _end_to_end(seed):
    S = mg.setup(mg.four_mixed_model, 1500)
    lw, obs = S["lw"], S["obs"]
    eng = Engine(lw, obs, dist_mode=1)
    try:
        cfg = InferenceConfig(2, 2, use_mh_instead_of_pg=True, rejuv_frequency=500)
        tr = Trace(lw, obs.shape[1], seed)
        initialize_trace(eng, tr, cfg, seed, max_batch=512)
        run_inference(eng, tr, cfg, seed)
        tr.check_consistency()
        return S, tr
    finally:
        eng.close()


def test_four_terms_end_to_end():
    S, tr = _end_to_end(7)
    _, tr2 = _end_to_end(7)
    assert np.array_equal(tr.cur, tr2.cur) and np.array_equal(tr.locals[0], tr2.locals[0])
    assert len(tr.mean_params) == 4 and (tr.locals[0] >= 0).all()
    for g in range(4):
        assert np.array_equal(tr.mean_params[g].value, tr2.mean_params[g].value)
    assert all(not np.array_equal(tr.mean_params[a].value[:50], tr.mean_params[b].value[:50]) for a in range(4) for b in range(a))
    # every parameter's Gibbs draw given the final assignment: every occupied cell — those with 20 or more rows among them, few
    # at 1500 rows — lies within 6 posterior standard deviations of its closed-form conjugate mean
    tr.resample_parameters("Obs")
    n_big = []
    for g, spec in enumerate(S["lw"].gauss_specs):
        _, sigma, prior_mean, _ = mg.TERMS[spec["gauss_attr"]]
        rows, idx, xs = tr.gaussian_index(g)
        n = np.bincount(idx, minlength=len(tr.mean_params[g].value))
        sm = np.bincount(idx, weights=xs, minlength=len(tr.mean_params[g].value))
        cells = np.flatnonzero(n >= 1)
        n_big.append(int((n >= 20).sum()))
        assert len(cells) >= 50
        var = 1.0 / (1.0 / mg.PRIOR_STD ** 2 + n[cells] / sigma ** 2)
        post = var * (prior_mean / mg.PRIOR_STD ** 2 + sm[cells] / sigma ** 2)
        assert (np.abs(tr.mean_params[g].value[cells] - post) <= 6 * np.sqrt(var)).all(), spec["gauss_attr"]
    print(f"cells with 20 or more rows per term: {n_big}")
