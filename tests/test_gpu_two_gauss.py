"""GPU runs of the programs with two Gaussian observations in one block (tests/two_gauss_program.py).  The C++ oracle
knows one Gaussian per block, so: (1) with one term present the sweeps must equal the one-term programs' — which
tests/test_gpu_addnoise.py holds to the oracle — bit for bit; (2)-(4) the Gaussian part of candidate scores, new-row
options and evidence sets against the float64 restatement of two_gauss_program.gauss_part; (5) draws that need BOTH
numbers to find the referent; (6) inference end to end."""
import numpy as np
import pytest

import addnoise_program as ap
import posterior_exact
import two_gauss_program as tg
from pclean_amd.analysis import evaluate_accuracy
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import build_evidence, commit_latent, initialize_trace, latent_current_choices, run_inference
from pclean_amd.trace import Trace

pytestmark = pytest.mark.gpu


def _fix_locals(S):
    """own choices of every row: the observed br where there is one, a fixed pattern elsewhere; unit 0 / 1 alternating"""
    lw, tr = S["lw"], S["trace"]
    if not lw.locals:
        return
    n = tr.cur.shape[1]
    br = S["obs"][lw.obs_index["br"]]
    tr.locals[0][:, 0] = np.where(br >= 0, br, np.arange(n) % 5)
    if len(lw.locals[0]) > 1:
        tr.locals[0][:, 1] = np.arange(n) % 2


def _one_latent_and_one_observed_sweep(S, particles, mh, dd):
    lw, tr, obs = S["lw"], S["trace"], S["obs"]
    tr.rng = np.random.default_rng(77)  # (the two programs' host generators stand at different draws after construction)
    eng = Engine(lw, obs, dist_mode=1)
    try:
        cfg = InferenceConfig(1, particles, use_mh_instead_of_pg=mh, rejuv_frequency=500, use_dd_proposals=dd)
        pl = lw.latent_plans["County"]
        live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "County")
        excl = (np.full((len(pl["roots"]), len(live)), -1, dtype=np.int32) if dd
                else latent_current_choices(lw, tr, "County", live, cfg))
        eng.upload_trace(tr)
        eng.hip.set_active_rows(0, -1)
        lat = eng.hip.sweep_latent(cfg.as_c(), 5, 0, pl["block_id"], pl["roots"], live, ev_off, ev_rows, ev_ctx, excl,
                                   len(pl["nodes"]))
        commit_latent(lw, tr, "County", live, lat[0], lat[1])
        tr.check_consistency()
        eng.upload_trace(tr)
        choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 5, 0)
        out = dict(lat_chosen=lat[0].copy(), lat_vals=lat[1].copy(), choice=choice.copy(), chosen=chosen.copy(),
                   logml=logml.copy())
        for b in sorted(new_rows):
            out[f"new_rows_{b}"], out[f"new_vals_{b}"] = new_rows[b][0].copy(), new_rows[b][1].copy()
        if lw.locals:
            out["pending_locals"] = tr.pending_locals[0].copy()
        return out
    finally:
        eng.close()


@pytest.mark.parametrize("pair", ["own_br", "candidate_only"])
@pytest.mark.parametrize("particles,mh,dd", [(2, True, True), (20, False, True), (6, False, False)])
def test_one_term_present_is_the_one_term_path_bit_for_bit(particles, mh, dd, pair):
    two_fn, one_fn = {"own_br": (tg.two_model, ap.addnoise_model),
                      "candidate_only": (tg.two_candidate_model, ap.candidate_mean_model)}[pair]
    A = tg.setup(tg.all_missing(two_fn), 3000)
    B = ap.setup(one_fn, 3000)
    assert np.array_equal(A["obs"], B["obs"]) and np.isnan(A["lw"].xnum[1]).all()
    assert np.array_equal(A["lw"].xnum[0], B["lw"].xnum[0], equal_nan=True)
    assert len(A["lw"].gauss_more[(0, 0)]) == 1 and not getattr(B["lw"], "gauss_more", {})
    tg.seed_means(A)
    B["trace"].mean_param.value = A["trace"].mean_params[0].value.copy()
    out = []
    for S in (A, B):
        _fix_locals(S)
        out.append(_one_latent_and_one_observed_sweep(S, particles, mh, dd))
    assert sorted(out[0]) == sorted(out[1])
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert (out[0]["logml"] != 0).any()


def _row_kinds(S):
    """rows of every kind the Gaussian part distinguishes, a dozen each"""
    lw = S["lw"]
    rent = ~np.isnan(lw.xnum[lw.gauss_specs[0]["x_col"]])
    dep = ~np.isnan(lw.xnum[lw.gauss_specs[1]["x_col"]])
    n = len(rent)
    br = S["obs"][lw.obs_index["br"]] >= 0 if "br" in lw.obs_index else None
    kinds = {"both present": rent & dep, "deposit missing": rent & ~dep, "rent missing": ~rent & dep}
    if br is not None:
        kinds["br observed"] = br & (rent | dep)
        kinds["br missing"] = ~br & (rent | dep)
    rows = []
    for name, sel in kinds.items():
        assert sel.sum() >= 1, f"no row of kind '{name}' among the {n}"
        rows.extend(np.flatnonzero(sel)[:12])
    rows.extend(np.flatnonzero(~rent & ~dep)[:4])  # (every number missing: the Gaussian part is 0.0)
    return np.array(sorted(set(int(r) for r in rows)), dtype=np.int32), kinds


def _engines(model_fn, base_fn, n_rows=600):
    S, S0 = tg.setup(model_fn, n_rows), tg.setup(base_fn, n_rows)
    tg.seed_means(S)
    assert S0["lw"].gauss == {} and np.array_equal(S["trace"].cur, S0["trace"].cur)
    e, e0 = Engine(S["lw"], S["obs"], dist_mode=1), Engine(S0["lw"], S0["obs"], dist_mode=1)
    e.upload_trace(S["trace"])
    e0.upload_trace(S0["trace"])
    return S, S0, e, e0


CASES = {"two_model": (tg.two_model, tg.base_model), "two_candidate_model": (tg.two_candidate_model, tg.base_candidate_model),
         "mixed_model": (tg.mixed_model, tg.base_model)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_gaussian_part_of_existing_candidates(case):
    S, S0, e, e0 = _engines(*CASES[case])
    try:
        lw, tr = S["lw"], S["trace"]
        t = tr.tables["County"]
        rows, kinds = _row_kinds(S)
        excl = tr.cur[0, rows]
        _, a, _ = e.hip.score_node(0, 0, rows, excl=excl, n_cand=t.n + 1, want_scores=True)
        _, b, _ = e0.hip.score_node(0, 0, rows, excl=excl, n_cand=t.n + 1, want_scores=True)
        a, b = a[:, :t.n], b[:, :t.n]
        assert np.array_equal(np.isfinite(a), np.isfinite(b))
        st, ck = t.cols[lw.colidx["County"]["state"]], t.cols[lw.colidx["County"]["countykey"]]
        n_checked, worst = 0, 0.0
        for r, i in enumerate(rows):
            for k in np.flatnonzero(np.isfinite(a[r])):
                want, n_comb = tg.gauss_part(S, int(i), {"state": int(st[k]), "countykey": int(ck[k])})
                tol = posterior_exact.logml_bound(n_comb, want) + 1e-12 * max(1.0, abs(a[r, k]))
                err = abs((a[r, k] - b[r, k]) - want)
                worst = max(worst, err / tol)
                assert err <= tol, (case, int(i), int(k), a[r, k] - b[r, k], want, tol)
                n_checked += 1
        print(f"{case}: {n_checked} candidate scores, worst error / tolerance {worst:.3g}")
        assert n_checked >= 30
        for name, sel in kinds.items():  # the test visited every kind of row
            assert sel[rows].any(), name
    finally:
        e.close()
        e0.close()


@pytest.mark.parametrize("case", sorted(CASES))
def test_gaussian_part_of_the_new_row_branch(case):
    S, S0, e, e0 = _engines(*CASES[case])
    try:
        lw = S["lw"]
        leaf = next(nid for nid, info in enumerate(lw.blocks[0]["node_info"]) if info["kind"] == "leaf" and info["path"] == "state")
        assert len(lw.gauss_more[(0, leaf)]) == 1
        opts = lw.option_values[("County", "state")]
        rows, _ = _row_kinds(S)
        _, a, _ = e.hip.score_node(0, leaf, rows, n_cand=len(opts), want_scores=True)
        _, b, _ = e0.hip.score_node(0, leaf, rows, n_cand=len(opts), want_scores=True)
        assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.isfinite(a).any()
        ck = S["obs"][lw.obs_index["county.countykey"]]
        n_checked = 0
        for r, i in enumerate(rows):
            for k in np.flatnonzero(np.isfinite(a[r])):
                want, n_comb = tg.gauss_part(S, int(i), {"state": int(opts[k]), "countykey": int(ck[i])})
                tol = posterior_exact.logml_bound(n_comb, want) + 1e-12 * max(1.0, abs(a[r, k]))
                assert abs((a[r, k] - b[r, k]) - want) <= tol, (case, int(i), int(k), a[r, k] - b[r, k], want, tol)
                n_checked += 1
        assert n_checked >= len(rows)
    finally:
        e.close()
        e0.close()


def test_declaration_order_does_not_move_the_root_scores():
    """the whole root, NEW column included: rent + deposit against deposit + rent"""
    out = []
    rows = np.arange(600, dtype=np.int32)
    for fn in (tg.two_model, tg.two_model_swapped):
        S = tg.setup(fn, 600)
        tg.seed_means(S)
        eng = Engine(S["lw"], S["obs"], dist_mode=1)
        try:
            eng.upload_trace(S["trace"])
            t = S["trace"].tables["County"]
            lse, sc, _ = eng.hip.score_node(0, 0, rows, excl=S["trace"].cur[0], n_cand=t.n + 1, want_scores=True)
            out.append((lse, sc))
        finally:
            eng.close()
    (la, a), (lb, b) = out
    assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.isfinite(a[:, -1]).any()
    fin = np.isfinite(a)
    assert (np.abs(a[fin] - b[fin]) <= 1e-12 * np.maximum(1.0, np.abs(a[fin]))).all()
    assert (np.abs(la - lb) <= 1e-12 * np.maximum(1.0, np.abs(la))).all()


def test_gaussian_part_of_evidence_sets():
    S, S0 = tg.setup(tg.two_model, 600), tg.setup(tg.base_model, 600)
    tg.seed_means(S)
    _fix_locals(S)
    lw, tr = S["lw"], S["trace"]
    pl, pl0 = lw.latent_plans["County"], S0["lw"].latent_plans["County"]
    node = next(nid for nid, info in enumerate(pl["node_info"]) if info["kind"] == "leaf" and info["path"] == "state")
    assert pl0["node_info"][node]["path"] == "state" and len(lw.gauss_more[(pl["block_id"], node)]) == 1
    live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "County")
    live0, ev_off0, ev_rows0, ev_ctx0 = build_evidence(S0["lw"], S0["trace"], "County")
    assert np.array_equal(live, live0) and np.array_equal(ev_rows, ev_rows0) and ev_ctx is not None
    n_lat = 20
    assert len(live) >= n_lat and (np.diff(ev_off[:n_lat + 1]) > 0).all()
    n_ev = int(ev_off[n_lat])
    opts = lw.option_values[("County", "state")]
    e, e0 = Engine(lw, S["obs"], dist_mode=1), Engine(S0["lw"], S0["obs"], dist_mode=1)
    try:
        e.upload_trace(tr)
        e0.upload_trace(S0["trace"])
        e.hip.set_active_rows(0, -1)
        e0.hip.set_active_rows(0, -1)
        _, a, _ = e.hip.score_node_ev(pl["block_id"], node, live[:n_lat], ev_off[:n_lat + 1], ev_rows[:n_ev],
                                      ev_ctx=ev_ctx[:n_ev], n_cand=len(opts), want_scores=True)
        _, b, _ = e0.hip.score_node_ev(pl0["block_id"], node, live[:n_lat], ev_off[:n_lat + 1], ev_rows[:n_ev],
                                       n_cand=len(opts), want_scores=True)
    finally:
        e.close()
        e0.close()
    assert np.array_equal(np.isfinite(a), np.isfinite(b))
    ck = S["obs"][lw.obs_index["county.countykey"]]
    n_checked = n_two = 0
    for j in range(n_lat):
        for k in np.flatnonzero(np.isfinite(a[j])):
            want, mag = 0.0, 0.0
            for pos in range(ev_off[j], ev_off[j + 1]):
                i = int(ev_rows[pos])
                terms = [tg.term_value(S, g, i, {"state": int(opts[k]), "countykey": int(ck[i])}, [int(v) for v in ev_ctx[pos]])
                         for g in range(2)]
                n_two += all(x is not None for x in terms)
                for x in terms:
                    if x is not None:
                        want += x
                        mag += abs(x)
            assert abs((a[j, k] - b[j, k]) - want) <= 1e-12 * (1.0 + mag), (j, int(k), a[j, k] - b[j, k], want)
            n_checked += 1
    assert n_checked >= n_lat and n_two >= n_lat


# ---- draws: four counties that only BOTH numbers tell apart
D_SIGMAS = 8.0
STATES4 = ["S0", "S1", "S2", "S3"]


def _four_counties(n_rows=2000, seed=21):
    """one county name and key, four states; State is observed in a fifth of the rows, so the referent of the others is
    found through the numbers: means (rent, deposit) = (0,0), (0,D), (D,0), (D,D) above (1000, 1500), D = 8 sigma each"""
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 4, n_rows)
    rent_mean = 1000.0 + D_SIGMAS * tg.RENT_STD * (s // 2)
    dep_mean = 1500.0 + D_SIGMAS * tg.DEPOSIT_STD * (s % 2)
    rent = np.round(rent_mean + rng.normal(0, tg.RENT_STD, n_rows))
    dep = np.round(dep_mean + rng.normal(0, tg.DEPOSIT_STD, n_rows))
    seen = rng.random(n_rows) < 0.2
    seen[:4] = True
    s[:4] = np.arange(4)  # (every state occurs in the observed column)
    no_rent, no_dep = rng.random(n_rows) < 0.1, rng.random(n_rows) < 0.1
    name = "Alder County"
    clean = {"County": [name] * n_rows, "State": [STATES4[v] for v in s], "Monthly Rent": [float(v) for v in rent],
             "Deposit": [float(v) for v in dep]}
    dirty = {"County": [name] * n_rows, "CountyKey": [f"{name[0]}{name.split()[0][-1]}"] * n_rows,
             "State": [STATES4[v] if o else None for v, o in zip(s, seen)],
             "Monthly Rent": [None if m else float(v) for v, m in zip(rent, no_rent)],
             "Deposit": [None if m else float(v) for v, m in zip(dep, no_dep)]}
    return dirty, clean, s, rent_mean, dep_mean


def _fraction_right(model_fn, query_fn, dirty, truth, sel):
    from pclean_amd.model import LoweredModel
    m = model_fn(dirty)
    lw = LoweredModel(m, query_fn(m), dirty)
    obs = lw.encode_observations(dirty)
    eng = Engine(lw, obs, dist_mode=1)
    try:
        cfg = InferenceConfig(2, 2, use_mh_instead_of_pg=True, rejuv_frequency=500)
        tr = Trace(lw, obs.shape[1], 9)
        initialize_trace(eng, tr, cfg, 9, max_batch=256)
        run_inference(eng, tr, cfg, 9)
        tr.check_consistency()
    finally:
        eng.close()
    t = tr.tables["County"]
    dom = lw.latent_dom[("County", "state")]
    got = t.cols[lw.colidx["County"]["state"], tr.cur[0]]
    want = np.array([dom.get(STATES4[v]) for v in truth])
    return float(np.mean(got[sel] == want[sel]))


def test_draws_need_both_numbers():
    dirty, clean, s, rent_mean, dep_mean = _four_counties()
    both = np.array([r is not None and d is not None for r, d in zip(dirty["Monthly Rent"], dirty["Deposit"])])
    assert both.sum() >= 1500
    # the restatement's MAP at the true means: argmax over the four counties of N(rent) + N(deposit)
    rent = np.array([np.nan if v is None else v for v in dirty["Monthly Rent"]])
    dep = np.array([np.nan if v is None else v for v in dirty["Deposit"]])
    sc = np.stack([tg.normal_logpdf(rent, 1000.0 + D_SIGMAS * tg.RENT_STD * (c // 2), tg.RENT_STD)
                   + tg.normal_logpdf(dep, 1500.0 + D_SIGMAS * tg.DEPOSIT_STD * (c % 2), tg.DEPOSIT_STD) for c in range(4)])
    assert np.mean(np.argmax(sc[:, both], axis=0) == s[both]) >= 0.99
    two = _fraction_right(tg.two_candidate_model, tg.query, dirty, s, both)
    one = _fraction_right(ap.candidate_mean_model, ap.query, dirty, s, both)
    print(f"rows with both numbers at the right county: two terms {two:.4f}, rent alone {one:.4f}")
    assert two >= 0.95
    assert one < 0.70


def _end_to_end(seed):
    S = tg.setup(tg.two_model, 4000)
    lw, obs = S["lw"], S["obs"]
    eng = Engine(lw, obs, dist_mode=1)
    try:
        cfg = InferenceConfig(2, 2, use_mh_instead_of_pg=True, rejuv_frequency=500)
        tr = Trace(lw, obs.shape[1], seed)
        initialize_trace(eng, tr, cfg, seed, max_batch=1024)
        run_inference(eng, tr, cfg, seed)
        tr.check_consistency()
        return S, tr
    finally:
        eng.close()


def test_two_gauss_end_to_end():
    S, tr = _end_to_end(7)
    _, tr2 = _end_to_end(7)
    lw = S["lw"]
    assert np.array_equal(tr.cur, tr2.cur) and np.array_equal(tr.locals[0], tr2.locals[0])
    assert len(tr.mean_params) == 2
    for g in range(2):
        assert np.array_equal(tr.mean_params[g].value, tr2.mean_params[g].value)
    # both parameters' Gibbs draws given the final assignment: every cell with 20 or more rows lies within 6 posterior
    # standard deviations of its rows' mean (priors 1500 / 2000 +- 1000, sigma 150 / 80)
    tr.resample_parameters("Obs")
    for g, (prior_mean, sigma) in enumerate([(1500.0, tg.RENT_STD), (2000.0, tg.DEPOSIT_STD)]):
        rows, idx, xs = tr.gaussian_index(g)
        n = np.bincount(idx, minlength=len(tr.mean_params[g].value))
        sm = np.bincount(idx, weights=xs, minlength=len(tr.mean_params[g].value))
        cells = np.flatnonzero(n >= 20)
        assert len(cells) >= 5
        var = 1.0 / (1.0 / 1000.0 ** 2 + n[cells] / sigma ** 2)
        post = var * (prior_mean / 1000.0 ** 2 + sm[cells] / sigma ** 2)
        assert (np.abs(tr.mean_params[g].value[cells] - post) <= 6 * np.sqrt(var)).all(), g
    # imputations are counted for both numeric columns
    acc = evaluate_accuracy(lw, tr, S["dirty"], S["clean"])
    n_imp = {c: sum(1 for d, k in zip(S["dirty"][c], S["clean"][c]) if d is None and k is not None)
             for c in ("Monthly Rent", "Deposit")}
    assert n_imp["Monthly Rent"] > 100 and n_imp["Deposit"] > 300
    only_rent = dict(S["dirty"]), dict(S["clean"])
    del only_rent[0]["Deposit"], only_rent[1]["Deposit"]
    acc_rent = evaluate_accuracy(lw, tr, *only_rent)
    assert acc["imputed"] == acc_rent["imputed"] + n_imp["Deposit"] and acc_rent["imputed"] >= n_imp["Monthly Rent"]


@pytest.mark.parametrize("dd", [True, False])
def test_many_small_windows_equal_one_sweep(dd):
    """300 windows of two rows against one sweep of the 600: every window resolves the further terms of the root and of the
    open leaf to pointers of its own, hundreds of times in a row; draws are keyed by the row, nothing is committed in
    between, so every output of every row must be the same bit for bit"""
    S = tg.setup(tg.two_model, 600)
    tg.seed_means(S)
    _fix_locals(S)
    lw, tr, obs = S["lw"], S["trace"], S["obs"]
    n, W = obs.shape[1], 2
    cfg = InferenceConfig(1, 3, use_mh_instead_of_pg=False, rejuv_frequency=500, use_dd_proposals=dd)
    eng = Engine(lw, obs, dist_mode=1)
    try:
        eng.upload_trace(tr)

        def sweep(lo, hi):
            choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 5, 0, lo=lo, hi=hi)
            rows, vals = new_rows.get(0, (np.zeros(0, np.int32), np.zeros((0, len(lw.blocks[0]["nodes"])), np.int32)))
            order = np.argsort(rows, kind="stable")  # (one record per row that chose NEW)
            return [choice.copy(), chosen.copy(), logml.copy(), tr.pending_locals[0].copy(), rows[order] + lo, vals[order]]

        whole = sweep(0, n)
        parts = [sweep(lo, min(lo + W, n)) for lo in range(0, n, W)]
    finally:
        eng.close()
    assert len(parts) > 256
    names = ["choice", "chosen_particle", "logml", "pending_locals", "new rows", "new-row values"]
    for k, name in enumerate(names):
        got = np.concatenate([p[k] for p in parts], axis=1 if name == "choice" else 0)
        assert got.shape == whole[k].shape and np.array_equal(got, whole[k]), name
    assert (whole[2] != 0).any() and (whole[3][:, 0] >= 0).all()
