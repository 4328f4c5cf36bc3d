"""IndexedProportionsParameter (keyed form) and NumberCodePrior on the GPU: per-candidate scores of the new-row leaves and
of the latent roots against the restatement's sum of the same doubles in plan order, sweep draws against the exact
posteriors of tests/indexed_program.py (new rows, existing rows, latent rows under evidence; the size of the code deciding
between a new row and an existing one), the device commit against the host commit, and run_inference end to end."""
import copy

import numpy as np
import pytest

import indexed_program as ip
import posterior_exact as pe
from pclean_amd import _lib
from pclean_amd import inference as inf
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import build_evidence, latent_current_choices
from pclean_amd.trace import Trace
from test_indexed_proportions import expected_outputs

pytestmark = pytest.mark.gpu

HALF_LOG26 = 1.629048269010741


# ---- scores --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scored():
    """the program with missing observations (npi and the city each missing on some rows, both on row 0) under
    the number-code prior and under its Unmodeled twin, one engine each"""
    out = {}
    for code_prior in (True, False):
        S = ip.draw_program(missing=True, code_prior=code_prior)
        eng = Engine(S["lw"], S["obs"], dist_mode=1)
        eng.upload_trace(S["trace"])
        S["eng"] = eng
        out[code_prior] = S
    yield out
    for S in out.values():
        S["eng"].close()


def _term_values(S, t, cols):
    """function(observed value index or -1) -> the term's double per option (None: the term is skipped), restated"""
    lw, eng = S["lw"], S["eng"]
    val = cols[int(t["cand_col"])]
    if t["dens_kind"] == _lib.DENS_EQUAL:
        return lambda o: None if o < 0 else np.where(val == o, 0.0, -np.inf)
    assert t["dens_kind"] == _lib.DENS_ADD_TYPOS
    _, _, _, nb, logl = eng.hip.get_density_tables()
    (odom, ldom), = [(od, ld) for pid, od, ld in lw.pair_id.values() if pid == int(t["pair_table"])]
    D = eng.hip.get_pair_table(int(t["pair_table"]), len(odom), len(ldom)).astype(np.int64)
    L = np.array([len(ldom.string(v)) for v in range(len(ldom))])

    def fn(o):
        if o < 0:
            return None  # an AddTypos term skips a missing observation (add_typos.jl:51-53)
        d = D[o, val]
        l = nb[(L[val] + 4) // 5, d].copy()  # the three operations of term_density
        l -= logl[L[val]] * d.astype(np.float64)
        l -= HALF_LOG26 * d.astype(np.float64)
        return l
    return fn


def _leaf_prior(S, attr):
    """the option prior of a Doc leaf restated from the strings, in the lowering's option order, and its value columns"""
    lw = S["lw"]
    dom = lw.latent_dom[("Doc", attr)]
    vals = lw.option_values[("Doc", attr)]
    if attr == "npi":
        codes = np.array([float(int(dom.string(int(v)))) for v in vals])
        return (-np.log(codes) if S["code_prior"] else np.zeros(len(vals))), {0: vals}
    if attr == "state":
        return np.zeros(len(vals)), {0: vals}
    keys = lw.option_keycol[("Doc", attr)]
    th = ip.theta_by_string(S)
    kdom = lw.latent_dom[("Doc", "state")]
    return np.array([np.log(th[kdom.string(int(k))][dom.string(int(v))]) for v, k in zip(vals, keys)]), {0: vals, 1: keys}


def _node_terms(arrays, nid):
    nodes, terms = arrays[0], arrays[1]
    return terms[nodes[nid]["term_begin"]:nodes[nid]["term_begin"] + nodes[nid]["n_terms"]]


@pytest.mark.parametrize("attr", ["npi", "state", "city"])
@pytest.mark.parametrize("code_prior", [True, False], ids=["NumberCodePrior", "Unmodeled"])
def test_new_row_leaf_scores_equal_the_restatement(scored, code_prior, attr):
    """score_node on a leaf of the new-row branch, every row: prior, then the terms in plan order — with the code's
    observation missing, the city's missing, both and neither"""
    S = scored[code_prior]
    lw, eng, obs = S["lw"], S["eng"], S["obs"]
    arrays = lw.block_arrays(0)
    (nid,) = [i for i, info in enumerate(lw.blocks[0]["node_info"]) if info["kind"] == "leaf" and info["attr"] == attr]
    logp, cols = _leaf_prior(S, attr)
    dev_logp, _, _ = eng.hip.get_table_priors(lw.option_id[("Doc", attr)], len(logp), is_options=True)
    assert np.array_equal(dev_logp, logp)
    terms = [(int(t["obs_col"]), _term_values(S, t, cols)) for t in _node_terms(arrays, nid)]
    n = obs.shape[1]
    want = np.empty((n, len(logp)))
    seen = set()
    for i in range(n):
        sk = logp.copy()
        for col, fn in terms:
            v = fn(int(obs[col, i]))
            if v is not None:
                sk = sk + v
        want[i] = sk
        seen.add((obs[lw.obs_index["d.npi"], i] < 0, obs[lw.obs_index["city_obs"], i] < 0))
    assert len(seen) == 4  # the code missing, the city missing, both, neither (the key never is: the lowering refuses that)
    _, got, _ = eng.hip.score_node(0, nid, np.arange(n, dtype=np.int32), n_cand=len(logp), want_scores=True)
    assert np.array_equal(got, want)


def test_number_code_shifts_the_new_row_by_minus_log_code(scored):
    """the npi leaf under NumberCodePrior minus the leaf of the Unmodeled twin: -np.log(code) at the prior's place, so the
    restated sums differ by exactly that double wherever the score is finite; and the slot's new-row candidate takes
    the leaves' marginals in plan order on both programs"""
    A, B = scored[True], scored[False]
    lw, obs = A["lw"], A["obs"]
    n = obs.shape[1]
    rows = np.arange(n, dtype=np.int32)
    dom = lw.latent_dom[("Doc", "npi")]
    codes = np.array([float(int(dom.string(v))) for v in range(len(dom))])
    _, a, _ = A["eng"].hip.score_node(0, 1, rows, n_cand=len(dom), want_scores=True)
    _, b, _ = B["eng"].hip.score_node(0, 1, rows, n_cand=len(dom), want_scores=True)
    assert np.array_equal(np.isfinite(a), np.isfinite(b)) and np.isfinite(a).any()
    assert np.array_equal(a, -np.log(codes)[None, :] + b)  # (b is 0.0 or -inf: the sum is the restated one)
    for S in (A, B):
        eng, tr = S["eng"], S["trace"]
        t = tr.tables["Doc"]
        lse = [eng.hip.score_node(0, nid, rows, n_cand=len(S["lw"].option_values[("Doc", attr)]))[0]
               for nid, attr in ((1, "npi"), (2, "state"), (3, "city"))]
        _, _, scal = eng.hip.get_table_priors(lw.table_id["Doc"], t.n)
        excl = tr.cur[0]
        _, got, _ = eng.hip.score_node(0, 0, rows, excl=excl, n_cand=t.n + 1, want_scores=True)
        for i in range(n):
            deleted = t.counts[excl[i]] <= 1
            snew = 0.0
            for l in lse:
                snew += l[i]
            assert got[i, t.n] == ((scal[3] if deleted else scal[2]) - scal[1]) + snew, i


def test_latent_root_scores_equal_the_restatement(scored):
    """score_node_ev on the city root of Doc's own plan: evidence sets of 1, 3 and 40 rows with repeats and missing values;
    per term multiplicity x density over the distinct observed values ascending, missing first"""
    S = scored[True]
    lw, eng, obs = S["lw"], S["eng"], S["obs"]
    pl = lw.latent_plans["Doc"]
    arrays = lw.latent_block_arrays("Doc")
    n = obs.shape[1]
    rng = np.random.default_rng(4)
    sets = [np.array([5]), np.array([0, 9, 9]), np.concatenate([[0, 1, 2, 7], rng.integers(0, n, 36)])]
    ev_rows = np.concatenate(sets).astype(np.int32)
    ev_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    eng.hip.set_active_rows(0, -1)
    for node, attr in enumerate(pl["root_attr"]):
        logp, cols = _leaf_prior(S, attr)
        terms = [(int(t["obs_col"]), _term_values(S, t, cols), int(t["dens_kind"])) for t in _node_terms(arrays, node)]
        want = np.empty((3, len(logp)))
        for k, rows in enumerate(sets):
            sk = logp.copy()
            for col, fn, kind in terms:
                vals, mult = np.unique(obs[col, rows], return_counts=True)
                for o, c in zip(vals, mult):
                    v = fn(int(o))
                    if v is not None:
                        with np.errstate(invalid="ignore"):
                            sk = sk + np.where(np.isinf(v), v, np.float64(c) * v)
            want[k] = sk
        _, got, _ = eng.hip.score_node_ev(pl["block_id"], node, np.arange(3, dtype=np.int32), ev_off, ev_rows, n_cand=len(logp),
                                          want_scores=True)
        assert np.array_equal(got, want), attr


# ---- exact posteriors --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drawn():
    S = ip.draw_program()
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    eng.upload_trace(S["trace"])
    S["eng"] = eng
    yield S
    eng.close()


def _codes(S, choice_row, new_rows):
    """referent, or ('NEW', city string) from the new-row record's option (value, key) — whose key must be the observed one"""
    lw = S["lw"]
    out = [int(c) for c in choice_row]
    if new_rows is not None:
        rows, vals = new_rows
        opt = vals[:, 3]
        kdom = lw.latent_dom[("Doc", "state")]
        for j, (i, o) in enumerate(zip(rows, opt)):
            assert kdom.string(int(lw.option_keycol[("Doc", "city")][o])) == S["dirty"]["State"][i]
            assert vals[j, 2] == lw.option_keycol[("Doc", "city")][o]  # the state leaf took the same key
            out[i] = ("NEW", ip.CITIES[int(lw.option_values[("Doc", "city")][o])])
    assert all(not isinstance(c, int) or c >= 0 for c in out)
    return out


@pytest.mark.parametrize("P,mh", [(2, True), (5, False)], ids=["MH", "PG5"])
def test_sweep_draws_follow_the_exact_posterior(drawn, P, mh):
    """every observed row, S_GPU sweeps of the frozen trace: existing referents and ('NEW', city) against the closed forms
    of posterior_exact with pi restated from the strings; the rows of the large codes must stay with existing rows, those
    of code 1 open new rows"""
    S = drawn
    tr, eng = S["trace"], S["eng"]
    n = tr.cur.shape[1]
    rows = np.arange(n)
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
    D = [[] for _ in rows]
    for s in range(pe.S_GPU):
        choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 411 + P, s)
        for i, c in enumerate(_codes(S, choice[0], new_rows.get(0))):
            D[i].append(c)
        if s == 0:
            for i in rows:
                z = pe.log_marginal(ip.block_scores(S, int(i)))
                assert abs(float(logml[i]) - z) <= pe.logml_bound(tr.tables["Doc"].n + 40, z), i
    items, new_mass = [], {}
    for i in rows:
        pi = pe.normalise(ip.block_scores(S, int(i)))
        cur = int(tr.cur[0, i])
        e = pe.mh_one_block(pi, cur) if mh else pe.pg_one_block(pi, cur, P)
        items.append((int(i), e, pe.tabulate(D[i])))
        # (the row's entity outlives the row and holds the observed city, or none is observed: an existing row fits)
        if tr.tables["Doc"].counts[cur] >= 2 and S["rows"][i][3] in (None, S["ents"][S["rows"][i][0]][2]):
            new_mass.setdefault(S["dirty"]["NPI"][i], []).append(sum(v for k, v in pi.items() if isinstance(k, tuple)))
    res = pe.gof(items)
    print(f"\n[P={P}{' MH' if mh else ''}] {pe.describe(res)}; new-row mass by code: "
          + ", ".join(f"{c}: {min(v):.2g}..{max(v):.2g}" for c, v in new_mass.items()))
    # the code's size decides: below code 1 a new row competes with the entity the row came from, below a ten-digit code
    # (-log(code) = -20.9) it does not; counts (1-3) and theta move the ratio by two orders of magnitude at the most
    assert min(new_mass["1"]) >= 1e-3 and max(new_mass["1234567893"]) <= 1e-6
    assert res["p"] > pe.ALPHA, pe.describe(res)
    wrong = pe.gof([(i, e, o) for (i, _, o), e in zip(items, expected_outputs(S, rows, P, ip.theta_by_string(S, shift=1)))]) \
        if not mh else None
    assert wrong is None or wrong["p"] < pe.ALPHA


@pytest.mark.parametrize("P,mh", [(2, True), (5, False)], ids=["MH", "PG5"])
def test_latent_city_draws_follow_the_exact_posterior(drawn, P, mh):
    """sweep_latent of Doc: the city root's option (value, key) under the evidence rows' states and cities"""
    S = drawn
    lw, tr, eng = S["lw"], S["trace"], S["eng"]
    live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "Doc")
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
    excl = latent_current_choices(lw, tr, "Doc", live, cfg)
    pl = lw.latent_plans["Doc"]
    root = pl["roots"][pl["root_attr"].index("city")]
    t, ci = tr.tables["Doc"], lw.colidx["Doc"]
    nb = len(ip.CITIES)
    cur = t.cols[ci["state"], live].astype(np.int64) * nb + t.cols[ci["city"], live]
    D = np.empty((pe.S_GPU, len(live)), dtype=np.int64)
    for s in range(pe.S_GPU):
        chosen, vals = eng.sweep_latent(tr, "Doc", cfg, 77 + P, s, live, ev_off, ev_rows, ev_ctx, excl)
        D[s] = np.where(chosen == 0, cur, vals[:, root])
    kdom = lw.latent_dom[("Doc", "state")]
    kidx = {kdom.string(k): k for k in range(len(kdom))}
    items = []
    for j in range(len(live)):
        ev = [tuple(S["dirty"][c][r] for c in ("NPI", "State", "City")) for r in ev_rows[ev_off[j]:ev_off[j + 1]]]
        pi = {kidx[st] * nb + ip.CITIES.index(c): v for (st, c), v in pe.normalise(ip.latent_city_scores(S, ev)).items()}
        e = pe.mh_one_block(pi, int(cur[j])) if mh else pe.pg_one_block(pi, int(cur[j]), P)
        items.append((j, e, pe.tabulate(D[:, j].tolist())))
    res = pe.gof(items)
    print(f"\n[latent P={P}{' MH' if mh else ''}] {pe.describe(res)}")
    assert res["p"] > pe.ALPHA, pe.describe(res)


# ---- commits and run_inference -------------------------------------------------------------------------------------------
def _run(cfg, device_commit, monkeypatch, seed=5):
    from test_gpu_commit import _same_state  # noqa: F401
    monkeypatch.setattr(inf, "DEVICE_COMMIT", device_commit)
    S = ip.synthetic()
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        tr = Trace(S["lw"], S["obs"].shape[1], 3)
        inf.initialize_trace(eng, tr, cfg, seed, max_batch=64)
        inf.run_inference(eng, tr, cfg, seed)
        dc = dict(commits=eng._dc["commits"], fallbacks=eng._dc["fallbacks"]) if eng._dc is not None else None
        tr.check_consistency()
        return copy.deepcopy(tr), dc, S
    finally:
        eng.close()


@pytest.mark.parametrize("mh", [True, False], ids=["MH", "PG5"])
def test_run_inference_device_commit_equals_host_commit(monkeypatch, mh):
    """300 rows with strongly state-dependent cities, 3 iterations: rows created through the keyed leaf, collected and
    their ids reused; committed on the device without a refusal == committed on the host; [key][option] counts == the
    recount; a second run with the same seed is identical"""
    from test_gpu_commit import _same_state
    cfg = InferenceConfig(3, 5, use_mh_instead_of_pg=mh)
    a, dc, S = _run(cfg, True, monkeypatch)
    assert dc is not None and dc["commits"] >= 3 and dc["fallbacks"] == 0, dc
    b, _, _ = _run(cfg, False, monkeypatch)
    _same_state(a, b, "device vs host commit")
    c, dc2, _ = _run(cfg, True, monkeypatch)
    _same_state(a, c, "two runs with one seed")
    for k in a.params:
        assert np.array_equal(a.params[k].value, c.params[k].value)
    t = a.tables["Doc"]
    assert np.array_equal(a.params[("Doc", "theta")].counts, a.recount("Doc", "city"))
    assert a.params[("Doc", "theta")].counts.sum() == int(t.live[:t.n].sum()) and len(t.free) + int(t.live[:t.n].sum()) == t.n
    # brute force over the strings
    lw = S["lw"]
    kdom, vdom, ci = lw.latent_dom[("Doc", "state")], lw.latent_dom[("Doc", "city")], lw.colidx["Doc"]
    want = np.zeros((len(kdom), len(ip.CITIES)), dtype=np.int64)
    for r in np.flatnonzero(t.live[:t.n]):
        want[int(t.cols[ci["state"], r]), ip.CITIES.index(vdom.string(int(t.cols[ci["city"], r])))] += 1
    assert np.array_equal(want, a.params[("Doc", "theta")].counts)
