"""The product leaf (an indexed ChooseProportionally enumerated jointly with its sibling index) on the GPU: per-candidate
scores of the new-row leaf and of the latent pair root against the restatement's sum of the same doubles in plan order,
sweep draws and latent updates against exact posteriors restated from the strings, the refusal of prior proposals, the
device commit against the host commit and run_inference end to end."""
import numpy as np
import pytest

import indexed_program as ip
import posterior_exact as pe
from pclean_amd import _lib
from pclean_amd import inference as inf
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import build_evidence, latent_current_choices
from pclean_amd.trace import Trace
from test_gpu_indexed_proportions import _node_terms, _term_values

pytestmark = pytest.mark.gpu

NA, NB = len(ip.DEGREES), len(ip.SPECS)


@pytest.fixture(scope="module", params=[False, True], ids=["ChooseProportionally", "ChooseUniformly"])
def prog(request):
    S = ip.product_program(uniform_index=request.param, free_every=3)
    assert (S["trace"].cur[0] < 0).sum() >= 5
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    eng.upload_trace(S["trace"])
    S["eng"] = eng
    yield S
    eng.close()


@pytest.fixture(scope="module")
def full():
    """every observed row has a referent (evidence sets cover all rows)"""
    S = ip.product_program(seed=1)
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    eng.upload_trace(S["trace"])
    S["eng"] = eng
    yield S
    eng.close()


def _joint_prior(S):
    """log pA(a) + log theta_a[b] in option order a * |B| + b, the two doubles added in that order"""
    la, lt = ip.product_priors(S)
    return np.array([np.float64(la[a]) + np.float64(lt[a][b]) for a in ip.DEGREES for b in ip.SPECS])


def test_leaf_scores_equal_the_restatement(prog):
    """score_node on the product leaf, every row: deg_obs missing, spec_obs missing, both, neither"""
    S = prog
    lw, eng, obs = S["lw"], S["eng"], S["obs"]
    logp = _joint_prior(S)
    dev_logp, _, _ = eng.hip.get_table_priors(lw.option_id[("Doc", "spec")], NA * NB, is_options=True)
    assert np.array_equal(dev_logp, logp)
    cols = {0: lw.option_cols[("Doc", "spec")][0], 1: lw.option_cols[("Doc", "spec")][1]}
    terms = [(int(t["obs_col"]), _term_values(S, t, cols)) for t in _node_terms(lw.block_arrays(0), 1)]
    n = obs.shape[1]
    want = np.empty((n, NA * NB))
    seen = set()
    for i in range(n):
        sk = logp.copy()
        for col, fn in terms:
            v = fn(int(obs[col, i]))
            if v is not None:
                sk = sk + v
        want[i] = sk
        seen.add((obs[0, i] < 0, obs[1, i] < 0))
    assert len(seen) == 4
    _, got, _ = eng.hip.score_node(0, 1, np.arange(n, dtype=np.int32), n_cand=NA * NB, want_scores=True)
    assert np.array_equal(got, want)


def test_latent_root_scores_equal_the_restatement(prog):
    S = prog
    lw, eng, obs = S["lw"], S["eng"], S["obs"]
    pl = lw.latent_plans["Doc"]
    n = obs.shape[1]
    rng = np.random.default_rng(6)
    sets = [np.array([4]), np.array([1, 8, 8]), np.concatenate([[0, 1, 2, 5], rng.integers(0, n, 36)])]
    ev_rows = np.concatenate(sets).astype(np.int32)
    ev_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    eng.hip.set_active_rows(0, -1)
    logp = _joint_prior(S)
    cols = {0: lw.option_cols[("Doc", "spec")][0], 1: lw.option_cols[("Doc", "spec")][1]}
    terms = [(int(t["obs_col"]), _term_values(S, t, cols)) for t in _node_terms(lw.latent_block_arrays("Doc"), 0)]
    want = np.empty((3, NA * NB))
    for k, rows in enumerate(sets):
        sk = logp.copy()
        for col, fn in terms:
            vals, mult = np.unique(obs[col, rows], return_counts=True)  # ascending: missing first
            for o, c in zip(vals, mult):
                v = fn(int(o))
                if v is not None:
                    sk = sk + np.float64(c) * v
        want[k] = sk
    _, got, _ = eng.hip.score_node_ev(pl["block_id"], 0, np.arange(3, dtype=np.int32), ev_off, ev_rows, n_cand=NA * NB,
                                      want_scores=True)
    assert np.array_equal(got, want)


def _expected(S, rows, P, mh, shift=0):
    out = []
    for i in rows:
        pi = pe.normalise(ip.product_block_scores(S, int(i), shift))
        cur = int(S["trace"].cur[0, i])
        cur = None if cur < 0 else cur
        out.append(pe.mh_one_block(pi, cur) if (mh and cur is not None) else pe.pg_one_block(pi, cur, P))
    return out


def test_restatement_rejects_theta_of_the_wrong_key_cpu_side(prog):
    """before the device is asserted on: draws sampled from the exact output distributions (S_GPU per row) pass gof() at
    the threshold of the device test against themselves and fail against the twin reading theta one degree further"""
    S = prog
    rows = np.arange(S["trace"].cur.shape[1])
    right, wrong = _expected(S, rows, 5, False), _expected(S, rows, 5, False, shift=1)
    rng = np.random.default_rng(2)
    ir, iw = [], []
    for i, e, w in zip(rows, right, wrong):
        keys = list(e)
        p = np.array([e[k] for k in keys])
        obs = pe.tabulate([keys[j] for j in rng.choice(len(keys), size=pe.S_GPU, p=p / p.sum())])
        ir.append((int(i), e, obs))
        iw.append((int(i), w, obs))
    assert pe.gof(ir)["p"] > pe.ALPHA and pe.gof(iw)["p"] < pe.ALPHA


@pytest.mark.parametrize("P,mh", [(2, True), (5, False), (20, False)], ids=["MH", "PG5", "PG20"])
def test_sweep_draws_follow_the_exact_posterior(prog, P, mh):
    """existing referents and ('NEW', (degree, spec)) of every observed row — with and without a current referent —
    against the closed forms of posterior_exact; the new row's record names the pair by its option a * |B| + b"""
    S = prog
    tr, eng = S["trace"], S["eng"]
    n = tr.cur.shape[1]
    rows = np.arange(n)
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
    D = [[] for _ in rows]
    n_new = 0
    for s in range(pe.S_GPU):
        choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 900 + P, s)
        out = [int(c) for c in choice[0]]
        if 0 in new_rows:
            r_, v_ = new_rows[0]
            n_new += len(r_)
            for i, o in zip(r_, v_[:, 1]):
                out[i] = ("NEW", (ip.DEGREES[int(o) // NB], ip.SPECS[int(o) % NB]))
        assert all(not isinstance(c, int) or c >= 0 for c in out)
        for i, c in enumerate(out):
            D[i].append(c)
        if s == 0:
            for i in rows:
                z = pe.log_marginal(ip.product_block_scores(S, int(i)))
                assert abs(float(logml[i]) - z) <= pe.logml_bound(tr.tables["Doc"].n + NA * NB + 1, z), i
    res = pe.gof([(int(i), e, pe.tabulate(D[i])) for i, e in zip(rows, _expected(S, rows, P, mh))])
    print(f"\n[product P={P}{' MH' if mh else ''}] {pe.describe(res)}; {n_new} new-row records")
    assert n_new > 0
    assert res["p"] > pe.ALPHA, pe.describe(res)


@pytest.mark.parametrize("P,mh", [(2, True), (5, False)], ids=["MH", "PG5"])
def test_latent_pair_draws_follow_the_exact_posterior(full, P, mh):
    """sweep_latent of Doc: the pair root's option under the evidence rows' two observations"""
    S = full
    lw, tr, eng = S["lw"], S["trace"], S["eng"]
    live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "Doc")
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
    excl = latent_current_choices(lw, tr, "Doc", live, cfg)
    t, ci = tr.tables["Doc"], lw.colidx["Doc"]
    cur = t.cols[ci["degree"], live].astype(np.int64) * NB + t.cols[ci["spec"], live]
    D = np.empty((pe.S_GPU, len(live)), dtype=np.int64)
    for s in range(pe.S_GPU):
        chosen, vals = eng.sweep_latent(tr, "Doc", cfg, 55 + P, s, live, ev_off, ev_rows, ev_ctx, excl)
        D[s] = np.where(chosen == 0, cur, vals[:, 0])
    items = []
    for j in range(len(live)):
        ev = [(S["dirty"]["Degree"][r], S["dirty"]["Spec"][r]) for r in ev_rows[ev_off[j]:ev_off[j + 1]]]
        pi = {ip.DEGREES.index(a) * NB + ip.SPECS.index(b): v for (a, b), v in pe.normalise(ip.product_latent_scores(S, ev)).items()}
        e = pe.mh_one_block(pi, int(cur[j])) if mh else pe.pg_one_block(pi, int(cur[j]), P)
        items.append((j, e, pe.tabulate(D[:, j].tolist())))
    res = pe.gof(items)
    print(f"\n[product latent P={P}{' MH' if mh else ''}] {pe.describe(res)}")
    assert res["p"] > pe.ALPHA, pe.describe(res)


def test_prior_proposals_are_refused(full):
    S = full
    cfg = InferenceConfig(1, 3, use_dd_proposals=False)
    with pytest.raises(_lib.PCleanHipError, match=r"Engine\.sweep: a product leaf .* under use_dd_proposals = false"):
        S["eng"].sweep(S["trace"], cfg, 1, 0)
    live, ev_off, ev_rows, ev_ctx = build_evidence(S["lw"], S["trace"], "Doc")
    with pytest.raises(_lib.PCleanHipError, match=r"Engine\.sweep_latent: a product leaf .* under use_dd_proposals = false"):
        S["eng"].sweep_latent(S["trace"], "Doc", cfg, 1, 0, live, ev_off, ev_rows, ev_ctx,
                              np.full((1, len(live)), -1, np.int32))


def _run(cfg, device_commit, monkeypatch, seed=9):
    import copy
    monkeypatch.setattr(inf, "DEVICE_COMMIT", device_commit)
    S = ip.product_synthetic()
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
    """300 rows whose speciality depends on the degree, 3 iterations: rows created through the product leaf (both columns
    written on the device), collected and reused; no refusal; device == host; counts == recount; two runs identical"""
    from test_gpu_commit import _same_state
    cfg = InferenceConfig(3, 5, use_mh_instead_of_pg=mh)
    a, dc, S = _run(cfg, True, monkeypatch)
    assert dc is not None and dc["commits"] >= 3 and dc["fallbacks"] == 0, dc
    b, _, _ = _run(cfg, False, monkeypatch)
    _same_state(a, b, "device vs host commit")
    c, _, _ = _run(cfg, True, monkeypatch)
    _same_state(a, c, "two runs with one seed")
    t, ci = a.tables["Doc"], S["lw"].colidx["Doc"]
    want = np.zeros((NA, NB), dtype=np.int64)
    for r in np.flatnonzero(t.live[:t.n]):
        want[t.cols[ci["degree"], r], t.cols[ci["spec"], r]] += 1
    assert np.array_equal(a.params[("Doc", "theta")].counts, want)
    assert np.array_equal(a.params[("Doc", "deg_p")].counts, want.sum(axis=1))
    assert (want > 0).sum() > NA  # (more pairs than degrees survive: both columns were written)


@pytest.mark.parametrize("na,nb", [(3, 5), (7, 300), (51, 500)], ids=["3x5", "7x300", "51x500"])
def test_shapes_score_like_the_restatement_and_sweep(na, nb):
    """15, 2 100 (scores resident in LDS) and 25 500 joint options (more than 20 k: the recomputing kernel): the leaf's
    scores equal prior + terms in plan order bit for bit over 64 rows, and a sweep from the empty table gives every row a
    new-row record whose option lies in the product, identically when repeated"""
    S = ip.product_shape_program(na, nb)
    lw, obs, tr = S["lw"], S["obs"], S["trace"]
    eng = Engine(lw, obs, dist_mode=1)
    try:
        eng.upload_trace(tr)
        S["eng"] = eng
        la = np.log(tr.params[("Doc", "deg_p")].value)
        lt = np.log(tr.params[("Doc", "theta")].value)
        logp = (la[:, None] + lt).reshape(-1)
        cols = {0: lw.option_cols[("Doc", "spec")][0], 1: lw.option_cols[("Doc", "spec")][1]}
        assert np.array_equal(cols[0], np.arange(na * nb) // nb) and np.array_equal(cols[1], np.arange(na * nb) % nb)
        terms = [(int(t["obs_col"]), _term_values(S, t, cols)) for t in _node_terms(lw.block_arrays(0), 1)]
        n = obs.shape[1]
        want = np.empty((n, na * nb))
        for i in range(n):
            sk = logp.copy()
            for col, fn in terms:
                v = fn(int(obs[col, i]))
                if v is not None:
                    sk = sk + v
            want[i] = sk
        lse, got, _ = eng.hip.score_node(0, 1, np.arange(n, dtype=np.int32), n_cand=na * nb, want_scores=True)
        assert np.array_equal(got, want)
        for P, mh in ((2, True), (5, False), (20, False)):
            cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
            outs = []
            for rep in range(2):
                choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 31, 0)
                rows, vals = new_rows[0]
                assert (choice[0] == -1).all() and np.array_equal(rows, np.arange(n))
                assert ((vals[:, 1] >= 0) & (vals[:, 1] < na * nb)).all()
                outs.append((chosen.copy(), logml.copy(), np.array(vals)))
            assert all(np.array_equal(x, y) for x, y in zip(*outs))
            # an observed factor decides its half of the option: an exactly observed degree is the drawn one
            dom = lw.latent_dom[("Doc", "degree")]
            for i in range(n):
                if S["dirty"]["Degree"][i] in S["A"]:
                    assert dom.string(int(outs[0][2][i, 1]) // nb) == S["dirty"]["Degree"][i], i
            # the log-weight is the new row's prior mass plus the leaf's marginal: the same for every particle
            assert np.allclose(logml, lse + (logml[0] - lse[0]), rtol=0, atol=1e-9)
    finally:
        eng.close()
