"""Own blocks on the device: pclean_sweep_own / pclean_score_own / pclean_own_counts against the existing leaf path, the
particle rule of pclean_final_choice, exact conditionals from the literal interpreter, and end to end.

1  parity      pclean_score_own == pclean_score_node on the TWIN's new-row leaf (the same choice behind a slot: what the code
               computed for these rows before own blocks existed), bit for bit in scores and lse; the draws of both are
               recomputed from the scores with Python integers and pclean_debug_rand64 (the two leaves have different
               draw sites).  K below, at and above the LDS-resident limit: both kernel variants.
2  windows     one sweep over all rows == the same sweep issued as windows of 1, 64, 65 rows and the rest.
3  particles   the chosen particle is pclean_final_choice's on equal weights; particle 0 keeps every value of the row.
4  exact       S sweeps from one frozen state against posterior_exact's closed forms; pi from oracle/literal.py.
5  counts      pclean_own_counts == bincount of the values.
6  recovery    planted rows whose exact pi is a point mass come back as the truth from initialize_trace + run_inference.
7  end to end  1 000 hospital rows, three columns: the device runs' mean accuracy against a NumPy sequential restatement.
8  refusals    the C ABI refuses what it does not serve and leaves the loaded plan as it was."""
import math

import numpy as np
import pytest

import own_choice_program as ocp
import posterior_exact as pe
from pclean_amd import _lib
from pclean_amd import experiments as ex
from pclean_amd import inference as inf
from pclean_amd.analysis import reconstructed_table
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.model import LoweredModel
from pclean_amd.trace import Trace

pytestmark = pytest.mark.gpu

LIMIT = 4096  # own_block.hip: OWN_LDS_OPTIONS (pclean_own_stats.lds_options says so)


def _site(block, node):
    return (block << 16) | node


def _flat_engine(S, params):
    lw, obs = ocp.lower(S)
    eng = Engine(lw, obs, dist_mode=1)
    tr = Trace(lw, S["n_rows"], 0)
    for k, v in params.items():
        tr.params[("Obs", k)].value = np.asarray(v, dtype=np.float64)
    eng.upload_trace(tr)
    return lw, eng, tr


def _twin_engine(T, p):
    lw = LoweredModel(T["model"], T["query"], T["dirty"])
    eng = Engine(lw, lw.encode_observations(T["dirty"]), dist_mode=1)
    tr = Trace(lw, T["n_rows"], 0)
    tr.params[("A", "p")].value = np.asarray(p, dtype=np.float64)
    eng.upload_trace(tr)
    return eng


def _draws_from_scores(hip, scores, rows, seed, site, sweep, n_draws):
    """min{k : u_0 + .. + u_k > mulhi64(R, U)} per (row, particle) from fp64 scores: u_k by the device's own fixw
    (pclean_debug_detmath), the sums and the 128-bit product in Python integers; -1 where every score is -inf"""
    m = scores.max(axis=1)
    with np.errstate(invalid="ignore"):
        d = scores - m[:, None]
    u = hip.debug_detmath(np.ascontiguousarray(d).ravel())[2].reshape(scores.shape)
    cum = np.cumsum(u, axis=1, dtype=np.uint64)
    out = np.full((len(rows), n_draws), -1, dtype=np.int64)
    for j in range(n_draws):
        R = hip.debug_rand64(seed, np.asarray(rows, dtype=np.uint32), site, j, sweep)
        for t in range(len(rows)):
            U = int(cum[t, -1])
            if U:
                out[t, j] = int(np.searchsorted(cum[t], np.uint64((int(R[t]) * U) >> 64), side="right"))
    return out


def _parity(S, T, p, pname, K, seed=11, sweep=3, n_draws=3):
    lw, eng, _ = _flat_engine(S, {pname: p})
    engt = _twin_engine(T, p)
    try:
        rows = np.arange(S["n_rows"], dtype=np.int32)
        lse_o, sc_o, dr_o = eng.hip.score_own(0, 0, rows, seed=seed, sweep=sweep, n_draws=n_draws, n_cand=K, want_scores=True)
        st = eng.hip.get_own_stats()
        lse_t, sc_t, dr_t = engt.hip.score_node(0, 1, rows, seed=seed, sweep=sweep, n_draws=n_draws, n_cand=K, want_scores=True)
        assert np.array_equal(sc_o.view(np.uint64), sc_t.view(np.uint64)), "scores differ from the twin's leaf"
        assert np.array_equal(lse_o.view(np.uint64), lse_t.view(np.uint64)), "lse differs from the twin's leaf"
        live = np.isfinite(lse_o)
        want_o = _draws_from_scores(eng.hip, sc_o, rows, seed, _site(0, 0), sweep, n_draws)
        want_t = _draws_from_scores(eng.hip, sc_t, rows, seed, _site(0, 1), sweep, n_draws)
        assert np.array_equal(dr_t[live], want_t[live]), "the recomputation does not restate the existing leaf path"
        assert np.array_equal(dr_o[live], want_o[live]), "draws differ from the scores' inverse CDF"
        # a probe of a few rows, out of order and with a row twice, answers as the probe of all rows
        some = np.array([5, 0, S["n_rows"] - 1, 5, 17], dtype=np.int32)
        l2, s2, d2 = eng.hip.score_own(0, 0, some, seed=seed, sweep=sweep, n_draws=n_draws, n_cand=K, want_scores=True)
        assert np.array_equal(l2.view(np.uint64), lse_o[some].view(np.uint64)) and np.array_equal(d2[live[some]], dr_o[some][live[some]])
        assert np.array_equal(s2.view(np.uint64), sc_o[some].view(np.uint64))
        return lw, st, lse_o, live
    finally:
        eng.close()
        engt.close()


@pytest.mark.parametrize("K", [1, 63, 64, 65, 257, LIMIT, LIMIT + 1])
def test_parity_with_the_leaf_path_flat1(K):
    S = ocp.flat1(K=K, seed=K)
    p = np.random.default_rng(K).dirichlet(np.ones(K))
    lw, st, lse, live = _parity(S, ocp.twin1(S), p, "p", K)
    assert st.lds_options == LIMIT
    assert st.variants == (1 if K <= LIMIT else 2), "the other kernel variant ran"
    # the static runs: one per distinct observation (the missing one included), the longest of RUNS rows
    assert st.n_runs == len(set(S["dirty"]["Y"])) and st.longest_run == max(ocp.RUNS)
    lens = sorted(np.unique(lw.obs_host[0], return_counts=True)[1])
    assert set(ocp.RUNS) <= set(lens)
    assert live.all()


def test_parity_with_the_leaf_path_flat3_and_an_impossible_row():
    S = ocp.flat3()
    K = len(S["choices"]["name"])
    p = np.random.default_rng(3).dirichlet(np.ones(K))
    seen = next(i for i in range(S["n_rows"]) if S["dirty"]["Name"][i] is not None)
    dead = S["choices"]["name"].index(S["dirty"]["Name"][seen])
    p[dead] = 0.0  # the directly observed option of row `seen` has no prior mass: every option of that row scores -inf
    p /= p.sum()
    lw, st, lse, live = _parity(S, ocp.twin3(S), p, "p", K)
    assert st.variants == 1 and st.longest_run == max(ocp.RUNS)
    assert not live[seen] and lse[seen] == -math.inf
    assert live.sum() == S["n_rows"] - sum(S["dirty"]["Name"][i] == S["choices"]["name"][dead] for i in range(S["n_rows"]))


# ---- 2: windows -----------------------------------------------------------------------------------------------------
def _start(S, lw, seed, none_from):
    """current values for the rows below none_from (uniform over the options), none for the others"""
    rng = np.random.default_rng(seed)
    tr0 = Trace(lw, S["n_rows"], 0)
    own = np.full((len(tr0.own_leaves()), S["n_rows"]), -1, dtype=np.int32)
    for li, (a, _, _) in enumerate(tr0.own_leaves()):
        own[li, :none_from] = rng.integers(len(S["choices"][a]), size=none_from)
    return own


@pytest.mark.parametrize("prog", ["flat1", "flat2b"])
def test_window_independence(prog):
    S = ocp.flat1(K=70, seed=4) if prog == "flat1" else ocp.flat2b()
    n = S["n_rows"]
    lw, eng, tr = _flat_engine(S, {})
    try:
        start = _start(S, lw, 1, n // 2)
        cfg = InferenceConfig(1, 3)
        tr.own = start.copy()
        chosen, logml = eng.sweep_own(tr, cfg, 21, 5)
        vals = tr.own.copy()
        assert (vals >= 0).all() and (vals[:, :n // 2] != start[:, :n // 2]).any()
        tr.own = start.copy()
        parts = [eng.sweep_own(tr, cfg, 21, 5, lo, hi) for lo, hi in ((0, 1), (1, 65), (65, 130), (130, n))]
        assert np.array_equal(np.concatenate([c for c, _ in parts]), chosen)
        assert np.array_equal(np.concatenate([l for _, l in parts]).view(np.uint64), logml.view(np.uint64))
        assert np.array_equal(tr.own, vals)
        # a window leaves the rows outside it alone
        tr.own = start.copy()
        eng.sweep_own(tr, cfg, 21, 5, 65, 130)
        after = tr.own
        assert np.array_equal(after[:, :65], start[:, :65]) and np.array_equal(after[:, 130:], start[:, 130:])
        assert np.array_equal(after[:, 65:130], vals[:, 65:130])
        tr.check_consistency()
    finally:
        eng.close()


# ---- 3: the chosen particle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,mh", [(1, False), (2, False), (2, True), (3, False), (33, False), (64, False)],
                         ids=["P1", "P2-PG", "P2-MH", "P3", "P33", "P64"])
def test_chosen_particle_is_final_choice_on_equal_weights(P, mh):
    S = ocp.flat2b()
    n = S["n_rows"]
    lw, eng, tr = _flat_engine(S, {})
    try:
        start = _start(S, lw, 2, n // 2)
        tr.own = start.copy()
        cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
        seed, sweep = 77 + P, 9
        chosen, logml = eng.sweep_own(tr, cfg, seed, sweep)
        vals = tr.own
        w = np.zeros((n, P))
        with_cur, _ = eng.hip.final_choice(w, mh, 1, seed, sweep)
        without, _ = eng.hip.final_choice(w, mh, 0, seed, sweep)
        want = np.where(np.arange(n) < n // 2, with_cur, without)
        assert np.array_equal(chosen, want)
        if P > 1:
            assert len(set(chosen.tolist())) > 1
        kept = (np.arange(n) < n // 2) & (chosen == 0)
        if mh:  # accepted with 0.5 / (1e-10 + 0.5): the proposal, in every row that has values
            assert (chosen[:n // 2] == 1).all()
        else:
            assert kept.any()
        assert np.array_equal(vals[:, kept], start[:, kept]), "a row that chose particle 0 lost a value (some block's)"
        if P == 1:
            assert kept[:n // 2].all()
        assert (vals[:, n // 2:] >= 0).all(), "a row without values did not draw"
        moved = (np.arange(n) < n // 2) & (chosen != 0)
        if moved.any():  # the chosen particle names the draw: the probe's draw `chosen` of every leaf
            for li, (a, b, nd) in enumerate(tr.own_leaves()):
                rows = np.nonzero(moved)[0].astype(np.int32)
                _, _, dr = eng.hip.score_own(b, nd, rows, seed=seed, sweep=sweep, n_draws=P)
                assert np.array_equal(dr[np.arange(len(rows)), chosen[rows]], vals[li, rows])
        assert np.isfinite(logml).all()
    finally:
        eng.close()


# ---- 4: exact distribution ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dist():
    S, params, scores, pis, cur = ocp.dist_case()
    lw, eng, tr = _flat_engine(S, params)
    try:
        yield S, scores, pis, cur, eng
    finally:
        eng.close()


def _sweeps(eng, S, cur_idx, P, mh, n_sweeps, seed):
    n = S["n_rows"]
    hip = eng.hip
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh).as_c()
    hip.set_active_rows(0, n)
    draws = np.empty((n_sweeps, n), dtype=np.int32)
    first = None
    for s in range(n_sweeps):  # nothing is committed: every sweep starts from the same values
        hip.set_own(0, cur_idx[None, :])
        _, logml = hip.sweep_own(cfg, seed, s, n)
        draws[s] = hip.get_own(0, 1, n)[0]
        if s == 0:
            first = logml
    return draws, first


def _items(S, expected, draws):
    names = S["choices"]["name"]
    items = []
    for i, e in enumerate(expected):
        cnt = np.bincount(draws[:, i], minlength=len(names))
        items.append((i, e, {names[k]: int(c) for k, c in enumerate(cnt) if c}))
    return items


@pytest.mark.parametrize("P,mh", pe.TAB_PARTICLES, ids=[f"P{p}{'-MH' if m else ''}" for p, m in pe.TAB_PARTICLES])
def test_values_follow_the_exact_conditional(dist, P, mh):
    S, scores, pis, cur, eng = dist
    names = S["choices"]["name"]
    cur_idx = np.array([names.index(s) for s in cur], dtype=np.int32)
    draws, logml = _sweeps(eng, S, cur_idx, P, mh, pe.S_GPU, seed=9100 + P)
    res = pe.gof(_items(S, [ocp.expected_output(pi, s, P, mh) for pi, s in zip(pis, cur)], draws))
    dev = max(abs(logml[i] - pe.log_marginal(scores[i])) / pe.logml_bound(len(names), pe.log_marginal(scores[i]))
              for i in range(S["n_rows"]))
    print(f"\n[own P={P}{' MH' if mh else ''}] {pe.describe(res)}; logml deviation {dev:.3f} of its bound")
    assert res["p"] > pe.ALPHA, pe.describe(res)
    assert dev <= 1.0
    if P == 1:
        assert (draws == cur_idx[None, :]).all()


def test_values_without_current_values_follow_pi(dist):
    S, scores, pis, _, eng = dist
    none = np.full(S["n_rows"], -1, dtype=np.int32)
    for P, mh in ((1, False), (2, True), (9, False)):
        draws, _ = _sweeps(eng, S, none, P, mh, pe.S_GPU, seed=9200 + P)
        res = pe.gof(_items(S, pis, draws))
        print(f"\n[own, no current values, P={P}{' MH' if mh else ''}] {pe.describe(res)}")
        assert res["p"] > pe.ALPHA, pe.describe(res)


# ---- 5: counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog", ["flat2b", "flat1-beyond-lds"])
def test_counts_equal_bincount(prog):
    S = ocp.flat2b() if prog == "flat2b" else ocp.flat1(K=LIMIT + 1, seed=8)
    lw, eng, tr = _flat_engine(S, {})
    try:
        cfg = InferenceConfig(1, 4)
        for s in range(3):
            eng.sweep_own(tr, cfg, 5, s)
        for li, (a, b, nd) in enumerate(tr.own_leaves()):
            K = len(S["choices"][a])
            cnt = eng.hip.own_counts(b, nd, K)
            vals = eng.hip.get_own(b, len([1 for _, bb, _ in tr.own_leaves() if bb == b]), S["n_rows"])[nd]
            assert np.array_equal(cnt, np.bincount(vals, minlength=K)) and cnt.sum() == S["n_rows"]
            assert np.array_equal(tr.own[li], vals)
        tr.check_consistency()
    finally:
        eng.close()


# ---- 6: planted recovery ----------------------------------------------------------------------------------------------
def test_planted_rows_are_recovered():
    S = ocp.flat2b(planted=True, seed=6)
    n = S["n_rows"]
    cols = {"city": "City", "state": "State", "cond": "Cond"}
    # first, from the exact conditional: under a uniform prior the true option holds all but 1e-12 of the mass, and no
    # other option comes within 40 nats of it — a prior ratio of e^12 (no Dirichlet draw of these sizes comes near) leaves
    # less than e^-28 elsewhere
    for choice, col in cols.items():
        K = len(S["choices"][choice])
        uniform = {ocp.param_of(S, choice): np.full(K, 1.0 / K)} if ocp.param_of(S, choice) else {}
        for i in range(n):
            sc = ocp.exact_scores(S, uniform, choice, i)
            t = S["truth"][col][i]
            assert pe.normalise(sc).get(t, 0.0) >= 1.0 - 1e-12
            assert sc[t] - max(v for o, v in sc.items() if o != t) >= 40.0
    lw, obs = ocp.lower(S)
    eng = Engine(lw, obs, dist_mode=1)
    try:
        tr = Trace(lw, n, 6)
        cfg = InferenceConfig(5, 4, rejuv_frequency=50)
        inf.initialize_trace(eng, tr, cfg, 6)
        assert (tr.own >= 0).all()
        inf.run_inference(eng, tr, cfg, 6)
        tab = reconstructed_table(lw, tr, S["dirty"])
        for col in cols.values():
            assert tab[col] == S["truth"][col], col
        tr.check_consistency()
    finally:
        eng.close()


# ---- 7: end to end ------------------------------------------------------------------------------------------------------
def test_hospital_columns_against_the_sequential_restatement(capsys):
    n, iters, P = 1000, 5, 4
    dirty, clean = ex.hospital_data()
    dirty = {c: dirty[c][:n] for c in ex.FLAT_COLUMNS}
    clean = {c: clean[c][:n] for c in ex.FLAT_COLUMNS}
    vocab = ex.flat_vocabulary(clean)
    m = ex.flat_model(vocab)
    lw = LoweredModel(m, ex.flat_query(m), dirty)
    obs = lw.encode_observations(dirty)
    got, want = [], []
    for seed in range(6):
        eng = Engine(lw, obs, dist_mode=1)
        try:
            tr = Trace(lw, n, seed)
            cfg = InferenceConfig(iters, P, rejuv_frequency=50)
            inf.initialize_trace(eng, tr, cfg, seed)
            inf.run_inference(eng, tr, cfg, seed)
            tr.check_consistency()
            got.append(ex.cell_accuracy(reconstructed_table(lw, tr, dirty), clean))
        finally:
            eng.close()
        want.append(ocp.sequential_flat(vocab, dirty, clean, iters, P, seed, rejuv=50))
    d = np.asarray(got) - np.asarray(want)
    se = d.std(ddof=1) / np.sqrt(len(d))
    with capsys.disabled():
        print(f"\n[flat hospital columns, {n} rows] device {np.round(got, 4).tolist()} (mean {np.mean(got):.4f})  sequential "
              f"restatement {np.round(want, 4).tolist()} (mean {np.mean(want):.4f}); dirty {ex.cell_accuracy(dirty, clean):.4f}; "
              f"difference {100 * d.mean():+.2f} pt (paired s.e. {100 * se:.2f} pt)")
    assert abs(d.mean()) <= 2 * se + 0.005, (d.mean(), se, got, want)


# ---- 8: what the C ABI refuses ----------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_plan_alone():
    S = ocp.flat3()
    lw, eng, tr = _flat_engine(S, {})
    try:
        cfg = InferenceConfig(1, 3)
        tr.own = _start(S, lw, 3, S["n_rows"] // 2)
        start = tr.own.copy()
        chosen, logml = eng.sweep_own(tr, cfg, 31, 2)
        vals = tr.own.copy()
        nodes, terms = lw.own_block_arrays(0)

        def refused(nodes_, terms_, what):
            with pytest.raises(_lib.PCleanHipError, match=what):
                eng.hip.load_own_block(0, nodes_, terms_)

        t = terms.copy()
        t["ctx_slot"][1], t["fn_table"][1] = 0, 0
        refused(nodes, t, "term 1 has a ctx slot")
        t = terms.copy()
        t["dens_kind"][2] = _lib.DENS_NAME3
        refused(nodes, t, "term 2 is a name3 term")
        nd = nodes.copy()
        nd["dummy_value"][0] = 1
        refused(nd, terms, "node 0 has a dummy value")
        nd = nodes.copy()
        nd["kind"][0] = _lib.NODE_FK
        refused(nd, terms, "node 0 is not a leaf")
        bad = InferenceConfig(1, 3, use_dd_proposals=False).as_c()
        eng.hip.set_active_rows(0, S["n_rows"])
        with pytest.raises(_lib.PCleanHipError, match="use_dd_proposals = 0"):
            eng.hip.sweep_own(bad, 31, 2, S["n_rows"])
        # the loaded plan and the values are what they were: the same sweep from the same start gives the same bits
        assert np.array_equal(eng.hip.get_own(0, 1, S["n_rows"]), vals)
        tr.own = start
        chosen2, logml2 = eng.sweep_own(tr, cfg, 31, 2)
        assert np.array_equal(chosen2, chosen) and np.array_equal(logml2.view(np.uint64), logml.view(np.uint64))
        assert np.array_equal(tr.own, vals)
    finally:
        eng.close()


def test_a_row_without_a_possible_option_is_named():
    S = ocp.flat3()
    K = len(S["choices"]["name"])
    seen = [i for i in range(S["n_rows"]) if S["dirty"]["Name"][i] is not None]
    p = np.ones(K)
    p[S["choices"]["name"].index(S["dirty"]["Name"][seen[0]])] = 0.0
    lw, eng, tr = _flat_engine(S, {"p": p / p.sum()})
    try:
        first = min(i for i in seen if S["dirty"]["Name"][i] == S["dirty"]["Name"][seen[0]])
        with pytest.raises(ValueError, match=rf"row {first}: none of the options of an own choice is possible"):
            eng.sweep_own(tr, InferenceConfig(1, 2), 1, 0)
    finally:
        eng.close()
