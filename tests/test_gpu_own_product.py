"""An own choice indexed by a sibling own choice on the device: own_product_kernel (csrc/own_block.hip).

1  parity        pclean_score_own on FLATP == pclean_score_node on the TWIN's new-row product leaf (what the code computed
                 before, through enum_product_kernel / the generic kernels), scores, lse and draws bit for bit; and against
                 the joint conditional restated from oracle/literal.py's densities.  Shapes below, at and across the chunk
                 of 64 options, the grid of OWN_LDS_OPTIONS, a wide grid, and one whose cached values do not fit the LDS.
2  sweeps        windows and the cut of a long run change nothing; pclean_own_counts == bincount of the joint values; a row
                 none of whose pairs is possible is named.
3  distribution  swept values follow the exact joint conditional.
4  planted       a dependency b = f(a) is recovered where b's observation is missing.
5  marginals     the joint top options == the definition on pclean_score_own's scores, decoded per choice."""
import numpy as np
import pytest

import own_choice_program as ocp
import own_marginal_program as omp
import own_product_program as opp
import posterior_exact as pe
from pclean_amd import inference as inf
from pclean_amd.analysis import evaluate_map_accuracy, map_table
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.trace import Trace

pytestmark = pytest.mark.gpu

PRODUCT, CHUNKED = 4, 2  # pclean_own_stats.variants
# own_block.hip: the dynamic LDS of own_product_kernel is 8 bytes per cached term value and per chunk of 64 options (a plan
# beyond OWN_PRODUCT_LDS_MAX = 160 KiB - 512 takes own_leaf_kernel<false>)
LDS_MAX = 160 * 1024 - 512
SHAPES = [(1, 1), (1, 65), (65, 1), (3, 4), (2, 63), (2, 64), (2, 65), (64, 64), (64, 65), (300, 70)]


def _lds_bytes(na, nb, terms_a=1, terms_b=1):
    return 8 * (terms_a * na + terms_b * nb + (na * nb + 63) // 64)


NOFIT = (19840, 2)
assert _lds_bytes(*NOFIT) > LDS_MAX >= _lds_bytes(NOFIT[0] - 200, 2)  # (derived from the layout: just beyond it)


def _site(block, node):
    return (block << 16) | node


def _flat_engine(S, pa, th):
    lw, obs = opp.lower(S)
    eng = Engine(lw, obs, dist_mode=1)
    tr = Trace(lw, S["n_rows"], 0)
    tr.params[("Obs", "pa")].value, tr.params[("Obs", "theta")].value = np.asarray(pa, np.float64), np.asarray(th, np.float64)
    eng.upload_trace(tr)
    return lw, eng, tr


def _twin_engine(S, pa, th):
    lw, obs, leaf = opp.twin(S)
    eng = Engine(lw, obs, dist_mode=1)
    tr = Trace(lw, S["n_rows"], 0)
    tr.params[("Doc", "deg_p")].value, tr.params[("Doc", "theta")].value = np.asarray(pa, np.float64), np.asarray(th, np.float64)
    eng.upload_trace(tr)
    return eng, leaf


def _draws_from_scores(hip, scores, rows, seed, site, sweep, n_draws):
    """min{k : u_0 + .. + u_k > mulhi64(R, U)} per (row, particle) from fp64 scores: u_k by the device's own fixw, the sums
    and the 128-bit product in Python integers; -1 where every score is -inf"""
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


def _probe_rows(S, per_tuple=3, max_tuples=None):
    """up to per_tuple rows of every distinct observed tuple (the grouped probe has members to serve), in row order"""
    seen, rows = {}, []
    for i in range(S["n_rows"]):
        key = tuple(S["dirty"][c][i] for c in S["dirty"])
        if key not in seen and max_tuples is not None and len(seen) >= max_tuples:
            continue
        seen[key] = seen.get(key, 0) + 1
        if seen[key] <= per_tuple:
            rows.append(i)
    return np.array(rows, dtype=np.int32)


def _against_definition(S, pa, th, rows, scores):
    """the device's scores of `rows` against exact_matrix.  Bound: a score is a sum of at most six non-positive doubles (the
    two priors and the terms).  Every term is the literal's formula evaluated through the library's fp64 tables — a few
    dozen roundings of quantities below 10^3 (log-binomials of word lengths) — well inside 1e-10 absolute; the sum itself
    rounds at most 8 times at the magnitude of the result (up to 1e5 per impossible AddTypos term)."""
    want = opp.exact_matrix(S, pa, th, rows)
    assert np.array_equal(np.isneginf(scores), np.isneginf(want)), "another set of impossible pairs"
    fin = np.isfinite(want)
    err = np.abs(scores[fin] - want[fin])
    bound = 1e-10 + 8 * np.finfo(np.float64).eps * np.abs(want[fin])
    print(f"\n[definition] {fin.sum()} finite scores, largest error / bound {float((err / bound).max()):.3g}")
    assert (err <= bound).all()


# ---- 1: parity -----------------------------------------------------------------------------------------------------------
def _parity(na, nb, want_variant, seed=11, sweep=3, n_draws=3, max_def_tuples=None):
    S = opp.flatp(na, nb, seed=na * 1000 + nb)
    K = na * nb
    pa, th = opp.draw_params(S, K)
    lw, eng, _ = _flat_engine(S, pa, th)
    engt, leaf = _twin_engine(S, pa, th)
    try:
        rows = _probe_rows(S)
        eng.hip.set_active_rows(0, S["n_rows"])
        lse_o, sc_o, dr_o = eng.hip.score_own(0, 0, rows, seed=seed, sweep=sweep, n_draws=n_draws, n_cand=K, want_scores=True)
        st = eng.hip.get_own_stats()
        assert st.variants == want_variant, f"variants {st.variants}: another kernel ran"
        lse_t, sc_t, dr_t = engt.hip.score_node(leaf[0], leaf[1], rows, seed=seed, sweep=sweep, n_draws=n_draws, n_cand=K,
                                                want_scores=True)
        assert np.array_equal(sc_o.view(np.uint64), sc_t.view(np.uint64)), "scores differ from the twin's leaf"
        assert np.array_equal(lse_o.view(np.uint64), lse_t.view(np.uint64)), "lse differs from the twin's leaf"
        assert np.isfinite(lse_o).all()
        # the two draw streams differ by the site (block 0 node 0 here, node 1 there): each against its own scores' inverse CDF
        want_o = _draws_from_scores(eng.hip, sc_o, rows, seed, _site(0, 0), sweep, n_draws)
        want_t = _draws_from_scores(eng.hip, sc_t, rows, seed, _site(*leaf), sweep, n_draws)
        assert np.array_equal(dr_t, want_t), "the recomputation does not restate the existing leaf path"
        assert np.array_equal(dr_o, want_o), "draws differ from the scores' inverse CDF"
        # a probe of a few rows, out of order and with a row twice, answers as the probe of all rows
        pick = np.array([5, 0, len(rows) - 1, 5, 17])
        l2, s2, d2 = eng.hip.score_own(0, 0, rows[pick], seed=seed, sweep=sweep, n_draws=n_draws, n_cand=K, want_scores=True)
        assert np.array_equal(l2.view(np.uint64), lse_o[pick].view(np.uint64)) and np.array_equal(d2, dr_o[pick])
        assert np.array_equal(s2.view(np.uint64), sc_o[pick].view(np.uint64))
        sub = _probe_rows(S, 1, max_def_tuples)
        pos = {int(r): t for t, r in enumerate(rows)}
        _against_definition(S, pa, th, sub, sc_o[[pos[int(r)] for r in sub]])
        return S, st
    finally:
        eng.close()
        engt.close()


@pytest.mark.parametrize("na,nb", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_parity_with_the_twin_and_the_definition(na, nb):
    # (a grid needs two values of both factors: pclean_set_options_cols' grid test; the others are plain option lists)
    want = PRODUCT if na >= 2 and nb >= 2 else 1
    S, st = _parity(na, nb, want, max_def_tuples=12 if na * nb > 5000 else None)
    assert st.longest_run == opp.LONG_RUN


def test_a_plan_beyond_the_lds_takes_the_chunked_kernel():
    """19 840 x 2: 8 (19 840 + 2 + 620) bytes of cached values and chunk sums exceed OWN_PRODUCT_LDS_MAX"""
    _parity(*NOFIT, CHUNKED, max_def_tuples=2)


def test_variant_terms_against_the_definition():
    """two terms per factor, a tabulated term (it scores a missing observation) and the equality term of a direct observation"""
    S = opp.flatp(5, 7, seed=3, variant=True)
    pa, th = opp.draw_params(S, 35)
    lw, eng, _ = _flat_engine(S, pa, th)
    try:
        rows = _probe_rows(S, 2)
        eng.hip.set_active_rows(0, S["n_rows"])
        lse, sc, dr = eng.hip.score_own(0, 0, rows, seed=5, sweep=1, n_draws=2, n_cand=35, want_scores=True)
        assert eng.hip.get_own_stats().variants == PRODUCT
        _against_definition(S, pa, th, rows, sc)
        assert np.isneginf(sc).any() and np.isfinite(lse).all()
        assert np.array_equal(dr, _draws_from_scores(eng.hip, sc, rows, 5, _site(0, 0), 1, 2))
        for t, i in enumerate(rows):
            z = pe.log_marginal(dict(enumerate(sc[t].tolist())))
            assert abs(float(lse[t]) - z) <= pe.logml_bound(35, z)
    finally:
        eng.close()


# ---- 2: sweeps -----------------------------------------------------------------------------------------------------------
def _start(S, seed, none_from):
    rng = np.random.default_rng(seed)
    own = np.full((2, S["n_rows"]), -1, dtype=np.int32)
    own[0, :none_from] = rng.integers(len(S["A"]), size=none_from)
    own[1, :none_from] = rng.integers(len(S["B"]), size=none_from)
    return own


def test_window_and_run_cut_independence_and_counts():
    S = opp.flatp(9, 11, seed=4)
    n, K = S["n_rows"], 99
    pa, th = opp.draw_params(S, 4)
    lw, eng, tr = _flat_engine(S, pa, th)
    try:
        start = _start(S, 1, n // 2)
        cfg = InferenceConfig(1, 3)
        tr.own = start.copy()
        chosen, logml = eng.sweep_own(tr, cfg, 21, 5)
        st = eng.hip.get_own_stats()
        assert st.variants == PRODUCT and st.longest_run == opp.LONG_RUN and st.n_workgroups == st.n_runs + 1  # (the cut run)
        # the counts while the device is ahead: the joint histogram
        joint_counts = eng.hip.own_counts(0, 0, K)
        vals = tr.own.copy()
        assert (vals >= 0).all() and (vals[:, :n // 2] != start[:, :n // 2]).any()
        joint = vals[0] * 11 + vals[1]
        assert np.array_equal(joint_counts, np.bincount(joint, minlength=K)) and joint_counts.sum() == n
        assert np.array_equal(eng.hip.get_own(0, 1, n)[0], joint)
        assert np.array_equal(tr.params[("Obs", "theta")].counts, joint_counts.reshape(9, 11))
        assert np.array_equal(tr.params[("Obs", "pa")].counts, joint_counts.reshape(9, 11).sum(axis=1))
        tr.check_consistency()
        # windows
        tr.own = start.copy()
        parts = [eng.sweep_own(tr, cfg, 21, 5, lo, hi) for lo, hi in ((0, 1), (1, 65), (65, 130), (130, n))]
        assert np.array_equal(np.concatenate([c for c, _ in parts]), chosen)
        assert np.array_equal(np.concatenate([l for _, l in parts]).view(np.uint64), logml.view(np.uint64))
        assert np.array_equal(tr.own, vals)
        tr.own = start.copy()
        eng.sweep_own(tr, cfg, 21, 5, 65, 130)
        after = tr.own
        assert np.array_equal(after[:, :65], start[:, :65]) and np.array_equal(after[:, 130:], start[:, 130:])
        assert np.array_equal(after[:, 65:130], vals[:, 65:130])
        # the cut of the long run: its rows share one lse, and every row's value is its own draw from the run's scores
        key = max(set(zip(S["dirty"]["Degree"], S["dirty"]["Spec"])), key=list(zip(S["dirty"]["Degree"], S["dirty"]["Spec"])).count)
        run = np.array([i for i in range(n) if (S["dirty"]["Degree"][i], S["dirty"]["Spec"][i]) == key], dtype=np.int32)
        assert len(run) == opp.LONG_RUN and len(set(logml[run].view(np.uint64).tolist())) == 1
        rows = np.concatenate([run[:40], run[-40:]])  # (members of both pieces)
        eng.hip.set_active_rows(0, n)
        _, sc, _ = eng.hip.score_own(0, 0, rows[:1], n_cand=K, want_scores=True)
        want = _draws_from_scores(eng.hip, np.repeat(sc, len(rows), axis=0), rows, 21, _site(0, 0), 5, 3)
        moved = ~((start[0, rows] >= 0) & (chosen[rows] == 0))
        assert moved.sum() > 40 and np.array_equal(joint[rows][moved], want[np.arange(len(rows)), chosen[rows]][moved])
        assert np.array_equal(vals[:, rows[~moved]], start[:, rows[~moved]])
    finally:
        eng.close()


def test_a_row_without_a_possible_pair_is_named():
    S = opp.flatp(5, 7, seed=3, variant=True)
    pa, th = opp.draw_params(S, 35)
    seen = [i for i in range(S["n_rows"]) if S["dirty"]["A"][i] is not None]
    dead = S["A"].index(S["dirty"]["A"][seen[0]])
    pa[dead] = 0.0  # the directly observed index of these rows has no prior mass: every pair scores -inf
    lw, eng, tr = _flat_engine(S, pa / pa.sum(), th)
    try:
        first = min(i for i in seen if S["dirty"]["A"][i] == S["A"][dead])
        with pytest.raises(ValueError, match=rf"row {first}: none of the options of an own choice is possible"):
            eng.sweep_own(tr, InferenceConfig(1, 2), 1, 0)
        with pytest.raises(NotImplementedError, match="use_dd_proposals=False"):
            eng.sweep_own(tr, InferenceConfig(1, 2, use_dd_proposals=False), 1, 0)
    finally:
        eng.close()


# ---- 3: exact distribution ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dist():
    S = opp.flatp(3, 4, seed=5, long_run=False)
    pa, th = opp.draw_params(S, 105)
    rng = np.random.default_rng(106)
    pairs = [(a, b) for a in S["A"] for b in S["B"]]
    memo, pis, scores = {}, [], []
    for i in range(S["n_rows"]):
        key = (S["dirty"]["Degree"][i], S["dirty"]["Spec"][i])
        if key not in memo:
            sc = opp.exact_scores(S, pa, th, i)
            memo[key] = (sc, pe.normalise(sc))
        scores.append(memo[key][0])
        pis.append(memo[key][1])
    cur = np.array([int(rng.choice(12, p=[pis[i].get(p, 0.0) for p in pairs])) for i in range(S["n_rows"])], dtype=np.int32)
    lw, eng, tr = _flat_engine(S, pa, th)
    try:
        yield S, pairs, scores, pis, cur, eng
    finally:
        eng.close()


@pytest.mark.parametrize("P,mh", pe.TAB_PARTICLES, ids=[f"P{p}{'-MH' if m else ''}" for p, m in pe.TAB_PARTICLES])
def test_values_follow_the_exact_joint_conditional(dist, P, mh):
    S, pairs, scores, pis, cur, eng = dist
    n, hip = S["n_rows"], eng.hip
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh).as_c()
    hip.set_active_rows(0, n)
    draws = np.empty((pe.S_GPU, n), dtype=np.int32)
    for s in range(pe.S_GPU):  # nothing is committed: every sweep starts from the same values
        hip.set_own(0, cur[None, :])
        _, logml = hip.sweep_own(cfg, 9100 + P, s, n)
        draws[s] = hip.get_own(0, 1, n)[0]
        if s == 0:
            first = logml
            assert hip.get_own_stats().variants == PRODUCT
    items = []
    for i in range(n):
        cnt = np.bincount(draws[:, i], minlength=12)
        items.append((i, ocp.expected_output(pis[i], pairs[cur[i]], P, mh), {pairs[k]: int(c) for k, c in enumerate(cnt) if c}))
    res = pe.gof(items)
    dev = max(abs(first[i] - pe.log_marginal(scores[i])) / pe.logml_bound(12, pe.log_marginal(scores[i])) for i in range(n))
    print(f"\n[own product P={P}{' MH' if mh else ''}] {pe.describe(res)}; logml deviation {dev:.3f} of its bound")
    assert res["p"] > pe.ALPHA, pe.describe(res)
    assert dev <= 1.0
    if P == 1:
        assert (draws == cur[None, :]).all()


# ---- 4: a planted dependency ---------------------------------------------------------------------------------------------------
def test_a_planted_dependency_repairs_the_missing_cell():
    """b = f(a), |B| = 4, 60 rows per a: 54 observe b (clean or with one typo), 6 observe a clean and b not at all.

    Why another outcome is negligible.  The words have 14-17 letters and lie pairwise far apart: for a row that observes a
    string at most one typo from its word, that word leads every other by more than 40 nats, which no prior ratio met here
    (Dirichlet draws on counts of this size differ by a few nats) offsets.  So from the first window on, the 54 observing rows
    of every a hold (a, f(a)), and counts[a][f(a)] >= 54 whatever the 6 others drew: counts[a][b'] <= 6 for b' != f(a).  For a
    row without b's observation the joint conditional is pa[a] theta_a[b] x (a's likelihood): a is the observed one by the
    same 40 nats, and the top pair is (a, argmax_b theta_a[b]) with theta_a ~ Dirichlet(1 + counts[a]).  The top is wrong only
    if theta_a[b'] > theta_a[f(a)] for some b', i.e. a Beta(<= 7, >= 55) variable above 1/2: at most P(Bin(61, 1/2) <= 6)
    < 4e-11 per pair, below 3e-9 over the 60 pairs (a, b')."""
    S = opp.planted()
    n, hidden = S["n_rows"], S["hidden"]
    per_a = {}
    for i in range(n):
        if S["dirty"]["Spec"][i] is not None:
            per_a[S["truth"]["Degree"][i]] = per_a.get(S["truth"]["Degree"][i], 0) + 1
    assert len(per_a) == len(S["A"]) and min(per_a.values()) >= 20 and hidden.sum() == n // 10
    assert all(S["dirty"]["Degree"][i] == S["truth"]["Degree"][i] and S["dirty"]["Spec"][i] is None for i in np.flatnonzero(hidden))
    lw, obs = opp.lower(S)
    eng = Engine(lw, obs, dist_mode=1)
    try:
        tr = Trace(lw, n, 6)
        cfg = InferenceConfig(3, 4, rejuv_frequency=50)
        inf.initialize_trace(eng, tr, cfg, 6)
        inf.run_inference(eng, tr, cfg, 6)
        assert eng.hip.get_own_stats().variants == PRODUCT
        tr.check_consistency()
        marg = eng.own_marginals(tr, top=1)
        assert set(marg) == {"a", "b"}
        got_a = [S["A"][int(k)] for k in marg["a"][0][0]]
        got_b = [S["B"][int(k)] for k in marg["b"][0][0]]
        rows = np.flatnonzero(hidden)
        assert [got_b[i] for i in rows] == [S["truth"]["Spec"][i] for i in rows]
        assert got_a == S["truth"]["Degree"] and got_b == S["truth"]["Spec"]
        # both cells carry the pair's joint probability
        assert np.array_equal(marg["a"][1], marg["b"][1]) and np.array_equal(marg["a"][2], marg["b"][2])
        table, conf = map_table(lw, marg, S["dirty"])
        assert table["Spec"] == S["truth"]["Spec"] and np.array_equal(conf["Spec"], conf["Degree"])
        acc = evaluate_map_accuracy(lw, marg, S["dirty"], S["truth"])
        assert acc["f1"] == 1.0 and acc["correctly_imputed"] == acc["imputed"] == int(hidden.sum())
    finally:
        eng.close()


# ---- 5: the joint top options ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("na,nb", [(3, 4), (64, 65)], ids=["3x4", "64x65"])
def test_joint_top_options_equal_the_definition_on_the_scores(na, nb):
    S = opp.flatp(na, nb, seed=8, long_run=False)
    n, K = S["n_rows"], na * nb
    pa, th = opp.draw_params(S, 8)
    lw, eng, tr = _flat_engine(S, pa, th)
    try:
        rows = np.arange(n, dtype=np.int32)
        eng.hip.set_active_rows(0, n)
        _, scores, _ = eng.hip.score_own(0, 0, rows, n_cand=K, want_scores=True)
        fixw = lambda d: eng.hip.debug_detmath(d)[2]  # noqa: E731
        want_opt, want_prob, u, U = omp.marginal_twin(scores, fixw, 8)
        tr.own = _start(S, 2, n // 2)
        cur = tr.own[0] * nb + tr.own[1]
        for top in (1, 3, 8):
            marg = eng.own_marginals(tr, top=top)
            oa, pr, pc = marg["a"]
            ob, pr_b, pc_b = marg["b"]
            assert np.array_equal(np.where(oa < 0, -1, oa * nb + ob), want_opt[:top]), "options differ from the definition"
            assert np.array_equal(pr.view(np.uint64), want_prob[:top].view(np.uint64)) and np.array_equal(pr, pr_b)
            assert np.array_equal(pc, omp.current_twin(u, U, np.where(tr.own[0] < 0, -1, cur))) and np.array_equal(pc, pc_b)
            assert ((oa < 0) == (ob < 0)).all()
    finally:
        eng.close()
