"""Several dependents on one index, enumerated collapsed, on the device: own_star_kernel (csrc/own_block.hip).

1  parity        pclean_score_own of the head and of every arm (scores, lse, draws for three particle ids) == the contract
                 restated in NumPy on the device's scores (own_star_program.definition), bit for bit; the scores against the
                 factors restated from oracle/literal.py's densities.
2  sweeps        windows, their order and the cut of a long run change nothing; pclean_own_counts of the head and of the arms
                 == the host's histograms; a kept row is untouched in every node; an impossible row is named.
3  skip          three rows against a fresh child process that weighs every index value (PCLEAN_NO_OWN_SKIP=1).
4  distribution  swept triples follow the exact joint conditional.
5  planted       two dependents that are functions of the index are recovered where their observations are missing.
6  marginals     the head's top values and every arm's conditional top values == the definition on the scores."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import own_choice_program as ocp
import own_marginal_program as omp
import own_star_program as osp
import posterior_exact as pe
from pclean_amd import inference as inf
from pclean_amd.analysis import evaluate_map_accuracy, map_table
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.trace import Trace

pytestmark = pytest.mark.gpu

STAR = 16  # pclean_own_stats.variants
SHAPES = [(1, (1, 1)), (1, (65, 2)), (65, (1, 1)), (3, (4, 2)), (2, (63, 65)), (64, (64, 64)), (65, (64, 130)), (300, (70, 5, 3)),
          (5, (2, 3, 2, 3))]


def _site(block, node):
    return (block << 16) | node


def _engine(S, pa, ths):
    lw, obs = osp.lower(S)
    eng = Engine(lw, obs, dist_mode=1)
    tr = Trace(lw, S["n_rows"], 0)
    tr.params[("Obs", "pa")].value = np.asarray(pa, np.float64)
    for j, th in enumerate(ths):
        tr.params[("Obs", f"theta{j}")].value = np.asarray(th, np.float64)
    eng.upload_trace(tr)
    return lw, eng, tr


def _twin_engine(S, pa):
    lw, obs = osp.head_twin(S)
    eng = Engine(lw, obs, dist_mode=1)
    tr = Trace(lw, S["n_rows"], 0)
    tr.params[("Obs", "pa")].value = np.asarray(pa, np.float64)
    eng.upload_trace(tr)
    return eng


def _tuples(S, per_tuple=3, max_tuples=None):
    """{observed tuple: up to per_tuple of its rows}, in row order"""
    out = {}
    for i in range(S["n_rows"]):
        key = tuple(S["dirty"][c][i] for c in S["dirty"])
        if key not in out and max_tuples is not None and len(out) >= max_tuples:
            continue
        if len(out.setdefault(key, [])) < per_tuple:
            out[key].append(i)
    return out


def _against_exact(S, pa, ths, i, H_dev, t_dev, S_dev):
    """The device's scores of row i against exact_parts.  Bound for H and t_j: _against_definition's of the product leaf
    (tests/test_gpu_own_product.py) — a sum of at most six non-positive doubles, every term the literal's formula through the
    library's fp64 tables, well inside 1e-10 absolute, and at most 8 roundings at the magnitude of the result.  S(a) adds
    L_1 .. L_D: each a fixed-point log-sum-exp with pe.logml_bound(K_j, L_j) = K_j 2^-40 + 1e-12 |L_j| on top of the errors of
    its inputs (a log-sum-exp moves by at most the largest error of an input)."""
    H, T = osp.exact_parts(S, pa, ths, i)
    eps = np.finfo(np.float64).eps
    worst = 0.0
    for got, want in [(H_dev, H)] + [(t, w) for t, w in zip(t_dev, T)]:
        assert np.array_equal(np.isneginf(got), np.isneginf(want)), "another set of impossible options"
        fin = np.isfinite(want)
        if fin.any():
            worst = max(worst, float((np.abs(got[fin] - want[fin]) / (1e-10 + 8 * eps * np.abs(want[fin]))).max()))
    want_S, bound = H.copy(), 1e-10 + 8 * eps * np.abs(np.where(np.isfinite(H), H, 0.0))
    for w in T:
        L = np.array([pe.log_marginal(dict(enumerate(row.tolist()))) if np.isfinite(row).any() else -np.inf for row in w])
        want_S = want_S + L
        fin_w = np.where(np.isfinite(w), np.abs(w), 0.0)
        bound = bound + 1e-10 + 8 * eps * fin_w.max(axis=1) + w.shape[1] * 2.0 ** -40 + 1e-12 * np.abs(np.where(np.isfinite(L), L, 0.0))
    assert np.array_equal(np.isneginf(S_dev), np.isneginf(want_S))
    fin = np.isfinite(want_S)
    if fin.any():
        worst = max(worst, float((np.abs(S_dev[fin] - want_S[fin]) / bound[fin]).max()))
    return worst


# ---- 1: parity -----------------------------------------------------------------------------------------------------------
def _parity(S, pa, ths, seed=11, sweep=3, n_draws=3, max_exact=None):
    ka, ks = len(S["A"]), [len(B) for B in S["Bs"]]
    D = len(ks)
    lw, eng, _ = _engine(S, pa, ths)
    twin = _twin_engine(S, pa)
    try:
        assert lw.own_star == {(0, 0): list(range(1, D + 1))}
        tup = _tuples(S)
        rows = np.array(sorted(r for v in tup.values() for r in v), dtype=np.int32)
        pos = {int(r): t for t, r in enumerate(rows)}
        hip = eng.hip
        hip.set_active_rows(0, S["n_rows"])
        twin.hip.set_active_rows(0, S["n_rows"])
        lse_h, S_dev, a_dev = hip.score_own(0, 0, rows, seed=seed, sweep=sweep, n_draws=n_draws, n_cand=ka, want_scores=True)
        st = hip.get_own_stats()
        assert st.variants & STAR and st.star_skipped == 0, "a probe that asks for the head's scores weighs every value"
        lse_2, _, a_2 = hip.score_own(0, 0, rows, seed=seed, sweep=sweep, n_draws=n_draws)  # (with the skip)
        skipped = hip.get_own_stats().star_skipped
        assert np.array_equal(lse_2.view(np.uint64), lse_h.view(np.uint64)) and np.array_equal(a_2, a_dev)
        arms = [hip.score_own(0, 1 + j, rows, seed=seed, sweep=sweep, n_draws=n_draws, n_cand=ka * ks[j], want_scores=True)
                for j in range(D)]
        assert hip.get_own_stats().variants & STAR
        _, H_dev, _ = twin.hip.score_own(0, 0, rows, n_cand=ka, want_scores=True)
        sites = [_site(0, n) for n in range(1 + D)]
        worst, n_exact = 0.0, 0
        for key, members in tup.items():
            t0 = pos[members[0]]
            ts = [arms[j][1][t0].reshape(ka, ks[j]) for j in range(D)]
            want = osp.definition(hip, H_dev[t0], ts, members, seed, sweep, n_draws, sites)
            for r, i in enumerate(members):
                t = pos[i]
                assert np.array_equal(S_dev[t].view(np.uint64), want["S"].view(np.uint64)), f"row {i}: S differs from the definition"
                assert lse_h[t].view(np.uint64) == np.float64(want["lse"]).view(np.uint64), f"row {i}: lse"
                assert np.array_equal(a_dev[t], want["a"][r]), f"row {i}: the head's draws"
                for j in range(D):
                    assert np.array_equal(arms[j][1][t].view(np.uint64), arms[j][1][t0].view(np.uint64))
                    assert np.array_equal(arms[j][2][t], want["b"][j][r]), f"row {i}: arm {j}'s draws"
                    La = want["L"][j][want["a"][r, 0]]
                    assert arms[j][0][t].view(np.uint64) == np.float64(La).view(np.uint64), f"row {i}: arm {j}'s lse"
            if max_exact is None or n_exact < max_exact:
                worst = max(worst, _against_exact(S, pa, ths, members[0], H_dev[t0], ts, S_dev[t0]))
                n_exact += 1
        print(f"\n[star {ka}; {ks}] {len(tup)} tuples, {n_exact} against the literal densities: largest error / bound {worst:.3g}; "
              f"{skipped} index values skipped in the probe without scores")
        assert worst <= 1.0
        assert np.isfinite(lse_h).all()
        # a probe of a few rows, out of order and with a row twice, answers as the probe of all rows
        pick = np.array([5, 0, len(rows) - 1, 5, min(17, len(rows) - 1)])
        for node, ref, K in [(0, (lse_h, S_dev, a_dev), ka)] + [(1 + j, arms[j], ka * ks[j]) for j in range(D)]:
            l2, s2, d2 = hip.score_own(0, node, rows[pick], seed=seed, sweep=sweep, n_draws=n_draws, n_cand=K, want_scores=True)
            assert np.array_equal(l2.view(np.uint64), ref[0][pick].view(np.uint64)) and np.array_equal(d2, ref[2][pick])
            assert np.array_equal(s2.view(np.uint64), ref[1][pick].view(np.uint64))
        return st
    finally:
        eng.close()
        twin.close()


@pytest.mark.parametrize("ka,ks", SHAPES, ids=[f"{a};{','.join(map(str, k))}" for a, k in SHAPES])
def test_parity_with_the_definition(ka, ks):
    S = osp.starp(ka, ks, seed=ka * 1000 + sum(ks))
    pa, ths = osp.draw_params(S, ka + sum(ks))
    st = _parity(S, pa, ths, max_exact=6 if ka * max(ks) > 4000 else 40)
    assert st.longest_run == osp.LONG_RUN


def test_variant_terms_against_the_definition():
    """two terms on the head (one tabulated: it scores a missing observation) and the equality term of a direct observation,
    two terms on arm 0, and an arm without any observation (drawn from theta_j[a])"""
    S = osp.starp(5, (7, 3), seed=3, variant=True, long_run=False)
    pa, ths = osp.draw_params(S, 35)
    _parity(S, pa, ths, max_exact=60)


# ---- 2: sweeps -----------------------------------------------------------------------------------------------------------
def _start(S, seed, none_from):
    rng = np.random.default_rng(seed)
    own = np.full((1 + len(S["Bs"]), S["n_rows"]), -1, dtype=np.int32)
    own[0, :none_from] = rng.integers(len(S["A"]), size=none_from)
    for j, B in enumerate(S["Bs"]):
        own[1 + j, :none_from] = rng.integers(len(B), size=none_from)
    return own


def test_window_and_run_cut_independence_and_counts():
    S = osp.starp(9, (11, 4), seed=4)
    n = S["n_rows"]
    pa, ths = osp.draw_params(S, 4)
    lw, eng, tr = _engine(S, pa, ths)
    try:
        start = _start(S, 1, n // 2)
        cfg = InferenceConfig(1, 3)
        tr.own = start.copy()
        chosen, logml = eng.sweep_own(tr, cfg, 21, 5)
        st = eng.hip.get_own_stats()
        assert st.variants == STAR and st.longest_run == osp.LONG_RUN and st.n_workgroups == st.n_runs + 1  # (the cut run)
        counts = [eng.hip.own_counts(0, 0, 9), eng.hip.own_counts(0, 1, 99), eng.hip.own_counts(0, 2, 36)]
        vals = tr.own.copy()
        assert (vals >= 0).all() and (vals[:, :n // 2] != start[:, :n // 2]).any()
        assert np.array_equal(counts[0], np.bincount(vals[0], minlength=9))
        assert np.array_equal(counts[1], np.bincount(vals[0] * 11 + vals[1], minlength=99))
        assert np.array_equal(counts[2], np.bincount(vals[0] * 4 + vals[2], minlength=36))
        assert np.array_equal(eng.hip.get_own(0, 3, n), vals)
        assert np.array_equal(tr.params[("Obs", "pa")].counts, counts[0])
        assert np.array_equal(tr.params[("Obs", "theta0")].counts, counts[1].reshape(9, 11))
        assert np.array_equal(tr.params[("Obs", "theta1")].counts, counts[2].reshape(9, 4))
        tr.check_consistency()
        # a kept row is untouched in every node
        kept = (start[0] >= 0) & (chosen == 0)
        assert kept.sum() > 20 and np.array_equal(vals[:, kept], start[:, kept])
        # windows, in order and out of order
        for wins in [((0, 1), (1, 65), (65, 130), (130, n)), ((130, n), (0, 1), (65, 130), (1, 65))]:
            tr.own = start.copy()
            parts = {(lo, hi): eng.sweep_own(tr, cfg, 21, 5, lo, hi) for lo, hi in wins}
            assert np.array_equal(np.concatenate([parts[w][0] for w in sorted(parts)]), chosen)
            assert np.array_equal(np.concatenate([parts[w][1] for w in sorted(parts)]).view(np.uint64), logml.view(np.uint64))
            assert np.array_equal(tr.own, vals)
        tr.own = start.copy()
        eng.sweep_own(tr, cfg, 21, 5, 65, 130)
        after = tr.own
        assert np.array_equal(after[:, :65], start[:, :65]) and np.array_equal(after[:, 130:], start[:, 130:])
        assert np.array_equal(after[:, 65:130], vals[:, 65:130])
        # the cut of the long run: its rows share one lse, and every row's values are its own draws from the run's scores
        keys = list(zip(*[S["dirty"][c] for c in S["dirty"]]))
        key = max(set(keys), key=keys.count)
        run = np.array([i for i in range(n) if keys[i] == key], dtype=np.int32)
        assert len(run) == osp.LONG_RUN and len(set(logml[run].view(np.uint64).tolist())) == 1
        rows = np.concatenate([run[:40], run[-40:]])  # (members of both pieces)
        eng.hip.set_active_rows(0, n)
        twin = _twin_engine(S, pa)
        try:
            twin.hip.set_active_rows(0, n)
            _, H, _ = twin.hip.score_own(0, 0, rows[:1], n_cand=9, want_scores=True)
        finally:
            twin.close()
        ts = [eng.hip.score_own(0, 1 + j, rows[:1], n_cand=9 * k, want_scores=True)[1][0].reshape(9, k) for j, k in enumerate((11, 4))]
        want = osp.definition(eng.hip, H[0], ts, rows, 21, 5, 3, [_site(0, 0), _site(0, 1), _site(0, 2)])
        moved = ~((start[0, rows] >= 0) & (chosen[rows] == 0))
        idx = (np.arange(len(rows)), chosen[rows])
        assert moved.sum() > 40 and np.array_equal(vals[0, rows][moved], want["a"][idx][moved])
        for j in range(2):
            assert np.array_equal(vals[1 + j, rows][moved], want["b"][j][idx][moved])
        assert logml[rows[0]].view(np.uint64) == np.float64(want["lse"]).view(np.uint64)
    finally:
        eng.close()


def test_an_impossible_row_is_named():
    S = osp.starp(5, (7, 3), seed=3, variant=True, long_run=False)
    pa, ths = osp.draw_params(S, 35)
    seen = [i for i in range(S["n_rows"]) if S["dirty"]["A"][i] is not None]
    dead = S["A"].index(S["dirty"]["A"][seen[0]])
    pa[dead] = 0.0  # the directly observed index of these rows has no prior mass: every value scores -inf
    lw, eng, tr = _engine(S, pa / pa.sum(), ths)
    try:
        bad = [i for i in seen if S["dirty"]["A"][i] == S["A"][dead]]
        with pytest.raises(ValueError, match=rf"row {min(bad)}: none of the options of an own choice is possible.*\({len(bad)} such rows"):
            eng.sweep_own(tr, InferenceConfig(1, 2), 1, 0)
        vals = eng.hip.get_own(0, 3, S["n_rows"])  # (U == 0: the last option in every node)
        assert (vals[:, bad] == np.array([[4], [6], [2]])).all()
        with pytest.raises(NotImplementedError, match="use_dd_proposals=False"):
            eng.sweep_own(tr, InferenceConfig(1, 2, use_dd_proposals=False), 1, 0)
    finally:
        eng.close()


# ---- 3: the skip ---------------------------------------------------------------------------------------------------------
def test_the_skip_changes_no_bit():
    """`far`, `none` and `loose` of own_star_program.skip_case, and a sweep of all rows, here (with the skip) and in a fresh
    child process that weighs every index value"""
    S, pa, ths, rows = osp.skip_case()
    H, T = osp.exact_parts(S, pa, ths, rows["loose"])
    Sx = H + sum(np.array([pe.log_marginal(dict(enumerate(r.tolist()))) for r in t]) for t in T)
    # the kernel's bound: per arm the largest term sum, the largest prior of the row and log K_j, each maximum on its own
    _, tau = osp.exact_parts(S, pa, [np.ones_like(th) for th in ths], rows["loose"])
    with np.errstate(divide="ignore"):
        bound = H + sum(tj.max(axis=1) + np.log(th).max(axis=1) + np.log(th.shape[1]) for tj, th in zip(tau, ths))
    assert (bound >= Sx).all()
    assert Sx[5] < Sx.max() - 28.5 - 2.0 and bound[5] > Sx.max() - 30.0 + 2.0, "the case is not the one it describes"
    here = osp.run_skip_case()
    env = dict(os.environ, PCLEAN_NO_OWN_SKIP="1")
    child = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "own_star_program.py")], env=env,
                           capture_output=True, text=True, timeout=240)
    assert child.returncode == 0, child.stderr[-2000:]
    there = json.loads(next(ln for ln in child.stdout.splitlines() if ln.startswith("RESULT "))[7:])
    print(f"\n[skip] skipped / weighed here: " + ", ".join(f"{k} {v['skipped']} / {v['weighed']}" for k, v in here.items()))
    assert here["far"]["skipped"] > 0 and here["none"]["skipped"] == 0 and here["far"]["variants"] & STAR
    assert here["loose"]["weighed"] >= 1 and here["sweep"]["skipped"] > 0
    for k, v in there.items():
        assert v["skipped"] == 0, "the child skipped"
        for f in v:
            if f not in ("skipped", "weighed"):
                assert v[f] == here[k][f], f"{k}.{f} differs between the skip and PCLEAN_NO_OWN_SKIP=1"
    # `loose`: index value 5 is weighed and weighs nothing — no draw takes it
    assert all(a != 5 for a in here["loose"]["a"][0])


# ---- 4: exact distribution -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dist():
    S = osp.starp(3, (2, 2), seed=5, long_run=False, runs=(2,))
    pa, ths = osp.draw_params(S, 105)
    rng = np.random.default_rng(106)
    triples = [(a, b, c) for a in S["A"] for b in S["Bs"][0] for c in S["Bs"][1]]
    memo, pis, scores = {}, [], []
    for i in range(S["n_rows"]):
        key = tuple(S["dirty"][c][i] for c in S["dirty"])
        if key not in memo:
            sc = osp.exact_scores(S, pa, ths, i)
            memo[key] = (sc, pe.normalise(sc))
        scores.append(memo[key][0])
        pis.append(memo[key][1])
    cur = np.array([int(rng.choice(12, p=[pis[i].get(t, 0.0) for t in triples])) for i in range(S["n_rows"])], dtype=np.int32)
    lw, eng, tr = _engine(S, pa, ths)
    try:
        yield S, triples, scores, pis, cur, eng
    finally:
        eng.close()


@pytest.mark.parametrize("P,mh", pe.TAB_PARTICLES, ids=[f"P{p}{'-MH' if m else ''}" for p, m in pe.TAB_PARTICLES])
def test_values_follow_the_exact_joint_conditional(dist, P, mh):
    S, triples, scores, pis, cur, eng = dist
    n, hip = S["n_rows"], eng.hip
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh).as_c()
    hip.set_active_rows(0, n)
    start = np.stack([cur // 4, (cur // 2) % 2, cur % 2]).astype(np.int32)
    draws = np.empty((pe.S_GPU, n), dtype=np.int32)
    for s in range(pe.S_GPU):  # nothing is committed: every sweep starts from the same values
        hip.set_own(0, start)
        _, logml = hip.sweep_own(cfg, 9100 + P, s, n)
        v = hip.get_own(0, 3, n)
        draws[s] = v[0] * 4 + v[1] * 2 + v[2]
        if s == 0:
            first = logml
            assert hip.get_own_stats().variants == STAR
    items = []
    for i in range(n):
        cnt = np.bincount(draws[:, i], minlength=12)
        items.append((i, ocp.expected_output(pis[i], triples[cur[i]], P, mh), {triples[k]: int(c) for k, c in enumerate(cnt) if c}))
    res = pe.gof(items)
    dev = max(abs(first[i] - pe.log_marginal(scores[i])) / pe.logml_bound(12, pe.log_marginal(scores[i])) for i in range(n))
    print(f"\n[own star P={P}{' MH' if mh else ''}] {pe.describe(res)}; logml deviation {dev:.3f} of its bound")
    assert res["p"] > pe.ALPHA, pe.describe(res)
    assert dev <= 1.0
    if P == 1:
        assert (draws == cur[None, :]).all()


# ---- 5: a planted dependency ---------------------------------------------------------------------------------------------
def test_a_planted_dependency_repairs_the_missing_cells():
    """b_0 = f_0(a), b_1 = f_1(a), |B_0| = 4, |B_1| = 5, 60 rows per a: 54 observe everything (clean or with one typo), 6 observe
    a clean and lack b_0's observation (two of them), b_1's (two) or both (two): 56 rows of every a observe b_j, 4 do not.

    Why another outcome is negligible.  The words have 14-17 letters and lie pairwise far apart: for a row that observes a
    string at most one typo from its word, that word leads every other by more than 40 nats, which no prior ratio met here
    (Dirichlet draws on counts of this size differ by a few nats) offsets.  So from the first window on, the rows of every a
    that observe b_j hold (a, f_j(a)): counts_j[a][f_j(a)] >= 56 whatever the 4 others drew, counts_j[a][b'] <= 4 for
    b' != f_j(a).  The head's marginal of a row without an observation of b_j is pa[a] x (a's likelihood) x L_j(a), where L_j is
    a log of a sum of theta_j[a][.] = 1 for every a: a is the observed one by the same 40 nats.  Given a* = a the arm's top b is
    argmax_b theta_j[a][b] with theta_j[a] ~ Dirichlet(1 + counts_j[a]); it is wrong only if theta_j[a][b'] > theta_j[a][f_j(a)]
    for some b', i.e. a Beta(<= 5, >= 57) variable above 1/2: at most P(Bin(61, 1/2) <= 4) < 1e-12 per pair, below 2e-10 over
    the 20 x (3 + 4) pairs (a, b')."""
    S = osp.planted()
    n, hidden = S["n_rows"], S["hidden"]
    assert hidden[0].sum() > 0 and hidden[1].sum() > 0 and (hidden[0] & hidden[1]).sum() > 0 and (hidden[0] ^ hidden[1]).sum() > 0
    for j in range(2):
        assert all(S["dirty"][f"C{j}"][i] is None and S["dirty"]["Ca"][i] == S["truth"]["Ca"][i] for i in np.flatnonzero(hidden[j]))
    lw, obs = osp.lower(S)
    eng = Engine(lw, obs, dist_mode=1)
    try:
        tr = Trace(lw, n, 6)
        cfg = InferenceConfig(3, 4, rejuv_frequency=50)
        inf.initialize_trace(eng, tr, cfg, 6)
        inf.run_inference(eng, tr, cfg, 6)
        assert eng.hip.get_own_stats().variants == STAR
        tr.check_consistency()
        marg = eng.own_marginals(tr, top=1)
        assert set(marg) == {"a", "b0", "b1"}
        got = {"Ca": [S["A"][int(k)] for k in marg["a"][0][0]], "C0": [S["Bs"][0][int(k)] for k in marg["b0"][0][0]],
               "C1": [S["Bs"][1][int(k)] for k in marg["b1"][0][0]]}
        for j in range(2):
            rows = np.flatnonzero(hidden[j])
            assert [got[f"C{j}"][i] for i in rows] == [S["truth"][f"C{j}"][i] for i in rows]
        assert got == S["truth"]
        table, conf = map_table(lw, marg, S["dirty"])
        assert table["C0"] == S["truth"]["C0"] and table["C1"] == S["truth"]["C1"]
        acc = evaluate_map_accuracy(lw, marg, S["dirty"], S["truth"])
        assert acc["f1"] == 1.0 and acc["correctly_imputed"] == acc["imputed"] == int(hidden.sum())
    finally:
        eng.close()


# ---- 6: marginals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ka,ks", [(3, (4, 2)), (65, (64, 70))], ids=["3;4,2", "65;64,70"])
def test_marginals_equal_the_definition_on_the_scores(ka, ks):
    S = osp.starp(ka, ks, seed=8, long_run=False)
    n, D = S["n_rows"], len(ks)
    pa, ths = osp.draw_params(S, 8)
    lw, eng, tr = _engine(S, pa, ths)
    try:
        rows = np.arange(n, dtype=np.int32)
        hip = eng.hip
        hip.set_active_rows(0, n)
        _, Sc, _ = hip.score_own(0, 0, rows, n_cand=ka, want_scores=True)
        ts = [hip.score_own(0, 1 + j, rows, n_cand=ka * ks[j], want_scores=True)[1].reshape(n, ka, ks[j]) for j in range(D)]
        fixw = lambda d: hip.debug_detmath(d)[2]  # noqa: E731
        want_opt, want_prob, u, U = omp.marginal_twin(Sc, fixw, 8)
        tr.own = _start(S, 2, n // 2)
        own = tr.own.copy()
        counts = [p.counts.copy() for p in tr.params.values()]
        a_star = want_opt[0]
        at = [ts_j[np.arange(n), np.maximum(a_star, 0)] for ts_j in ts]  # [D] of [n][kj]: t_j(a*, .)
        arm_want = [omp.marginal_twin(at[j], fixw, 8) for j in range(D)]
        for top in (1, 8):
            marg = eng.own_marginals(tr, top=top)
            oa, pr, pc = marg["a"]
            assert np.array_equal(oa, want_opt[:top]), "the head's options differ from the definition"
            assert np.array_equal(pr.view(np.uint64), want_prob[:top].view(np.uint64))
            assert np.array_equal(pc, omp.current_twin(u, U, own[0]))
            assert (pr[oa < 0] == 0.0).all()
            for j in range(D):
                ob, pb, cb = marg[f"b{j}"]
                wo, wp, uj, Uj = arm_want[j]
                assert np.array_equal(ob, wo[:top]), f"arm {j}: options differ from the definition"
                assert np.array_equal(pb.view(np.uint64), wp[:top].view(np.uint64))
                assert np.array_equal(cb, omp.current_twin(uj, Uj, own[1 + j]))
        assert np.array_equal(tr.own, own), "own_marginals wrote a value"
        assert all(np.array_equal(p.counts, c) for p, c in zip(tr.params.values(), counts)), "a count moved"
    finally:
        eng.close()
