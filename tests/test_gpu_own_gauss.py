"""Gaussian observations in an own block on the device: own_gauss_kernel behind pclean_score_own / pclean_sweep_own /
pclean_own_marginals, and pclean_own_gauss_stats.

1  scores      pclean_score_own against the float64 restatement of the conditional (own_gauss_program.exact_scores, from
               oracle/literal.py's densities), within 1e-12 (1 + sum |terms|), over grids from 1 x 1 to 1024 x 4 and 4095 x 1
2  bit for bit m, u_k, U, lse, the draws and the top options with their probabilities recomputed from the DEVICE'S OWN
               scores in Python integers (pclean_debug_detmath / pclean_debug_rand64); exact ties among the weights
3  launch      one sweep == the same sweep in windows; a run of 2 049 rows is cut; a probe out of order and with a repeat
4  particles   particle 0 keeps every value; a row whose options all score -inf takes the last one and is counted
5  statistics  pclean_own_gauss_stats == the NumPy integers; the two routes of Trace.resample_parameters leave the same bits
6  exact       sweeps from a frozen state against the exact joint conditional (posterior_exact.gof), PG and MH
7  recovery    planted wrong units come back
8  refusals    the C ABI refuses what it does not serve and leaves the loaded plan as it was"""
import math

import numpy as np
import pytest

import own_choice_program as ocp
import own_gauss_program as ogp
import posterior_exact as pe
from pclean_amd import _lib
from pclean_amd import inference as inf
from pclean_amd.analysis import evaluate_accuracy, map_table, reconstructed_table
from pclean_amd.engine import Engine, InferenceConfig, make_gauss
from pclean_amd.trace import Trace

pytestmark = pytest.mark.gpu

TWO_M40 = 9.094947017729282379150390625e-13  # 2^-40 (include/pclean_detmath.h: pclean_lse_from_fix)
SITE = (0 << 16) | 0  # PCLEAN_SITE_NODE(block 0, node 0)


def _engine(S, params=True):
    lw, obs = ogp.lower(S)
    eng = Engine(lw, obs, dist_mode=1)
    tr = Trace(lw, S["n_rows"], 0)
    if params:
        ogp.set_params(S, tr)
    eng.upload_trace(tr)
    return lw, eng, tr


def _recompute(hip, scores, rows, seed, sweep, n_draws, top):
    """(lse, draws, top options, top probabilities) from fp64 scores: u_k by the device's own fixw and log
    (pclean_debug_detmath), every sum and the 128-bit product in Python integers"""
    n, K = scores.shape
    m = scores.max(axis=1)
    with np.errstate(invalid="ignore"):
        d = np.where(np.isneginf(m)[:, None], -np.inf, scores - m[:, None])
    u = hip.debug_detmath(np.ascontiguousarray(d).ravel())[2].reshape(scores.shape)
    U = [sum(int(v) for v in row) for row in u]
    logs = hip.debug_detmath(np.array([float(x) * TWO_M40 if x else 1.0 for x in U]))[1]
    lse = np.array([m[t] + logs[t] if U[t] else -math.inf for t in range(n)])
    draws = np.full((n, n_draws), K - 1, dtype=np.int64)
    for j in range(n_draws):
        R = hip.debug_rand64(seed, np.asarray(rows, dtype=np.uint32), SITE, j, sweep)
        for t in range(n):
            if U[t]:
                x, acc = (int(R[t]) * U[t]) >> 64, 0
                for k in range(K):
                    acc += int(u[t, k])
                    if acc > x:
                        draws[t, j] = k
                        break
    top_k = np.full((top, n), -1, dtype=np.int64)
    top_p = np.zeros((top, n))
    for t in range(n):
        order = sorted((k for k in range(K) if u[t, k] > 0), key=lambda k: (-int(u[t, k]), k))[:top]
        for r, k in enumerate(order):
            top_k[r, t] = k
            top_p[r, t] = float(int(u[t, k])) / float(U[t])
    return lse, draws, top_k, top_p, u


GRIDS = [  # (na, nb, extras): the grids of the issue; the mixtures (missing numbers / strings, rows without anything) are in all
    (1, 1, {}), (1, 2, {}), (2, 1, {}), (3, 4, dict(nonlinear=True, second="room")),
    (31, 2, {}), (32, 2, dict(second="const")), (33, 2, dict(nonlinear=True)),
    (1024, 4, dict(nonlinear=True, pool=6, n_rows=300)), (4095, 1, dict(second="room", pool=6, n_rows=300)),
    (0, 2, {}), (3, 0, dict(direct=True, second="room")),
]


@pytest.mark.parametrize("na,nb,extra", GRIDS, ids=[f"{a}x{b}" for a, b, _ in GRIDS])
def test_scores_lse_draws_and_marginals(na, nb, extra):
    S = ogp.gauss_case(na, nb, seed=na + nb, **extra)
    n, K = S["n_rows"], S["K"]
    lw, eng, tr = _engine(S)
    try:
        hip = eng.hip
        rows = np.arange(n, dtype=np.int32)
        seed, sweep, n_draws, top = 31 + na, 4, 2, min(8, 5)
        lse, scores, draws = hip.score_own(0, 0, rows, seed=seed, sweep=sweep, n_draws=n_draws, n_cand=K, want_scores=True)
        assert hip.get_own_stats().variants == 8, "the Gaussian kernel did not run"
        # 1: against the float64 restatement
        worst = 0.0
        for i in range(n):
            want, mag = ogp.exact_scores(S, i)
            assert np.array_equal(np.isneginf(want), np.isneginf(scores[i])), f"row {i}: -inf pattern"
            ok = np.isfinite(want)
            err = np.abs(scores[i][ok] - want[ok]) / (1.0 + mag[ok])
            worst = max(worst, float(err.max(initial=0.0)))
        print(f"\n[{na}x{nb}] largest score deviation {worst:.3g} of 1 + sum |terms| (bound 1e-12)")
        assert worst <= 1e-12
        # 2: bit for bit from the device's own scores
        # (the Python integer sums of a large grid: a sample of the rows, at an odd stride so that it meets every kind of row)
        sub = rows if K <= 70 else rows[:: max(1, n // 24) | 1]
        w_lse, w_draws, w_k, w_p, u = _recompute(hip, scores[sub], sub, seed, sweep, n_draws, top)
        assert np.array_equal(lse[sub].view(np.uint64), w_lse.view(np.uint64)), "lse"
        assert np.array_equal(draws[sub], w_draws), "draws"
        tr.own = np.full((len(tr.own_leaves()), n), -1, dtype=np.int32)
        marg = eng.own_marginals(tr, top=top)
        assert eng.hip.get_own_stats().variants == 8
        names = [a for a, _, _ in tr.own_leaves()]
        opt = marg[names[-1]][0] if len(names) == 1 else tr.own_joint(np.stack([marg[a][0].reshape(-1) for a in names]), 0, 1).reshape(top, n)
        assert np.array_equal(opt[:, sub], w_k), "top options"
        assert np.array_equal(marg[names[-1]][1][:, sub].view(np.uint64), w_p.view(np.uint64)), "top probabilities"
        if nb >= 2:  # a missing number ties the units of every room: equal weights go to the smaller index
            ties = [t for t in range(len(sub)) if S["dirty"]["Rent"][sub[t]] is None and u[t, w_k[0, t]] == u[t, w_k[1, t]]]
            assert ties and all(w_k[0, t] < w_k[1, t] for t in ties)
    finally:
        eng.close()


def test_launch_shape_does_not_matter():
    S = ogp.gauss_case(3, 2, n_rows=2300, seed=5, long_run=2049, second="room")
    n, K = S["n_rows"], S["K"]
    lw, eng, tr = _engine(S)
    try:
        rng = np.random.default_rng(2)
        start = np.stack([rng.integers(0, 3, n), rng.integers(0, 2, n)]).astype(np.int32)
        start[:, n // 2:] = -1
        cfg = InferenceConfig(1, 3)
        tr.own = start.copy()
        chosen, logml = eng.sweep_own(tr, cfg, 21, 5)
        st = eng.hip.get_own_stats()
        assert st.variants == 8 and st.longest_run >= 2049 and st.n_workgroups > st.n_runs, "the long run was not cut"
        vals = tr.own.copy()
        assert (vals >= 0).all()
        tr.own = start.copy()
        cuts = (0, 1, 64, 128, 193, n)  # windows of 1, 63, 64, 65 rows and the rest
        parts = [eng.sweep_own(tr, cfg, 21, 5, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(np.concatenate([c for c, _ in parts]), chosen)
        assert np.array_equal(np.concatenate([l for _, l in parts]).view(np.uint64), logml.view(np.uint64))
        assert np.array_equal(tr.own, vals)
        # particle 0 keeps every value; every other row holds the probe's draw of its chosen particle
        kept = (start[0] >= 0) & (chosen == 0)
        assert kept.any() and np.array_equal(vals[:, kept], start[:, kept])
        rows = np.arange(n, dtype=np.int32)
        eng.hip.set_active_rows(0, n)  # (the last window is still the active one)
        lse, _, draws = eng.hip.score_own(0, 0, rows, seed=21, sweep=5, n_draws=3, n_cand=K)
        assert np.array_equal(lse.view(np.uint64), logml.view(np.uint64))
        joint = tr.own_joint(vals, 0, 1)
        assert np.array_equal(joint[~kept], draws[np.arange(n), chosen][~kept])
        # a probe of a few rows, out of order and with a repeat
        some = np.array([2100, 0, n - 1, 2100, 17, 2048, 2049], dtype=np.int32)
        l2, _, d2 = eng.hip.score_own(0, 0, some, seed=21, sweep=5, n_draws=3, n_cand=K)
        assert np.array_equal(l2.view(np.uint64), lse[some].view(np.uint64)) and np.array_equal(d2, draws[some])
        tr.check_consistency()
    finally:
        eng.close()


def test_an_impossible_row_takes_the_last_option_and_is_counted():
    S = ogp.gauss_case(3, 2, n_rows=60, seed=6, direct=True)
    n = S["n_rows"]
    seen = next(i for i in range(n) if S["dirty"]["Room"][i] is not None)
    dead = S["rooms"].index(S["dirty"]["Room"][seen])
    p = np.array(S["p"])
    p[dead] = 0.0  # the directly observed room of row `seen` has no prior mass: every option of that row scores -inf
    S["p"] = p / p.sum()
    lw, eng, tr = _engine(S)
    try:
        hip = eng.hip
        n_dead = sum(S["dirty"]["Room"][i] == S["rooms"][dead] for i in range(n))
        hip.set_own(0, np.full((1, n), -1, dtype=np.int32))
        hip.set_active_rows(0, n)
        chosen, logml = hip.sweep_own(InferenceConfig(1, 2).as_c(), 5, 1, n)
        st = hip.get_own_stats()
        assert st.impossible_rows == n_dead and st.first_impossible_row == seen and logml[seen] == -math.inf
        vals = hip.get_own(0, 1, n)[0]
        gone = np.array([S["dirty"]["Room"][i] == S["rooms"][dead] for i in range(n)])
        assert (vals[gone] == S["K"] - 1).all() and np.isfinite(logml[~gone]).all()
        with pytest.raises(ValueError, match="none of the options of an own choice is possible"):
            eng.sweep_own(tr, InferenceConfig(1, 2), 5, 1)
    finally:
        eng.close()


def test_statistics_and_the_two_routes_of_the_parameter_move():
    S = ogp.gauss_case(3, 4, n_rows=500, seed=9, nonlinear=True, second="room")
    n = S["n_rows"]
    lw, eng, tr = _engine(S)
    try:
        hip = eng.hip
        eng.sweep_own(tr, InferenceConfig(1, 2), 3, 0)
        assert tr._own_dev is eng, "the device is not ahead"
        vals = hip.get_own(0, 1, n)[0]
        for g in (0, 1):
            spec = lw.gauss_specs[g]
            count, qsum, e = hip.own_gauss_stats(0, 0, g, spec["n_mean"])
            assert e == tr.own_gauss_exponent(g) == hip.own_gauss_exponent(0, 0, g)
            c2, q2 = ogp.numpy_stats(S, lw, vals, g, e)
            assert np.array_equal(count, c2) and np.array_equal(qsum, q2) and count.sum() > 0
        # the device route (ahead) and the host route leave the same parameter values
        state = tr.rng.bit_generator.state
        before = {k: v.value.copy() for k, v in tr.params.items()}, [mp.value.copy() for mp in tr.mean_params]
        tr.resample_parameters()
        assert tr._own_dev is eng, "the parameter move pulled the rows"
        after = {k: v.value.copy() for k, v in tr.params.items()}, [mp.value.copy() for mp in tr.mean_params]
        own = tr.own.copy()  # (pulls)
        t2 = Trace(lw, n, 0)
        for k, v in before[0].items():
            t2.params[k].value = v.copy()
        for mp, v in zip(t2.mean_params, before[1]):
            mp.value = v.copy()
        t2.rng.bit_generator.state = state
        t2.own = own
        t2.resample_parameters()
        for k in after[0]:
            assert np.array_equal(t2.params[k].value.view(np.uint64), after[0][k].view(np.uint64)), k
        for g, v in enumerate(after[1]):
            assert np.array_equal(t2.mean_params[g].value.view(np.uint64), v.view(np.uint64)), f"mean parameter {g}"
            assert not np.array_equal(v, before[1][g])
        # after pclean_set_own, with rows at -1
        own[:, ::3] = -1
        tr.own = own
        eng._push_own(tr)
        joint = tr.own_joint(own, 0, 1)
        for g in (0, 1):
            count, qsum, e = hip.own_gauss_stats(0, 0, g, lw.gauss_specs[g]["n_mean"])
            c2, q2 = ogp.numpy_stats(S, lw, joint, g, e)
            assert np.array_equal(count, c2) and np.array_equal(qsum, q2)
            c3, q3, _ = tr.own_gauss_stats(g)
            assert np.array_equal(count, c3) and np.array_equal(qsum, q3)
    finally:
        eng.close()


@pytest.fixture(scope="module")
def dist():
    S, pis = ogp.dist_case()
    lw, eng, tr = _engine(S)
    rng = np.random.default_rng(77)
    cur = np.array([int(rng.choice(list(pi), p=np.array(list(pi.values())) / sum(pi.values()))) for pi in pis])
    yield S, pis, cur, eng, tr
    eng.close()


@pytest.mark.parametrize("P,mh", [(1, False), (2, False), (2, True), (9, False)], ids=["P1", "P2-PG", "P2-MH", "P9"])
def test_sweeps_follow_the_exact_joint_conditional(dist, P, mh):
    S, pis, cur, eng, tr = dist
    n, nb = S["n_rows"], S["nb"]
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
    draws = [[] for _ in range(n)]
    for s in range(ogp.S_DRAWS):
        tr.own = np.stack([cur // nb, cur % nb]).astype(np.int32)
        eng.sweep_own(tr, cfg, 9300 + P, s, want_outputs=False)
        own = tr.own
        for i, k in enumerate((own[0] * nb + own[1]).tolist()):
            draws[i].append(k)
    items = [(i, ocp.expected_output(pis[i], int(cur[i]), P, mh), pe.tabulate(draws[i])) for i in range(n)]
    res = pe.gof(items)
    print(f"\n[own gauss P={P}{' MH' if mh else ''}] {pe.describe(res)}")
    assert res["p"] > pe.ALPHA, pe.describe(res)
    if P == 1:
        assert all(set(d) == {int(cur[i])} for i, d in enumerate(draws)), "one particle: the retained one"


def test_planted_units_and_rooms_come_back():
    """a tenth of the rents stated in thousands, the rooms' means 10 sigma apart; the room is observed directly in four rows
    of five (that pins every room's mean: rooms seen through AddTypos alone can end with their means swapped when the first
    windows start from prior draws of the means) and has to come back from the rent in the others"""
    S = ogp.gauss_case(5, 2, n_rows=600, seed=12, spread=10.0, wrong_unit=0.1, typos=False, direct=True, room_missing=0.2)
    n = S["n_rows"]
    truth = np.array(S["truth"])
    planted = np.flatnonzero((truth[:, 1] == 1) | np.array([v is None for v in S["dirty"]["Room"]]))
    assert sum(v is None for v in S["dirty"]["Room"]) >= 90 and (truth[:, 1] == 1).sum() >= 40
    sure = np.array([ogp.exact_pi(S, i).get(int(truth[i, 0] * 2 + truth[i, 1]), 0.0) >= 1.0 - 1e-9 for i in range(n)])
    assert sure[planted].mean() >= 0.9, "the condition would hide a failure"
    lw, eng, tr = _engine(S, params=False)
    try:
        cfg = InferenceConfig(3, 5)
        inf.initialize_trace(eng, tr, cfg, 1)
        inf.run_inference(eng, tr, cfg, 1)
        tr.check_consistency()
        marg = eng.own_marginals(tr, top=2)
        own = tr.own
        bad = [i for i in np.flatnonzero(sure) if own[0, i] != truth[i, 0] or own[1, i] != truth[i, 1]]
        assert not bad, f"rows {bad[:10]} did not come back ({len(bad)} of {int(sure.sum())})"
        # the cleaned table reports the number under the row's unit; the MAP table under the MAP unit with its confidence
        table = reconstructed_table(lw, tr, S["dirty"])
        i = int(np.flatnonzero((truth[:, 1] == 1) & sure)[0])
        assert table["Rent"][i] == round(S["dirty"]["Rent"][i] * 1000.0)
        j = int(np.flatnonzero(np.array([v is None for v in S["dirty"]["Room"]]) & sure)[0])
        assert table["Room"][j] == S["rooms"][truth[j, 0]]
        mtab, conf = map_table(lw, marg, S["dirty"])
        assert mtab["Rent"][i] == table["Rent"][i] and conf["Rent"][i] > 0.999 and set(conf) == {"Room", "Rent"}
        assert mtab["Room"][j] == table["Room"][j]
        assert np.array_equal(conf["Rent"], marg["unit"][1][0])
        miss = np.array([v is None for v in S["dirty"]["Room"]])
        clean = dict(S["dirty"], Room=[S["rooms"][a] for a in truth[:, 0]])
        acc = evaluate_accuracy(lw, tr, S["dirty"], clean)
        assert acc["changed"] >= int(((truth[:, 1] == 1) & sure).sum())
        assert acc["imputed"] == int(miss.sum()) and acc["correctly_imputed"] >= int((miss & sure).sum())
    finally:
        eng.close()


def test_abi_refusals_leave_the_plan_as_it_was():
    S = ogp.gauss_case(3, 2, n_rows=80, seed=4)
    n, K = S["n_rows"], S["K"]
    lw, eng, tr = _engine(S)
    try:
        hip = eng.hip
        rows = np.arange(n, dtype=np.int32)
        ref = hip.score_own(0, 0, rows, seed=1, sweep=1, n_draws=1, n_cand=K, want_scores=True)
        spec = lw.own_gauss[(0, 0)]["specs"][0]

        def refused(status, block=0, node=0, **change):
            sp = dict(spec)
            sp.update(change)
            with pytest.raises(_lib.PCleanHipError, match=f"status {status}"):
                hip.add_own_gauss(block, node, make_gauss(sp))
        for kind in ("cand", "obs", "itemctx", "evctx"):
            refused(_lib_err("ARG"), kinds=[(kind, 0)])
        refused(_lib_err("ARG"), transform=("evctx", 0))
        refused(_lib_err("ARG"), node=1)
        refused(_lib_err("ARG"), block=3)
        refused(_lib_err("ARG"), local_n=[4097, 1])
        refused(_lib_err("ARG"), local_n=[3, 3])  # (not the table's grid)
        refused(_lib_err("ARG"), x_col=7)
        refused(_lib_err("ARG"), t_x_col=[5, -1], t_lad_col=[5, -1])
        def same_as_ref():
            got = hip.score_own(0, 0, rows, seed=1, sweep=1, n_draws=1, n_cand=K, want_scores=True)
            assert hip.get_own_stats().variants == 8
            for a, b in zip(ref, got):
                assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                                      b.view(np.uint64) if b.dtype == np.float64 else b)
        same_as_ref()
        for _ in range(_lib.MAX_GAUSS - 1):  # up to the capacity
            hip.add_own_gauss(0, 0, make_gauss(spec))
        refused(_lib_err("CAPACITY"))
        # reloading the block forgets the terms: the string-only kernels serve the leaf until they are attached again
        lw.load_blocks_into(hip)
        bare = hip.score_own(0, 0, rows, seed=1, sweep=1, n_draws=1, n_cand=K, want_scores=True)
        assert hip.get_own_stats().variants != 8 and not np.array_equal(bare[1], ref[1])
        with pytest.raises(_lib.PCleanHipError, match=f"status {_lib_err('ARG')}"):
            hip.own_gauss_stats(0, 0, 0, 3)
        eng._own_gauss_pending = True
        eng.upload_trace(tr)
        same_as_ref()
    finally:
        eng.close()


def _lib_err(name):
    return {"ARG": -1, "STATE": -4, "CAPACITY": -5}[name]
