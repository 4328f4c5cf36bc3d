"""Exact marginals of a flat class on the device: pclean_own_marginals / Engine.own_marginals.

1  parity        options and probabilities == own_marginal_program.marginal_twin on pclean_score_own's scores (themselves pinned
                 to the leaf path by tests/test_gpu_own_choice.py) with the device's own fixw, bit for bit; K below, at and above
                 the LDS-resident limit (both kernel variants), top 1, 3 and 8; an impossible row.
2  ties          equal weights go to the smaller option index (own_marginal_program.ties).
3  current       the probability of every row's current value, 0.0 for a row without one.
4  independence  windows of 1, 64, 65 rows and the rest == all rows; a probe changes neither the values nor a later sweep.
5  literal       against the conditional from oracle/literal.py on the strings, within own_marginal_program.bound.
6  refusals      the C ABI refuses what it does not serve and leaves plan and values as they were."""
import ctypes as C

import numpy as np
import pytest

import own_choice_program as ocp
import own_marginal_program as omp
from pclean_amd import _lib
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.model import LoweredModel
from pclean_amd.trace import Trace

pytestmark = pytest.mark.gpu

LIMIT = 4096  # own_block.hip: OWN_LDS_OPTIONS
TOPS = (1, 3, 8)


def _flat_engine(S, params):
    lw, obs = ocp.lower(S)
    eng = Engine(lw, obs, dist_mode=1)
    tr = Trace(lw, S["n_rows"], 0)
    for k, v in params.items():
        tr.params[("Obs", k)].value = np.asarray(v, dtype=np.float64)
    eng.upload_trace(tr)
    return lw, eng, tr


def _fixw(hip):
    return lambda d: hip.debug_detmath(d)[2]


def _expected(eng, block, node, K, n, top):
    """marginal_twin on the probe's scores of every row"""
    rows = np.arange(n, dtype=np.int32)
    eng.hip.set_active_rows(0, n)
    _, scores, _ = eng.hip.score_own(block, node, rows, n_cand=K, want_scores=True)
    return omp.marginal_twin(scores, _fixw(eng.hip), top)


def _same(got, want_opt, want_prob):
    opt, prob = got[0], got[1]
    assert opt.dtype == np.int32 and prob.dtype == np.float64 and opt.shape == want_opt.shape == prob.shape
    assert np.array_equal(opt, want_opt), "options differ from the definition"
    assert np.array_equal(prob.view(np.uint64), want_prob.view(np.uint64)), "probabilities differ from the definition"


# ---- 1: parity with the scores -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 63, 64, 65, 257, LIMIT, LIMIT + 1])
def test_parity_with_the_scores_flat1(K):
    S = ocp.flat1(K=K, seed=K)
    n = S["n_rows"]
    p = np.random.default_rng(K).dirichlet(np.ones(K))
    lw, eng, tr = _flat_engine(S, {"p": p})
    try:
        want_opt, want_prob, u, U = _expected(eng, 0, 0, K, n, max(TOPS))
        assert all(U)
        for top in TOPS:
            got = eng.hip.own_marginals(0, 0, top, n)
            st = eng.hip.get_own_stats()
            _same(got, want_opt[:top], want_prob[:top])
            assert st.variants == (1 if K <= LIMIT else 2), "the other kernel variant ran"
            assert st.lds_options == LIMIT and st.impossible_rows == 0 and st.first_impossible_row == -1
            assert st.n_runs == len(set(S["dirty"]["Y"])) and st.longest_run == max(ocp.RUNS) and st.n_workgroups == st.n_runs
            assert eng.hip.get_timing().total_ms > 0.0
            assert (got[2] == 0.0).all()  # no row has a value yet
        if K == 1:  # one option: the slots beyond it are free
            opt, prob, _ = eng.hip.own_marginals(0, 0, 3, n)
            assert (opt[0] == 0).all() and (prob[0] == 1.0).all() and (opt[1:] == -1).all() and (prob[1:] == 0.0).all()
        else:
            assert (want_opt[:min(K, 8)] >= 0).any(axis=1).all()
    finally:
        eng.close()


def test_parity_with_the_scores_flat3_and_an_impossible_row():
    S = ocp.flat3()
    n = S["n_rows"]
    names = S["choices"]["name"]
    K = len(names)
    p = np.random.default_rng(3).dirichlet(np.ones(K))
    seen = next(i for i in range(n) if S["dirty"]["Name"][i] is not None)
    dead = names.index(S["dirty"]["Name"][seen])
    p[dead] = 0.0  # the directly observed option of row `seen` has no prior mass: every option of that row scores -inf
    p /= p.sum()
    lw, eng, tr = _flat_engine(S, {"p": p})
    try:
        want_opt, want_prob, u, U = _expected(eng, 0, 0, K, n, max(TOPS))
        impossible = [i for i in range(n) if S["dirty"]["Name"][i] == names[dead]]
        assert [i for i in range(n) if U[i] == 0] == impossible and seen in impossible
        for top in TOPS:
            got = eng.hip.own_marginals(0, 0, top, n)
            st = eng.hip.get_own_stats()
            _same(got, want_opt[:top], want_prob[:top])
            assert (got[0][:, impossible] == -1).all() and (got[1][:, impossible] == 0.0).all()
            assert st.variants == 1 and st.impossible_rows == len(impossible) and st.first_impossible_row == impossible[0]
        # a row with a direct observation whose option is possible: that option alone
        alive = next(i for i in range(n) if S["dirty"]["Name"][i] not in (None, names[dead]))
        assert got[0][:, alive].tolist() == [names.index(S["dirty"]["Name"][alive])] + [-1] * 7 and got[1][0, alive] == 1.0
        # a window that holds no impossible row reports none
        lo = impossible[-1] + 1
        if lo < n:
            eng.hip.set_active_rows(lo, n - lo)
            part = eng.hip.own_marginals(0, 0, 3, n - lo)
            assert eng.hip.get_own_stats().impossible_rows == 0
            _same(part, want_opt[:3, lo:], want_prob[:3, lo:])
    finally:
        eng.close()


# ---- 2: ties -----------------------------------------------------------------------------------------------------------
def test_equal_weights_go_to_the_smaller_index():
    S = omp.ties()
    n = S["n_rows"]
    words = S["choices"]["state"]
    K = len(words)
    lw, eng, tr = _flat_engine(S, {})
    try:
        want_opt, want_prob, u, U = _expected(eng, 0, 0, K, n, 8)
        # first, on the expectation: the ties are there, inside the top
        none = [i for i in range(n) if S["dirty"]["Y"][i] is None]
        assert none
        for i in none:
            assert len(set(u[i].tolist())) == 1 and want_opt[:, i].tolist() == list(range(8))
        pairs = []
        for a, b, o in omp.TIE_PAIRS:
            ka, kb = sorted((words.index(a), words.index(b)))
            for i in (i for i in range(n) if S["dirty"]["Y"][i] == o):
                assert u[i, ka] == u[i, kb] == u[i].max() and want_opt[:2, i].tolist() == [ka, kb]
                pairs.append((i, ka, kb))
        assert len(pairs) > 64
        for top in (1, 2, 8):
            opt, prob, _ = eng.hip.own_marginals(0, 0, top, n)
            _same((opt, prob), want_opt[:top], want_prob[:top])
            for i in none:
                assert opt[:, i].tolist() == list(range(top))
            for i, ka, kb in pairs:
                assert opt[:2, i].tolist() == [ka, kb][:top]
    finally:
        eng.close()


# ---- 3: the current value ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [70, LIMIT + 1])
def test_probability_of_the_current_value(K):
    S = ocp.flat1(K=K, seed=5)
    n = S["n_rows"]
    p = np.random.default_rng(5).dirichlet(np.ones(K))
    lw, eng, tr = _flat_engine(S, {"p": p})
    try:
        want_opt, want_prob, u, U = _expected(eng, 0, 0, K, n, 2)
        rng = np.random.default_rng(6)
        cur = rng.integers(K, size=n).astype(np.int32)
        cur[::3] = want_opt[0, ::3]  # the MAP option, a random one (mostly of weight 0), none
        cur[1::7] = -1
        tr.own = cur[None, :]
        got = eng.own_marginals(tr, top=2)["city"]
        _same(got, want_opt, want_prob)
        want = omp.current_twin(u, U, cur)
        assert np.array_equal(got[2].view(np.uint64), want.view(np.uint64))
        assert (got[2][cur < 0] == 0.0).all() and np.array_equal(got[2][::3][cur[::3] >= 0], got[1][0, ::3][cur[::3] >= 0])
        assert (want > 0).any() and (want[cur >= 0] == 0.0).any()
        assert np.array_equal(eng.hip.get_own(0, 1, n)[0], cur)
    finally:
        eng.close()


# ---- 4: independence -------------------------------------------------------------------------------------------------------
def _start(S, lw, seed, none_from):
    rng = np.random.default_rng(seed)
    tr0 = Trace(lw, S["n_rows"], 0)
    own = np.full((len(tr0.own_leaves()), S["n_rows"]), -1, dtype=np.int32)
    for li, (a, _, _) in enumerate(tr0.own_leaves()):
        own[li, :none_from] = rng.integers(len(S["choices"][a]), size=none_from)
    return own


@pytest.mark.parametrize("prog", ["flat1", "flat2b"])
def test_windows_and_probing_change_nothing(prog):
    S = ocp.flat1(K=70, seed=4) if prog == "flat1" else ocp.flat2b()
    n = S["n_rows"]
    lw, eng, tr = _flat_engine(S, {})
    try:
        start = _start(S, lw, 1, n // 2)
        cfg = InferenceConfig(1, 3)
        tr.own = start.copy()
        chosen, logml = eng.sweep_own(tr, cfg, 21, 5)
        vals = tr.own.copy()
        # the same sweep with marginals probed before it, whole and in windows
        tr.own = start.copy()
        whole = eng.own_marginals(tr, top=3)
        parts = [eng.own_marginals(tr, top=3, lo=lo, hi=hi) for lo, hi in ((0, 1), (1, 65), (65, 130), (130, n))]
        for a in whole:
            for j in range(3):
                joined = np.concatenate([p[a][j] for p in parts], axis=-1)
                assert joined.dtype == whole[a][j].dtype and np.array_equal(joined.view(np.uint8), whole[a][j].view(np.uint8)), (a, j)
            assert (whole[a][2][:n // 2] >= 0).all() and (whole[a][2][n // 2:] == 0.0).all()
        for b, l0, l1 in eng._own_blocks(tr):
            assert np.array_equal(eng.hip.get_own(b, l1 - l0, n), start[l0:l1])
        assert getattr(tr, "_own_dev", None) is None  # the device is not ahead of the trace
        chosen2, logml2 = eng.sweep_own(tr, cfg, 21, 5)
        assert np.array_equal(chosen2, chosen) and np.array_equal(logml2.view(np.uint64), logml.view(np.uint64))
        assert np.array_equal(tr.own, vals)
        tr.check_consistency()
    finally:
        eng.close()


# ---- 5: the literal conditional --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prog", ["flat3", "flat2b"])
def test_against_the_literal_conditional(prog):
    S, params = omp.literal_cases()[prog]
    n = S["n_rows"]
    lw, eng, tr = _flat_engine(S, params)
    try:
        marg = eng.own_marginals(tr, top=8)
        compared = total = 0
        for choice, names in S["choices"].items():
            K = len(names)
            opt, prob, _ = marg[choice]
            pis = [pi for _, pi in omp.exact_rows(S, params, choice)]
            worst = 0.0
            for i, pi in enumerate(pis):
                assert (opt[:, i] >= 0).sum() == min(8, (prob[:, i] > 0).sum())
                for t in range(8):
                    if opt[t, i] >= 0:
                        worst = max(worst, abs(prob[t, i] - pi.get(names[opt[t, i]], 0.0)))
            print(f"\n[{prog}.{choice}] largest |prob - pi| {worst:.3g}, bound {omp.bound(K):.3g}")
            assert worst <= omp.bound(K)
            rows = omp.compared_rows(S, pis, choice)
            for i in rows:
                assert names[opt[0, i]] == max(pis[i], key=pis[i].get), (choice, i)
            compared += len(rows)
            total += n
        assert compared >= 0.9 * total
    finally:
        eng.close()


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_plan_and_values_alone():
    S = ocp.flat3()
    n = S["n_rows"]
    lw, eng, tr = _flat_engine(S, {})
    try:
        tr.own = _start(S, lw, 3, n // 2)
        start = tr.own.copy()
        before = eng.own_marginals(tr, top=8)["name"]
        for args, what in (((0, 0, 0), "top must be 1 .. 8"), ((0, 0, 9), "top must be 1 .. 8"),
                           ((1, 0, 1), "block 1 is not a loaded own block"), ((-1, 0, 1), "not a loaded own block"),
                           ((0, 1, 1), "block 0 has no node 1"), ((0, -1, 1), "block 0 has no node -1")):
            with pytest.raises(_lib.PCleanHipError, match=what):
                eng.hip.own_marginals(args[0], args[1], args[2], n)
            assert np.array_equal(eng.hip.get_own(0, 1, n), start)
        opt = np.empty((1, n), dtype=np.int32)
        with pytest.raises(_lib.PCleanHipError, match="null outputs"):
            _lib.check(eng.hip.h, eng.hip.lib.pclean_own_marginals(eng.hip.h, C.c_int32(0), C.c_int32(0), C.c_int32(1),
                                                                   _lib._p(opt, C.c_int32), None, None), "pclean_own_marginals")
        after = eng.own_marginals(tr, top=8)["name"]
        for j in range(3):
            assert np.array_equal(after[j].view(np.uint8), before[j].view(np.uint8))
        assert np.array_equal(eng.hip.get_own(0, 1, n), start)
    finally:
        eng.close()
    # a class with a reference slot has no own block: the engine refuses, and so does the library
    T = ocp.twin1(ocp.flat1())
    lwt = LoweredModel(T["model"], T["query"], T["dirty"])
    engt = Engine(lwt, lwt.encode_observations(T["dirty"]), dist_mode=1)
    try:
        with pytest.raises(_lib.PCleanHipError, match="the observed class is not flat"):
            engt.own_marginals(Trace(lwt, T["n_rows"], 0))
        with pytest.raises(_lib.PCleanHipError, match="block 0 is not a loaded own block"):
            engt.hip.own_marginals(0, 0, 1, T["n_rows"])
    finally:
        engt.close()
