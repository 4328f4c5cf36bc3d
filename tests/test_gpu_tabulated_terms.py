"""Tabulated likelihood terms (PCLEAN_DENS_TABULATED) on the GPU: the class-table kernels against the Python restatement
byte for byte, an equality constraint restated as a tabulated term against the oracle-verified path, the per-candidate
scores of tests/tabulated_program.py (single rows and evidence sets) with the same doubles added in the same order, a
consequence that is exact under the fixed-point contract, and the refusals of the C ABI."""
import ctypes as C

import numpy as np
import pytest

import posterior_exact as pe
import tabulated_program as tp
from pclean_amd import _lib
from pclean_amd._lib import HipContext, PCleanHipError
from pclean_amd.encode import StringPool
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import initialize_trace, observed_sweep
from pclean_amd.trace import Trace

pytestmark = pytest.mark.gpu

HALF_LOG26 = 1.629048269010741
NEG_INF = -np.inf


# ---- 1. class tables ---------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 63, 64, 65, 300]  # around one staged piece of the observed string (64 symbols), and many pieces


def _strings(n, seed, dots=True):
    """n strings whose lengths walk LENGTHS, over a small mixed-case alphabet so that subsequences and equal-ignoring-case
    pairs occur, with a few initial forms ("x.")"""
    rng = np.random.default_rng(seed)
    alpha = "abAB" + ("." if dots else "") + "Éé"
    out = []
    for i in range(n):
        L = LENGTHS[i % len(LENGTHS)]
        if i % 11 == 3:
            out.append("ab"[int(rng.integers(0, 2))] + ".")
        else:
            out.append("".join(alpha[int(rng.integers(0, len(alpha)))] for _ in range(L)))
    return out


@pytest.fixture(scope="module")
def string_world():
    """latent strings: random ones, copies of observed strings in another case (class 0 of both rules) and thinned copies
    (short versions); one context holds them all"""
    obs = _strings(131, 1)
    lat = _strings(257, 2)
    rng = np.random.default_rng(3)
    for j in range(0, 257, 5):
        o = obs[int(rng.integers(0, len(obs)))]
        lat[j] = o.swapcase() if j % 10 == 0 else "".join(ch for ch in o if rng.random() < 0.5)
    pool = StringPool()
    oid, lid = pool.add_all(obs), pool.add_all(lat)
    hip = HipContext(0)
    sym, off, _, _ = pool.arrays()
    hip.load_strings(sym, off)
    hip.set_fold_table(pool.fold_symbols())
    want = {rule: tp.class_table(rule, obs, lat) for rule in (tp.SHORT, tp.FORMAT)}
    yield dict(hip=hip, pool=pool, obs=obs, lat=lat, oid=oid, lid=lid, want=want)
    hip.close()


@pytest.mark.parametrize("rule", [tp.SHORT, tp.FORMAT])
@pytest.mark.parametrize("n_lat", [1, 257])
@pytest.mark.parametrize("n_obs", [0, 1, 131])
def test_class_table_equals_python(string_world, rule, n_lat, n_obs):
    W = string_world
    # (n = 1: the longest strings, 300 symbols on both sides)
    osel = np.arange(n_obs) if n_obs != 1 else np.array([6])
    lsel = np.arange(n_lat) if n_lat != 1 else np.array([6])
    W["hip"].build_class_table(5, W["oid"][osel], W["lid"][lsel], rule, W["pool"].symbol_of("."))
    got = W["hip"].get_pair_table(5, n_obs, n_lat)
    want = W["want"][rule][np.ix_(osel, lsel)] if n_obs else np.zeros((0, n_lat), dtype=np.uint16)
    assert got.shape == want.shape and np.array_equal(got, want)
    if n_obs == 131 and n_lat == 257:  # every class occurs
        assert set(np.unique(want)) == ({0, 1} if rule == tp.SHORT else {0, 1, 2})


def test_class_table_without_a_dot_symbol(string_world):
    """dot_symbol = 0xFFFF: no observed string is an initial form"""
    W = string_world
    W["hip"].build_class_table(5, W["oid"], W["lid"], tp.FORMAT, 0xFFFF)
    got = W["hip"].get_pair_table(5, 131, 257)
    want = W["want"][tp.FORMAT].copy()
    want[want == 1] = 2
    assert np.array_equal(got, want)


def test_count_short_versions_equals_python(string_world):
    W = string_world
    got = W["hip"].count_short_versions(W["oid"], W["lid"])
    want = (W["want"][tp.SHORT] == 0).sum(axis=0)
    assert np.array_equal(got, want) and want.max() > 1
    assert np.array_equal(W["hip"].count_short_versions(W["oid"][:0], W["lid"]), np.zeros(257, dtype=np.int32))


def test_class_table_refusals(string_world):
    W = string_world
    hip = W["hip"]
    ids = np.zeros(65536, dtype=np.int32)
    rc = hip.lib.pclean_build_class_table(hip.h, 6, 65536, ids.ctypes.data_as(C.POINTER(C.c_int32)), 1,
                                          W["lid"].ctypes.data_as(C.POINTER(C.c_int32)), tp.SHORT, 0xFFFF)
    assert rc == -5 and b"n_obs > 65535" in hip.lib.pclean_last_error(hip.h)
    rc = hip.lib.pclean_build_class_table(hip.h, 6, 1, ids.ctypes.data_as(C.POINTER(C.c_int32)), 1,
                                          W["lid"].ctypes.data_as(C.POINTER(C.c_int32)), 7, 0xFFFF)
    assert rc == -1
    fresh = HipContext(0)
    try:
        sym, off, _, _ = W["pool"].arrays()
        fresh.load_strings(sym, off)
        with pytest.raises(PCleanHipError, match="pclean_set_fold_table first"):
            fresh.build_class_table(0, W["oid"], W["lid"], tp.SHORT)
    finally:
        fresh.close()


# ---- 2. an equality constraint is a tabulated term ------------------------------------------------------------------------
def test_equality_constraints_as_tabulated_terms_sweep_identically():
    """flights (tests/golden/plans_flights.json is this lowering): every DENS_EQUAL term turned into DENS_TABULATED on the
    same 0/1 table with T[v] = [0, -inf, -inf, 0] — one sweep, same seed, same bits"""
    from test_flights_cpu import flights_setup
    dirty, clean, lw, obs = flights_setup()
    eng = Engine(lw, obs, dist_mode=1)
    try:
        cfg = InferenceConfig(1, 4, rejuv_frequency=500)
        tr = Trace(lw, obs.shape[1], 2)
        initialize_trace(eng, tr, cfg, 2, max_batch=512)
        eng.upload_trace(tr)

        def sweep():
            choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 5, 0)
            return choice.copy(), chosen.copy(), logml.copy(), {b: (r.copy(), v.copy()) for b, (r, v) in new_rows.items()}
        a = sweep()
        n_turned = 0
        for key, (pid, n) in lw.eq_pairs.items():
            eng.hip.set_class_density(pid, np.tile([0.0, NEG_INF, NEG_INF, 0.0], (n, 1)))
        for bi, blk in enumerate(lw.blocks):
            if blk.get("score"):
                continue
            arrs = list(lw.block_arrays(bi))
            terms = arrs[1].copy()
            eq = terms["dens_kind"] == _lib.DENS_EQUAL
            n_turned += int(eq.sum())
            terms["dens_kind"][eq] = _lib.DENS_TABULATED
            eng.hip.load_block(bi, arrs[0], terms, *arrs[2:])
        if len(set(lw.block_group)) < len(lw.block_group):  # (as LoweredModel.load_blocks_into does)
            for bi, g in enumerate(lw.block_group):
                eng.hip.set_block_group(bi, g)
        assert n_turned >= 4
        b = sweep()
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert set(a[3]) == set(b[3])
        for blk in a[3]:
            assert np.array_equal(a[3][blk][0], b[3][blk][0]) and np.array_equal(a[3][blk][1], b[3][blk][1])
    finally:
        eng.close()


# ---- 3 / 4. per-candidate scores of the helper program -------------------------------------------------------------------
@pytest.fixture(scope="module")
def program():
    S = tp.setup()
    lw, who = S["lw"], S["who"]
    n = S["obs"].shape[1]
    tr = Trace.from_clean_values(lw, {0: {"name": [w[0] for w in who], "nick": [w[1] for w in who]}}, n, 3)
    eng = Engine(lw, S["obs"], dist_mode=1)
    eng.upload_trace(tr)
    S.update(trace=tr, eng=eng, tabs=tp.term_tables(lw), dens=eng.hip.get_density_tables())
    yield S
    eng.close()


def _term_rows(S, terms, latent_of_cand):
    """per term of a node: (observed column, function(observed value index or -1) -> value per candidate or None)"""
    lw, eng = S["lw"], S["eng"]
    _, _, _, nb, logl = S["dens"]
    typo_tables = {pid: (odom, ldom) for pid, odom, ldom in lw.pair_id.values()}
    out = []
    for t in terms:
        pid, val = int(t["pair_table"]), latent_of_cand[int(t["cand_col"])]
        if t["dens_kind"] == _lib.DENS_TABULATED:
            _, cls, T = S["tabs"][pid]

            def fn(o, cls=cls, T=T, val=val):
                return T[val, 3] if o < 0 else T[val, cls[o, val]]
        else:
            odom, ldom = typo_tables[pid]
            D = eng.hip.get_pair_table(pid, len(odom), len(ldom)).astype(np.int64)
            L = np.array([len(ldom.string(v)) for v in range(len(ldom))])

            def fn(o, D=D, L=L, val=val):
                if o < 0:
                    return None  # an AddTypos term skips a missing observation (add_typos.jl:51-53)
                d = D[o, val]
                l = nb[(L[val] + 4) // 5, d].copy()  # the three operations of term_density
                l -= logl[L[val]] * d.astype(np.float64)
                l -= HALF_LOG26 * d.astype(np.float64)
                return l
        out.append((int(t["obs_col"]), fn))
    return out


def _node_terms(lw, arrays, nid):
    nodes, terms = arrays[0], arrays[1]
    return terms[nodes[nid]["term_begin"]:nodes[nid]["term_begin"] + nodes[nid]["n_terms"]]


def _restated_scores(S):
    """{node: [64][candidates (+ new row for the slot)]} of block 0, restated: the device's own prior, then each term's
    value in plan order; the slot's new row takes the device's own leaf marginals"""
    lw, eng, tr, obs = S["lw"], S["eng"], S["trace"], S["obs"]
    arrays = lw.block_arrays(0)
    n = obs.shape[1]
    rows = np.arange(n, dtype=np.int32)
    out, lse = {}, {}
    for nid in (1, 2):
        info = lw.blocks[0]["node_info"][nid]
        opts = lw.option_values[("Person", info["attr"])]
        logp, _, _ = eng.hip.get_table_priors(lw.option_id[("Person", info["attr"])], len(opts), is_options=True)
        tr_ = _term_rows(S, _node_terms(lw, arrays, nid), {0: opts})
        sc = np.empty((n, len(opts)))
        for i in range(n):
            sk = logp.copy()
            for col, fn in tr_:
                v = fn(int(obs[col, i]))
                if v is not None:
                    sk = sk + v
            sc[i] = sk
        out[nid] = sc
        lse[nid], got, _ = eng.hip.score_node(0, nid, rows, n_cand=len(opts), want_scores=True)
        out[("device", nid)] = got
        for i in range(n):  # the leaf marginal the slot's new row takes from the device, against the restated scores
            z = pe.log_marginal(dict(enumerate(sc[i].tolist())))
            assert abs(float(lse[nid][i]) - z) <= pe.logml_bound(len(opts), z), (nid, i, float(lse[nid][i]), z)
    t = tr.tables["Person"]
    cols, counts = t.view()
    full, m1, scal = eng.hip.get_table_priors(lw.table_id["Person"], t.n)
    latent = {j: cols[j] for j in range(cols.shape[0])}
    tr_ = _term_rows(S, _node_terms(lw, arrays, 0), latent)
    sc = np.empty((n, t.n + 1))
    excl = tr.cur[0]
    for i in range(n):
        e = int(excl[i])
        deleted = counts[e] <= 1
        sk = full - scal[1]
        sk[e] = NEG_INF if deleted else m1[e] - scal[1]
        sk[counts == 0] = NEG_INF
        for col, fn in tr_:
            v = fn(int(obs[col, i]))
            if v is not None:
                sk = sk + v
        snew = 0.0
        for nid in (1, 2):  # the children's marginals in plan order
            snew += lse[nid][i]
        sc[i, :t.n] = sk
        sc[i, t.n] = ((scal[3] if deleted else scal[2]) - scal[1]) + snew
    out[0] = sc
    _, got, _ = eng.hip.score_node(0, 0, rows, excl=excl, n_cand=t.n + 1, want_scores=True)
    out[("device", 0)] = got
    return out


@pytest.fixture(scope="module")
def restated(program):
    return _restated_scores(program)


@pytest.mark.parametrize("node", [0, 1, 2])
def test_scores_equal_the_restatement(restated, node):
    """score_node on the slot and on both leaves, all 64 rows: identical doubles in identical order"""
    want, got = restated[node], restated[("device", node)]
    assert want.shape == got.shape and np.isfinite(want).any()
    assert np.array_equal(got, want)


def test_evidence_scores_equal_the_restatement(program):
    """score_node_ev on the Person plan: evidence sets of 1, 3 and 70 rows (more than a wavefront, more than CS_TC entries),
    with repeated rows and missing values; multiplicity x T over the distinct observed values ascending, missing first"""
    S = program
    lw, eng, obs = S["lw"], S["eng"], S["obs"]
    pl = lw.latent_plans["Person"]
    arrays = lw.latent_block_arrays("Person")
    rng = np.random.default_rng(9)
    sets = [np.array([5]), np.array([0, 30, 30]), np.concatenate([[0, 1, 2, 8, 14, 40, 40], rng.integers(0, 64, 63)])]
    assert [len(s) for s in sets] == [1, 3, 70]
    ev_rows = np.concatenate(sets).astype(np.int32)
    ev_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    keys = np.arange(3, dtype=np.int32)
    eng.hip.set_active_rows(0, -1)
    for node, attr in enumerate(pl["root_attr"]):
        opts = lw.option_values[("Person", attr)]
        logp, _, _ = eng.hip.get_table_priors(lw.option_id[("Person", attr)], len(opts), is_options=True)
        tr_ = _term_rows(S, _node_terms(lw, arrays, node), {0: opts})
        want = np.empty((3, len(opts)))
        n_missing = 0
        for t, rows in enumerate(sets):
            sk = logp.copy()
            for col, fn in tr_:
                vals, mult = np.unique(obs[col, rows], return_counts=True)  # ascending: missing (-1) first
                n_missing += int(vals[0] < 0)
                for o, c in zip(vals, mult):
                    v = fn(int(o))
                    if v is not None:
                        sk = sk + np.float64(c) * v
            want[t] = sk
        assert n_missing > 0
        _, got, _ = eng.hip.score_node_ev(pl["block_id"], node, keys, ev_off, ev_rows, n_cand=len(opts), want_scores=True)
        assert np.array_equal(got, want), attr


# ---- 5. a candidate with a -1000 term is never chosen ----------------------------------------------------------------------
def _name_impossible(S, name, i):
    obs = S["dirty"]["Name"][i]
    return ("*" in name or name == "") if obs is None else tp.format_name_class(obs, name) == 2


def _nick_impossible(S, nick, i):
    obs = S["dirty"]["Long"][i]
    return (nick not in tp.LONGS) if obs is None else not tp.is_short_version(nick, obs)


def _has_impossible_term(S, name, nick, i):
    return _name_impossible(S, name, i) or _nick_impossible(S, nick, i)


def test_impossible_candidates_are_never_chosen(program, restated):
    S = program
    lw = S["lw"]
    # (a) from the restated score vectors: a candidate with a -1000 term has a fixed-point weight of exactly 0 (more than
    # 28.5 nats below the maximum) — every observed name and long form is reachable through the new row
    tr0 = S["trace"]
    cols, _ = tr0.tables["Person"].view()
    ndom, kdom = lw.latent_dom[("Person", "name")], lw.latent_dom[("Person", "nick")]
    cn, ck = lw.colidx["Person"]["name"], lw.colidx["Person"]["nick"]
    n = S["obs"].shape[1]
    checked = 0
    for i in range(n):
        sc = restated[0][i]
        for k in range(cols.shape[1]):
            if _has_impossible_term(S, ndom.string(cols[cn, k]), kdom.string(cols[ck, k]), i):
                assert sc[k] < sc.max() - 28.5
                checked += 1
        for nid, dom, impossible in ((1, ndom, _name_impossible), (2, kdom, _nick_impossible)):
            sl = restated[nid][i]
            for v in range(sl.shape[0]):
                if impossible(S, dom.string(v), i):
                    assert sl[v] < sl.max() - 28.5
                    checked += 1
    assert checked > 500

    # (b) initialize_trace and three sweeps with 5 particles, twice with one seed
    def run():
        eng = Engine(lw, S["obs"], dist_mode=1)
        try:
            cfg = InferenceConfig(3, 5, rejuv_frequency=500)
            tr = Trace(lw, n, 11)
            initialize_trace(eng, tr, cfg, 11, max_batch=32)
            for sweep in range(3):
                observed_sweep(eng, tr, cfg, 11, sweep)
            tr.check_consistency()
            c, _ = tr.tables["Person"].view()
            lw2 = eng.lw
            nd, kd = lw2.latent_dom[("Person", "name")], lw2.latent_dom[("Person", "nick")]
            people = [(nd.string(c[cn, r]), kd.string(c[ck, r])) for r in tr.cur[0]]
            return tr.cur.copy(), people
        finally:
            eng.close()
    cur_a, people_a = run()
    cur_b, people_b = run()
    assert np.array_equal(cur_a, cur_b) and people_a == people_b
    for i, (name, nick) in enumerate(people_a):
        assert not _has_impossible_term(S, name, nick, i), (i, name, nick)


# ---- 6. refusals on a loaded context --------------------------------------------------------------------------------------
def test_refusals_leave_the_loaded_plan_alone(program):
    S = program
    lw, eng, tr = S["lw"], S["eng"], S["trace"]
    hip = eng.hip
    cfg = InferenceConfig(1, 4, rejuv_frequency=500)

    def sweep():
        choice, chosen, logml, _ = eng.sweep(tr, cfg, 21, 1)
        return choice.copy(), chosen.copy(), logml.copy()
    before = sweep()
    pid = next(iter(lw.class_pairs))
    n_lat = len(lw.class_pairs[pid][2])
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    good = np.full((n_lat, 4), -1.0)
    err = lambda: hip.lib.pclean_last_error(hip.h)  # noqa: E731
    assert hip.lib.pclean_set_class_density(hip.h, 40, n_lat, dp(good)) == -1 and b"not valid" in err()
    assert hip.lib.pclean_set_class_density(hip.h, pid, n_lat + 1, dp(np.full((n_lat + 1, 4), -1.0))) == -1
    assert b"latent values" in err()
    for bad_value in (1e-300, np.nan, np.inf):
        bad = good.copy()
        bad[n_lat // 2, 1] = bad_value
        assert hip.lib.pclean_set_class_density(hip.h, pid, n_lat, dp(bad)) == -1 and b"log-probability" in err()
    # a tabulated term with a ctx slot
    arrs = list(lw.block_arrays(0))
    terms = arrs[1].copy()
    tab = np.flatnonzero(terms["dens_kind"] == _lib.DENS_TABULATED)[0]
    terms["ctx_slot"][tab], terms["fn_table"][tab] = 0, 0
    with pytest.raises(PCleanHipError, match="status -1: pclean_load_block: tabulated term .* with a ctx slot"):
        hip.load_block(0, arrs[0], terms, arrs[2], arrs[3], [0], [0])
    # prior proposals
    with pytest.raises(PCleanHipError, match="tabulated likelihood term .* use_dd_proposals = false"):
        eng.sweep(tr, InferenceConfig(1, 4, rejuv_frequency=500, use_dd_proposals=False), 21, 1)
    after = sweep()
    assert all(np.array_equal(x, y) for x, y in zip(before, after))
    # -inf is allowed, and the same values uploaded again change nothing
    T = S["tabs"][pid][2].copy()
    hip.set_class_density(pid, T)
    assert all(np.array_equal(x, y) for x, y in zip(before, sweep()))
