"""The three-name FormatName term (PCLEAN_DENS_NAME3, format_name.jl:14-26) on the GPU, against the Python restatement of
tests/name3_program.py: the prefix / suffix byte tables byte for byte; the scores of every (row, candidate) of the slot at
the candidate counts where the generic enumeration takes another kernel or another scoring loop, and the log-marginals
from the fixed-point contract, bit for bit; the leaves of a new row; the Person plan against evidence sets with its draws;
observed sweeps against the same plan with the term replaced by a table of its restated values; the refusals."""
import ctypes as C

import numpy as np
import pytest

import name3_program as n3
from pclean_amd import _lib
from pclean_amd._lib import HipContext, PCleanHipError
from pclean_amd.encode import StringPool
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.trace import Trace

pytestmark = pytest.mark.gpu

NEG_INF = -np.inf
TWO_M40 = 9.094947017729282379150390625e-13  # 2^-40 (include/pclean_detmath.h: pclean_lse_from_fix)


# ---- the fixed-point contract, restated with the oracle's own pieces ------------------------------------------------------
def fix_weights(orc, scores):
    """(m, [u_k]) of a score vector: u_k = pclean_fixw(s_k - m), exactly 0 from 28.5 nats below the maximum"""
    m = float(np.max(scores))
    L = orc.lib()
    if m == NEG_INF:
        return m, [0] * len(scores)
    return m, [int(L.pco_fixw(float(s - m))) if s - m > -40.0 else 0 for s in scores]


def fix_lse(orc, scores):
    m, u = fix_weights(orc, scores)
    U = sum(u)
    return NEG_INF if U == 0 else m + orc.lib().pco_det_log(float(U) * TWO_M40)


def fix_draw(orc, scores, seed, row, site, particle, sweep):
    """inverse-CDF draw of the kernels: the first k whose inclusive fixed-point prefix exceeds floor(R U / 2^64)"""
    _, u = fix_weights(orc, scores)
    U = sum(u)
    x = (int(orc.lib().pco_rand64(seed, row, site, particle, sweep)) * U) >> 64
    acc = 0
    for k, w in enumerate(u):
        acc += w
        if acc > x:
            return k
    raise AssertionError("empty score vector")


# ---- 1. the two byte tables ------------------------------------------------------------------------------------------------------
LENGTHS = [0, 1, 2, 3, 63, 64, 65, 66, 129, 300]  # around one and two staged pieces of the observed string (64 symbols)


def test_affix_tables_equal_python_on_long_strings():
    """observed strings of every length around the staged pieces; latent strings cut from them at a space (true prefixes
    and suffixes, in another case), cut one symbol off it (near misses), and random ones"""
    rng = np.random.default_rng(4)
    alpha = "abAB  Éé"
    obs = ["".join(alpha[int(rng.integers(0, len(alpha)))] for _ in range(LENGTHS[i % len(LENGTHS)])) for i in range(131)]
    lat = []
    for j in range(257):
        o = obs[int(rng.integers(0, len(obs)))]
        sp = [p for p, ch in enumerate(o) if ch == " "]
        if j % 4 == 3 or not sp:
            lat.append("".join(alpha[int(rng.integers(0, len(alpha)))] for _ in range(int(rng.integers(0, 6)))))
            continue
        p = sp[int(rng.integers(0, len(sp)))] + (1 if j % 8 == 4 else 0)
        lat.append((o[:p] if j % 2 == 0 else o[p + 1:]).swapcase())
    pool = StringPool()
    oid, lid = pool.add_all(obs), pool.add_all(lat)
    hip = HipContext(0)
    try:
        sym, off, _, _ = pool.arrays()
        hip.load_strings(sym, off)
        hip.set_fold_table(pool.fold_symbols())
        for rule, fn in ((_lib.CLASS_NAME_PREFIX, n3.is_prefix), (_lib.CLASS_NAME_SUFFIX, n3.is_suffix)):
            want = n3.affix_table(fn, obs, lat)
            assert 50 < int(want.sum()) < want.size // 2
            hip.build_class_table(5, oid, lid, rule, pool.symbol_of(" "))
            assert np.array_equal(hip.get_pair_table(5, len(obs), len(lat)), want)
            hip.build_class_table(5, oid[:1], lid[6:7], rule, pool.symbol_of(" "))
            assert np.array_equal(hip.get_pair_table(5, 1, 1), want[:1, 6:7])
            hip.build_class_table(5, oid, lid, rule, 0xFFFF)  # no separator in the pool: nothing matches
            assert not hip.get_pair_table(5, len(obs), len(lat)).any()
    finally:
        hip.close()


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(variant, tagged=False):
        key = (variant, tagged)
        if key not in made:
            S = n3.setup(variant, tagged)
            lw, d = S["lw"], S["dirty"]
            n = S["obs"].shape[1]
            clean = {"first": d["First"], "middle": d["Middle"], "last": d["Last"]}
            if tagged:
                clean["tag"] = [n3.TAGS[j] for j in S["who"]]
            tr = Trace.from_clean_values(lw, {0: clean}, n, 3)
            eng = Engine(lw, S["obs"], dist_mode=1)
            eng.upload_trace(tr)
            S.update(trace=tr, eng=eng, n=n)
            made[key] = S
        return made[key]
    yield get
    for S in made.values():
        S["eng"].close()


@pytest.mark.parametrize("variant", n3.VARIANTS)
def test_program_tables_equal_the_restatement(worlds, variant):
    S = worlds(variant)
    lw, hip = S["lw"], S["eng"].hip
    rules = {_lib.CLASS_NAME_PREFIX: n3.is_prefix, _lib.CLASS_NAME_SUFFIX: n3.is_suffix}
    assert sorted(r for r, *_ in lw.class_pairs.values()) == sorted(rules)
    for pid, (rule, odom, ldom, _) in lw.class_pairs.items():
        want = n3.affix_table(rules[rule], [odom.string(u) for u in range(len(odom))], [ldom.string(v) for v in range(len(ldom))])
        assert np.array_equal(hip.get_pair_table(pid, len(odom), len(ldom)), want) and want.any()


# ---- 2. scores of the slot ---------------------------------------------------------------------------------------------------------
def _node_terms(arrays, nid):
    nodes, terms = arrays[0], arrays[1]
    return terms[nodes[nid]["term_begin"]:nodes[nid]["term_begin"] + nodes[nid]["n_terms"]]


def _slot_scores(S, R, cand, counts, rows, prior):
    """prior, then the slot's terms in plan order: the name3 term from the restatement on the candidates' strings, an
    equality constraint as 0.0 / -inf on the strings; a missing observation is skipped"""
    lw, d = S["lw"], S["dirty"]
    terms = _node_terms(lw.block_arrays(0), 0)
    col_of = {"p.first": (0, "First"), "p.middle": (1, "Middle"), "p.last": (2, "Last")}
    out = np.empty((len(rows), len(cand)))
    memo = {}
    live = counts != 0
    for r, i in enumerate(rows):
        key = tuple(d[c][i] for c in ("Full", "First", "Middle", "Last"))
        sk = memo.get(key)
        if sk is None:
            sk = prior.copy()
            for t in terms:
                name = lw.obs_cols[int(t["obs_col"])]
                if t["dens_kind"] == _lib.DENS_NAME3:
                    if key[0] is not None:
                        sk = sk + np.array([R(key[0], *c) for c in cand])
                else:
                    assert t["dens_kind"] == _lib.DENS_EQUAL
                    j, col = col_of[name]
                    sk = sk + np.array([0.0 if c[j] == d[col][i] else NEG_INF for c in cand])
            sk[~live] = NEG_INF  # (a free slot: its values are never looked at)
            memo[key] = sk
        out[r] = sk
    return out


@pytest.fixture(scope="module")
def score_world():
    """an engine of its own for the hand-made Person tables (the sweeps below keep theirs)"""
    S = n3.setup("observed")
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    S.update(eng=eng, n=S["obs"].shape[1], R=n3.Restated())
    yield S
    eng.close()


@pytest.mark.parametrize("k,rows,slot", n3.SCORE_CASES, ids=[f"{c[0]}-{c[2]}" for c in n3.SCORE_CASES])
def test_slot_scores_equal_the_restatement(score_world, oracle, k, rows, slot):
    S = score_world
    lw, hip = S["lw"], S["eng"].hip
    cand, counts = n3.candidates(k)
    ci = lw.colidx["Person"]
    cols = np.zeros((len(lw.layout["Person"]), k), dtype=np.int32)
    for j, name in enumerate(("first", "middle", "last")):
        dom = lw.latent_dom[("Person", name)]
        cols[ci[name]] = [dom.index_of(c[j]) for c in cand]
    tid = lw.table_id["Person"]
    hip.set_table(tid, cols, counts, 1.0, 0.0)
    full, _, scal = hip.get_table_priors(tid, k)
    rows = n3.case_rows(S["n"], rows)
    want = _slot_scores(S, S["R"], cand, counts, rows, full - scal[0])
    hip.enum_launches(reset=True)
    lse, got, draws = hip.score_node(0, 0, rows, snew=np.zeros(len(rows)), n_cand=k + 1, want_scores=True, seed=77, sweep=2,
                                     n_draws=1)
    launched = {s: c for s, c in hip.enum_launches().items() if c}
    assert set(launched) == {slot}, launched
    new = (scal[2] - scal[0]) + 0.0
    assert np.array_equal(got[:, :k], want), np.argwhere(got[:, :k] != want)[:5]
    assert np.all(got[:, k] == new)
    site = (0 << 16) | 0
    for r in range(0, len(rows), max(1, len(rows) // 40)):  # the log-marginal and the draw of every ~27th row
        sc = np.append(want[r], new)
        assert float(lse[r]) == fix_lse(oracle, sc), (r, float(lse[r]))
        assert int(draws[r, 0]) == (lambda x: -1 if x == k else x)(fix_draw(oracle, sc, 77, int(rows[r]), site, 0, 2)), r


# ---- 3. the leaves of a new row -----------------------------------------------------------------------------------------------------
def _leaf_scores(S, R, nid, rows, ev_sets=None):
    """scores of option list `nid` of block 0 (or of the Person plan, with ev_sets: one evidence set per item): the device's
    own option priors, then the leaf's terms in plan order"""
    lw, d, hip = S["lw"], S["dirty"], S["eng"].hip
    pl = lw.latent_plans["Person"]
    if ev_sets is None:
        arrays, info = lw.block_arrays(0), lw.blocks[0]["node_info"][nid]
    else:
        arrays, info = lw.latent_block_arrays("Person"), pl["node_info"][nid]
    attr = info["attr"]
    dom = lw.latent_dom[("Person", attr)]
    opts = lw.option_values[("Person", attr)]
    ostr = [dom.string(int(v)) for v in opts]
    logp, _, _ = hip.get_table_priors(lw.option_id[("Person", attr)], len(opts), is_options=True)
    terms = _node_terms(arrays, nid)
    names = ("first", "middle", "last")
    dcol = {"first": "First", "middle": "Middle", "last": "Last"}
    items = [[int(i)] for i in rows] if ev_sets is None else ev_sets
    out = np.empty((len(items), len(opts)))
    for r, ev in enumerate(items):
        sk = logp.copy()
        for t in terms:
            name = lw.obs_cols[int(t["obs_col"])]
            # distinct observed values ascending by their index, each multiplicity x density; a single row: one value, once
            vals, mult = np.unique(S["obs"][int(t["obs_col"]), ev], return_counts=True)
            for o, c in zip(vals, mult):
                if o < 0:
                    continue
                i = next(e for e in ev if S["obs"][int(t["obs_col"]), e] == o)
                if t["dens_kind"] == _lib.DENS_NAME3:
                    i0 = ev[0]  # (the other two names: the latent row's own, which its evidence rows agree on)
                    v = np.array([R(d["Full"][i], *[s if n == attr else d[dcol[n]][i0] for n in names]) for s in ostr])
                else:
                    assert t["dens_kind"] == _lib.DENS_EQUAL and name == "p." + attr
                    v = np.array([0.0 if s == d[dcol[attr]][i] else NEG_INF for s in ostr])
                sk = sk + (v if ev_sets is None else np.float64(c) * v)
        out[r] = sk
    return out


@pytest.mark.parametrize("variant", ["middle", "last", "observed"])
def test_new_row_leaves_equal_the_restatement(worlds, oracle, variant):
    """all three option lists of a new Person row, every row: scores and log-marginals; the carrier's list holds the name3
    term, which reads the option's string and the row's own two other names"""
    S = worlds(variant)
    lw, hip = S["lw"], S["eng"].hip
    R = n3.Restated()
    rows = np.arange(S["n"], dtype=np.int32)
    carrier = "first" if variant == "observed" else variant
    n_kind = {}
    for nid in (1, 2, 3):
        attr = lw.blocks[0]["node_info"][nid]["attr"]
        want = _leaf_scores(S, R, nid, rows)
        lse, got, _ = hip.score_node(0, nid, rows, n_cand=want.shape[1], want_scores=True)
        assert np.array_equal(got, want), (attr, np.argwhere(got != want)[:5])
        for r in range(len(rows)):
            assert float(lse[r]) == fix_lse(oracle, want[r]), (attr, r)
        if attr == carrier:
            for v in (n3.LOG_THREE, n3.LOG_TWO, n3.NEITHER):
                n_kind[v] = sum(1 for key, val in R.memo.items() if val == v)
    assert min(n_kind.values()) >= 20, n_kind


# ---- 4. the Person plan against its evidence sets ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["middle", "last"])
def test_latent_plan_equals_the_restatement(worlds, oracle, variant):
    """every person with the rows that refer to it (1 to a dozen rows, repeated and missing full names among them): scores,
    log-marginals and the draw of every root of the Person plan; then one pclean_sweep_latent over the same sets, whose
    chosen fresh particles must hold the restated draws at their own Philox counters"""
    S = worlds(variant)
    lw, hip, tr = S["lw"], S["eng"].hip, S["trace"]
    R = n3.Restated()
    pl = lw.latent_plans["Person"]
    cur = np.asarray(tr.cur[0])
    t = tr.tables["Person"]
    sets = [np.flatnonzero(cur == k).astype(np.int32) for k in range(t.n)]
    keep = [k for k in range(t.n) if len(sets[k])]
    sets = [sets[k] for k in keep]
    assert len(sets) >= 250 and max(len(s) for s in sets) >= 8
    ev_rows = np.concatenate(sets).astype(np.int32)
    ev_off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int32)
    keys = np.array(keep, dtype=np.int32)
    hip.set_active_rows(0, -1)
    want_by_root = {}
    for node, attr in enumerate(pl["root_attr"]):
        want = _leaf_scores(S, R, node, None, ev_sets=[list(map(int, s)) for s in sets])
        hip.enum_launches(reset=True)
        lse, got, draws = hip.score_node_ev(pl["block_id"], node, keys, ev_off, ev_rows, n_cand=want.shape[1], want_scores=True,
                                            seed=91, sweep=4, n_draws=1)
        assert all(s.endswith("_ev") for s, c in hip.enum_launches().items() if c)
        assert np.array_equal(got, want), (attr, np.argwhere(got != want)[:5])
        site = (pl["block_id"] << 16) | node
        for r in range(len(sets)):
            assert float(lse[r]) == fix_lse(oracle, want[r]), (attr, r)
            assert int(draws[r]) == fix_draw(oracle, want[r], 91, int(keys[r]), site, 0, 4), (attr, r)
        want_by_root[node] = want
    cfg = InferenceConfig(1, 3, rejuv_frequency=500).as_c()
    excl = np.full((len(pl["roots"]), len(keys)), -1, dtype=np.int32)
    runs = [hip.sweep_latent(cfg, 91, 4, pl["block_id"], pl["roots"], keys, ev_off, ev_rows, None, excl, len(pl["nodes"]))
            for _ in range(2)]
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    chosen, vals = runs[0]
    n_fresh = 0
    for r in range(len(keys)):
        if chosen[r] == 0:
            continue
        n_fresh += 1
        for node, root in enumerate(pl["roots"]):
            sc = want_by_root[node][r]
            assert sc[vals[r, root]] > sc.max() - 28.5, (r, node)
            # the chosen fresh particle p holds the draw of (seed, latent row, site of the root, p, sweep)
            site = (pl["block_id"] << 16) | root
            assert int(vals[r, root]) == fix_draw(oracle, sc, 91, int(keys[r]), site, int(chosen[r]), 4), (r, node)
    assert n_fresh > 50


# ---- 5. observed sweeps: the term against a table of its restated values -----------------------------------------------------------
def test_observed_sweeps_equal_the_injected_restatement(worlds):
    """P = 1 and P = 6 on the tagged program (a never observed tag tells the Person rows apart): the same plan with both
    name3 terms turned into tabulated terms — observed value = the row's number (one more observed column), latent value =
    the candidate's tag on the slot, the option on the carrier's leaf, class = which restated value the pair has — must
    choose the same referents and particles with the same log-weights"""
    S = worlds("middle", tagged=True)
    lw, eng, tr, d = S["lw"], S["eng"], S["trace"], S["dirty"]
    n = S["n"]
    R = n3.Restated()

    def sweeps(e):
        out = []
        for P in (1, 6):
            choice, chosen, logml, new_rows = e.sweep(tr, InferenceConfig(1, P, rejuv_frequency=500), 13, 1)
            out.append((choice.copy(), chosen.copy(), logml.copy(), {b: (r.copy(), v.copy()) for b, (r, v) in new_rows.items()}))
        return out
    a = sweeps(eng)
    klass = {n3.LOG_THREE: 0, n3.LOG_TWO: 1, n3.NEITHER: 2, 0.0: 3}  # (3: the missing observation's column of T)
    T = [n3.LOG_THREE, n3.LOG_TWO, n3.NEITHER, 0.0]
    obs2 = np.vstack([S["obs"], np.arange(n, dtype=np.int32)[None, :]])
    eng2 = Engine(lw, obs2, dist_mode=1)
    try:
        eng2.upload_trace(tr)
        hip = eng2.hip
        cols, _ = tr.tables["Person"].view()
        ci = lw.colidx["Person"]
        tdom = lw.latent_dom[("Person", "tag")]
        doms = {k: lw.latent_dom[("Person", k)] for k in ("first", "middle", "last")}
        by_tag = {int(cols[ci["tag"], r]): tuple(doms[k].string(int(cols[ci[k], r])) for k in ("first", "middle", "last"))
                  for r in range(cols.shape[1])}
        assert len(by_tag) == cols.shape[1]  # one tag per row of the table
        croot = np.full((n, len(tdom)), 2, dtype=np.uint8)  # (a tag no row holds is never looked up)
        mopts = [doms["middle"].string(v) for v in range(len(doms["middle"]))]
        cleaf = np.empty((n, len(mopts)), dtype=np.uint8)
        for i in range(n):
            o = d["Full"][i]
            for tag, person in by_tag.items():
                croot[i, tag] = klass[R(o, *person)]
            cleaf[i] = [klass[R(o, d["First"][i], s, d["Last"][i])] for s in mopts]
        p_root, p_leaf = lw._next_pair, lw._next_pair + 1
        hip.set_pair_table(p_root, croot)
        hip.set_class_density(p_root, np.tile(T, (len(tdom), 1)))
        hip.set_pair_table(p_leaf, cleaf)
        hip.set_class_density(p_leaf, np.tile(T, (len(mopts), 1)))
        arrs = list(lw.block_arrays(0))
        terms = arrs[1].copy()
        is3 = np.flatnonzero(terms["dens_kind"] == _lib.DENS_NAME3)
        assert list(is3) == sorted(lw.name3_terms[0]) and len(is3) == 2
        for ti in is3:
            on_slot = ti == 0
            terms["dens_kind"][ti] = _lib.DENS_TABULATED
            terms["obs_col"][ti] = obs2.shape[0] - 1
            terms["cand_col"][ti] = ci["tag"] if on_slot else 0
            terms["pair_table"][ti] = p_root if on_slot else p_leaf
        hip.load_block(0, arrs[0], terms, *arrs[2:])
        b = sweeps(eng2)
    finally:
        eng2.close()
    moved = 0
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])
        assert set(x[3]) == set(y[3])
        for blk in x[3]:
            assert np.array_equal(x[3][blk][0], y[3][blk][0]) and np.array_equal(x[3][blk][1], y[3][blk][1])
        moved += int((x[0][0] != np.asarray(tr.cur[0])).sum())
    assert moved > 0  # (rows whose full name is another person's do move)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_loaded_plan_alone(worlds):
    S = worlds("middle")
    lw, eng, tr = S["lw"], S["eng"], S["trace"]
    hip = eng.hip
    cfg = InferenceConfig(1, 4, rejuv_frequency=500)
    err = lambda: hip.lib.pclean_last_error(hip.h)  # noqa: E731

    def sweep():
        choice, chosen, logml, _ = eng.sweep(tr, cfg, 21, 1)
        return choice.copy(), chosen.copy(), logml.copy()
    before = sweep()
    # a name3 term with a ctx slot
    arrs = list(lw.block_arrays(0))
    terms = arrs[1].copy()
    terms["ctx_slot"][0], terms["fn_table"][0] = 0, 0
    with pytest.raises(PCleanHipError, match="status -1: pclean_load_block: name3 term 0 with a ctx slot"):
        hip.load_block(0, arrs[0], terms, arrs[2], arrs[3], [0], [0])
    # the entry point: a term of another kind, tables of another shape, a positive constant
    spec = lw.name3_terms[0][0]
    args = lw.name3_call(spec)
    with pytest.raises(PCleanHipError, match="status -1: pclean_set_term_name3: term 1 of block 0 is not a name3 term"):
        hip.set_term_name3(0, 1, *args)
    with pytest.raises(PCleanHipError, match="status -1: pclean_set_term_name3: name3 term 0: the tables are"):
        hip.set_term_name3(0, 0, *args[:3], args[3][:-1], *args[4:])
    with pytest.raises(PCleanHipError, match="status -1: .*log-probabilities <= 0"):
        hip.set_term_name3(0, 0, *args[:-1], 0.5)
    # prior proposals
    with pytest.raises(PCleanHipError, match=r"name3 likelihood term \(FormatName\(first, middle, last\)\) under "
                                             r"use_dd_proposals = false"):
        eng.sweep(tr, InferenceConfig(1, 4, rejuv_frequency=500, use_dd_proposals=False), 21, 1)
    assert all(np.array_equal(x, y) for x, y in zip(before, sweep()))
    # a block loaded without pclean_set_term_name3 says so
    hip.load_block(0, *arrs)
    with pytest.raises(PCleanHipError, match="status -4: name3 term 0: its sources and tables are not set"):
        hip.score_node(0, 0, np.arange(4, dtype=np.int32), snew=np.zeros(4), n_cand=tr.tables["Person"].n + 1, want_scores=True)
    for ti, sp in lw.name3_terms[0].items():
        hip.set_term_name3(0, ti, *lw.name3_call(sp))
    assert all(np.array_equal(x, y) for x, y in zip(before, sweep()))


def test_a_product_leaf_with_the_term_takes_the_generic_kernels(worlds):
    """the carrier's option table as a full 2 x |middles| grid (what enum_product_kernel serves): with the name3 term on the
    leaf the launch is the generic kernels', and the scores are the restatement's, every option twice"""
    S = worlds("middle")
    lw, eng, tr, d = S["lw"], S["eng"], S["trace"], S["dirty"]
    hip = eng.hip
    cfg = InferenceConfig(1, 4, rejuv_frequency=500)
    before = eng.sweep(tr, cfg, 23, 1)
    nid = next(i for i, info in enumerate(lw.blocks[0]["node_info"]) if info["attr"] == "middle")
    mdom = lw.latent_dom[("Person", "middle")]
    nm = len(mdom)
    tid = lw.option_id[("Person", "middle")]
    logp = np.full(2 * nm, -np.log(2.0 * nm))
    rows = np.arange(64, dtype=np.int32)
    (ti, spec), = [(t, s) for t, s in lw.name3_terms[0].items() if t != 0]
    args = list(lw.name3_call(spec))
    try:
        hip.set_options_cols(tid, np.stack([np.repeat(np.arange(2, dtype=np.int32), nm), np.tile(np.arange(nm, dtype=np.int32), 2)]),
                             logp)
        args[1] = [c if k == _lib.NAME3_OBS else 1 for k, c in zip(args[0], args[1])]  # the option's value: column 1 now
        hip.set_term_name3(0, ti, *args)
        hip.enum_launches(reset=True)
        _, got, _ = hip.score_node(0, nid, rows, n_cand=2 * nm, want_scores=True)
        launched = {s for s, c in hip.enum_launches().items() if c}
        assert launched and not any(s.startswith("product") for s in launched), launched
        R = n3.Restated()
        for i in rows:
            o = d["Full"][i]
            one = np.array([0.0 if o is None else R(o, d["First"][i], mdom.string(v), d["Last"][i]) for v in range(nm)])
            want = logp + np.tile(one, 2) if o is not None else logp
            assert np.array_equal(got[i], want), i
    finally:
        hip.set_options(tid, lw.option_values[("Person", "middle")], eng.option_logp[("Person", "middle")])
        hip.set_term_name3(0, ti, *lw.name3_call(spec))
    after = eng.sweep(tr, cfg, 23, 1)
    assert all(np.array_equal(x, y) for x, y in zip(before[:3], after[:3]))
