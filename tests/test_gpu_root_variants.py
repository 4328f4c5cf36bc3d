"""Every path of the compact-table root launch (pclean_launch_root_fast, root_wave.hip) against the CPU oracle, bit for bit,
at shapes built for the ladder's thresholds (tests/root_variants_program.py names them; tests/test_root_variants_cpu.py
shows on the oracle and a NumPy model alone that every row kind takes the path it is named for), with what the library
reports saying that the path ran.  Per shape:

  (a) score_node of the reference slot against the oracle: log-marginals, draws and (want_scores) candidate scores, on
      the default path and with force_generic(True);
  (b) one whole sweep with 1 and with 6 particles against pco_sweep_batched: chosen referents, chosen particle, logml and
      new-row records — lazy draws, and in the shape of 4 096 groups and more the settle kernel and its work list.

What says that the path ran:
  * pclean_debug_root_launches: the fk_root_wave_kernel instantiation (<2> .. <16>), group_settle_kernel,
    worklist_pack_kernel, a scan that was given the lazy lists, overflow_lds_kernel;
  * get_root_stats: fast, n_terms, n_pre, the pre-filter columns, kpad % 64 != 0 (a partial last block), overflow_items ==
    the model's count, lazy_entries, resolved_groups (settled groups: only in the two shapes of 4 096 groups and more), fine_blocks against
    full_scans * kblk in the shape with more than 128 passing blocks (inequalities: which wave reuses which list depends on
    the grid);
  * root_flags: bit 0 (overflowed) and bit 1 (guess-and-refine) equal the model's, row by row.

Paths no counter can show have none — the hot kernel is not instrumented; the CPU model proves that the inputs force them,
and the bit-equality then covers them:
  * the SPP switch between by-term and per-lane scoring: few(SPP) / few(SPP + 1) rows have exactly that many survivors at
    every cut-off a wave can scan;
  * the retry without WAVE_SLACK: the slack rows have more than 256 survivors with the slack and 200 without;
  * the widening count: refine_wide rows have nothing within the first two cut-offs;
  * the descriptor-scored sole survivor: peaked rows (one survivor, the current referent, not in refine mode);
  * the `same`-descriptor and cached-list shortcuts: twin rows (100 identical rows: a group cut into pieces when the
    launch is not lazy; a second referent with the same pre-filter values);
  * dense_skip: every group of the dense shape has three blocks in four passing;
  * saturated bytes in either scoring scheme: far rows (from five terms on).

Left out on purpose: terms with a ctx slot (the hospital parity tests hold them); evidence-set mode
(pclean_launch_ev_leaf); PCLEAN_RESOLVE_GROUPS (opt-in and off: resolved_draws stays 0); the environment switches read
once per process; n_pre = 0 (try_fast_root drops the pre-filter only when the smallest cost of an edit over the density
tables is not a positive finite number, which no lowering reachable from Python produces: the tables are the
negative-binomial ones for every model).

Three shapes (root_variants_program.SPARE) are swept once more on a table uploaded with spare capacity (the device-resident
commit's upload): the scans stop at the 64-aligned high-water mark, kscan < kpad.  The path assertions are made on the
sweeps that draw (6 particles): with one particle a row that has a referent keeps it."""
import copy
import time

import numpy as np
import pytest

import helpers
import root_variants_program as rvp
from pclean_amd.engine import Engine, InferenceConfig
from test_gpu_sweep import oracle_sweep

pytestmark = pytest.mark.gpu

MOVED = ("a threshold of pclean_launch_root_fast moved: move this shape to the new threshold (tests/root_variants_program.py), "
         "do not loosen the assertion")


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: lse differs"
    if want[1] is not None and got[1] is not None:
        assert np.array_equal(got[1], want[1]), f"{what}: candidate scores differ"
    assert np.array_equal(got[2], want[2]), f"{what}: draws differ"


def same_sweep(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: chosen referents differ"
    assert np.array_equal(got[1], want[1]), f"{what}: chosen particle differs"
    assert np.array_equal(got[2], want[2]), f"{what}: logml differs"
    assert set(got[3]) == set(want[3]), f"{what}: new-row records of other blocks"
    for b in got[3]:
        assert np.array_equal(got[3][b][0], want[3][b][0]) and np.array_equal(got[3][b][1], want[3][b][1]), f"{what}: new-row records"


@pytest.mark.parametrize("name", sorted(rvp.SHAPES))
def test_root_variants(oracle, name):
    t0 = time.time()
    S = rvp.build(name, oracle, helpers)
    lw, tr, T = S["lw"], S["trace"], S["n_terms"]
    n = S["obs"].shape[1]
    n_ent = tr.tables["Ent"].n
    wave = f"wave_{rvp.variant(T)}"
    eng = Engine(lw, S["obs"], dist_mode=0)
    try:
        eng.upload_trace(tr)
        hip = eng.hip
        hip.set_timed_block(0)
        world = rvp.oracle_world(oracle, helpers, S, eng)
        rows = rvp.sample_rows(S)
        kind, cur = S["kind"][rows], tr.cur[0, rows]
        E = rvp.expected_paths(S, oracle, helpers, rows=rows, world=world, tables=hip.get_density_tables())
        rvp.check_paths(name, S, E, kind)
        t1 = time.time()
        # ---- (a) score_node against the oracle
        want = rvp.oracle_root(world, S, rows, cur, want_scores=True)
        rvp.check_draws(name, S, kind, cur, want[2])
        t2 = time.time()

        def call(**kw):
            return hip.score_node(0, 0, rows, excl=cur, seed=1, sweep=2, n_draws=rvp.N_DRAWS, n_cand=n_ent + 1, **kw)
        hip.root_launches(reset=True)
        got = call()
        ran_a = {k: v for k, v in hip.root_launches(reset=True).items() if v}
        same(got, (want[0], None, want[2]), f"{name}, compact-table path")
        assert ran_a.get(wave, 0) >= 1 and all(k == wave or not k.startswith("wave_") for k in ran_a), f"{name}: ran {ran_a} — {MOVED}"
        same(call(want_scores=True), want, f"{name}, with candidate scores")
        hip.force_generic(True)
        try:
            same(call(), (want[0], None, want[2]), f"{name}, generic kernels")
            assert not hip.root_launches(reset=True).get(wave), "force_generic took the compact-table path"
        finally:
            hip.force_generic(False)
        t3 = time.time()
        # ---- (b) whole sweeps against the oracle
        n_nodes = [len(b["nodes"]) for b in lw.blocks]
        # the settle kernel takes launches of 4 096 groups and more (rows with the same observed tuple and referent are one group)
        n_groups = len(np.unique(np.concatenate([S["obs"], tr.cur[:1]]), axis=1).T)
        groups = n_groups >= rvp.SETTLE_MIN_GROUPS
        assert groups == (name in ("groups", "blocks")), f"{name}: {n_groups} groups"
        for P in (1, 6):
            cfg = InferenceConfig(1, P)
            hip.root_launches(reset=True)
            got = eng.sweep(tr, cfg, 11, 0)
            ran = {k: v for k, v in hip.root_launches(reset=True).items() if v}
            rs = hip.get_root_stats()
            same_sweep(got, oracle_sweep(oracle, world, cfg, 11, 0, tr.cur, n_nodes), f"{name}, sweep with {P} particles")
            stats = {f: getattr(rs, f) for f in ("fast", "n_items", "n_groups", "n_cand", "kpad", "n_terms", "n_pre", "n_draws",
                                                 "overflow_items", "full_scans", "fine_blocks", "scored_terms", "resolved_groups",
                                                 "lazy_entries")}
            print(f"[{name}, P = {P}] ran {ran}; {stats}")
            what = f"{name}, P = {P}: ran {ran}, {stats} — {MOVED}"
            assert rs.fast == 1 and rs.n_terms == T and rs.n_pre == E["n_pre"] and rs.n_cand == n_ent, what
            assert ran.get(wave, 0) >= 1 and all(k == wave or not k.startswith("wave_") for k in ran), what
            if P == 1:  # (one particle: the retained one where a row has a referent; the path assertions are made on the sweep that draws)
                continue
            flags = hip.root_flags(n)
            assert rs.kpad == E["kpad"] and rs.kpad % 64 != 0, what
            pre_cols = [rvp.root_terms(S)[p][0] for p in E["pre"]]
            assert list(rs.pre_obs_col)[:rs.n_pre] == pre_cols, what
            assert "resolved_draws" not in ran, what
            # (the work list is kept while most groups settle: the shape of many peaked groups; elsewhere the library may drop it)
            assert ("settle" in ran) == groups and ("worklist_pack" in ran or name != "groups") and (groups or "worklist_pack" not in ran), what
            assert (rs.resolved_groups > 0) == groups, what
            assert (rs.n_groups >= rvp.SETTLE_MIN_GROUPS) == groups, what
            assert rs.overflow_items == int(E["overflow"].sum()), what
            # (overflow_lds_kernel is launched whenever the candidates fit its LDS, with or without items: that it re-ran the
            # right items is shown by overflow_items and the flags below, not by its launch count)
            assert "lazy" in ran and rs.lazy_entries > 0, what
            assert np.array_equal((flags[rows] & 1) != 0, E["overflow"]), f"{what}: overflow flags differ from the model at rows " \
                f"{rows[((flags[rows] & 1) != 0) != E['overflow']][:10]}"
            assert np.array_equal((flags[rows] & 2) != 0, E["refine"]), f"{what}: refine flags differ from the model at rows " \
                f"{rows[((flags[rows] & 2) != 0) != E['refine']][:10]}"
            if name == "blocks":
                # the streamed group reads every block in every scan of its own, the other never does.  The counters are sums
                # over all groups, so this is a sanity check; the evidence that both sides of WAVE_BLK_CAP run is the model's
                # n_pass_blocks (137 for block_a, 101 for block_b: check_paths)
                assert E["kblk"] <= rs.fine_blocks < rs.full_scans * E["kblk"], what
        t4 = time.time()
        # ---- the same sweep on a table uploaded with spare capacity (the device-resident commit's upload): the scans stop at
        # the high-water mark, kscan = 64-aligned n_used < kpad, and the spare rows are dead candidates
        if name in rvp.SPARE:
            tr2 = copy.deepcopy(tr)
            assert eng.enable_device_commit(tr2), getattr(eng, "_dc_why", "")
            cfg = InferenceConfig(1, 6)
            hip.root_launches(reset=True)
            got = eng.sweep(tr2, cfg, 11, 0)
            ran = {k: v for k, v in hip.root_launches(reset=True).items() if v}
            rs = hip.get_root_stats()
            flags = hip.root_flags(n)
            what = (f"{name}, spare capacity: ran {ran}, n_cand {rs.n_cand}, scanned {rs.kpad}, overflow_items {rs.overflow_items}, "
                    f"full_scans {rs.full_scans}, fine_blocks {rs.fine_blocks}, resolved_groups {rs.resolved_groups} — {MOVED}")
            print(f"[{what}]")
            same_sweep(got, oracle_sweep(oracle, world, cfg, 11, 0, tr.cur, n_nodes), f"{name}, sweep on the table with spare capacity")
            assert rs.fast == 1 and rs.n_cand > n_ent and ran.get(wave, 0) >= 1, what
            assert rs.kpad == (n_ent + 63) & ~63 and rs.kpad < (rs.n_cand + 15) & ~15, what  # (kscan < kpad)
            assert ("settle" in ran) == groups and (rs.resolved_groups > 0) == groups, what
            assert rs.overflow_items == int(E["overflow"].sum()), what
            assert np.array_equal((flags[rows] & 1) != 0, E["overflow"]) and np.array_equal((flags[rows] & 2) != 0, E["refine"]), what
        print(f"[{name}] {n} rows ({len(rows)} compared per candidate), {n_ent} entities: model {t1 - t0:.1f} s, oracle scores "
              f"{t2 - t1:.1f} s, score_node x3 {t3 - t2:.1f} s, two sweeps and their oracle {t4 - t3:.1f} s, spare capacity "
              f"{time.time() - t4:.1f} s; score_node ran {ran_a}")
    finally:
        eng.close()


def test_leaf_variant(oracle):
    """The option list as the root launch takes it: res_new = n_cand - 1, no new-row score, no prior_e.  What the library
    reports for a leaf: the launch counters (score_node and the sweeps) and the number of items the overflow re-run took
    (get_timing().reserved).  The root statistics and root_flags describe block 0's ROOT launch alone — here the
    reference slot of a 64-row table, which the generic kernel scores — so fast, n_terms, n_pre, kpad, lazy_entries and
    the per-row flags cannot be read for a leaf: the model's overflow count is held against the re-run's item count, and
    the bit-equality of log-marginals, draws and scores covers the rest.  The compact-table launch on a leaf is reached through
    score_node; the sweeps of this program (1 and 6 particles) are held against the oracle, but they evaluate the list inside
    the new-row branch with the generic kernel (no compact-table launch is counted), so they pin no rung of the ladder."""
    S = rvp.leaf_program()
    lw, tr = S["lw"], S["trace"]
    n_opt = len(S["words"])
    eng = Engine(lw, S["obs"], dist_mode=0)
    try:
        eng.upload_trace(tr)
        hip = eng.hip
        world = rvp.oracle_world(oracle, helpers, S, eng)
        rows = np.arange(S["obs"].shape[1], dtype=np.int32)
        E = rvp.expected_paths(S, oracle, helpers, rows=rows, world=world, tables=hip.get_density_tables(), node_id=1)
        assert E["refine"].all() and E["certain"].all() and E["overflow"].any() and not E["overflow"].all()
        assert E["kpad"] % 64 != 0 and E["n_pre"] == 3
        want = world.score_node(0, 1, rows, seed=1, sweep=2, n_draws=rvp.N_DRAWS, n_cand=n_opt, want_scores=True)
        assert (rvp.diversity(want[2]) >= 3).sum() * 8 >= len(rows)

        def call(**kw):
            return hip.score_node(0, 1, rows, seed=1, sweep=2, n_draws=rvp.N_DRAWS, n_cand=n_opt, **kw)
        hip.root_launches(reset=True)
        got = call()
        ran = {k: v for k, v in hip.root_launches(reset=True).items() if v}
        rerun = hip.get_timing().reserved
        print(f"[leaf] {len(rows)} rows, {n_opt} options: ran {ran}, {rerun} items re-run; model: overflow {int(E['overflow'].sum())}, "
              f"schemes {sorted(set(E['scheme']))}")
        same(got, (want[0], None, want[2]), "leaf, compact-table path")
        assert ran.get("wave_4", 0) >= 1 and "overflow_lds" in ran and "settle" not in ran, f"leaf: ran {ran} — {MOVED}"
        assert rerun == int(E["overflow"].sum()), f"leaf: {rerun} items re-run, the model says {int(E['overflow'].sum())} — {MOVED}"
        same(call(want_scores=True), want, "leaf, with candidate scores")
        hip.force_generic(True)
        try:
            same(call(), (want[0], None, want[2]), "leaf, generic kernels")
        finally:
            hip.force_generic(False)
        n_nodes = [len(b["nodes"]) for b in lw.blocks]
        for P in (1, 6):
            cfg = InferenceConfig(1, P)
            hip.root_launches(reset=True)
            got = eng.sweep(tr, cfg, 11, 0)
            ran = {k: v for k, v in hip.root_launches(reset=True).items() if v}
            print(f"[leaf, sweep with P = {P}] ran {ran}; root statistics: fast {hip.get_root_stats().fast}")
            same_sweep(got, oracle_sweep(oracle, world, cfg, 11, 0, tr.cur, n_nodes), f"leaf program, sweep with {P} particles")
            # (printed, not asserted: in a sweep the option list is evaluated inside the new-row branch, marginal only and for
            # the groups that pass the gate — up to 1 024 items of that kind go to the generic kernel, and they do here)
    finally:
        eng.close()
