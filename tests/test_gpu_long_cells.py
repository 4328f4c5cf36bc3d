"""Sweeps over a 16-bit distance table (tests/long_cell_program.py: one cell longer than 255 characters switches its
column's pair table to elem_bytes == 2) against the CPU oracle, bit for bit.  Every scorer then takes its other load
branch: the generic enumeration (LDS-resident, wide, recomputing; with and without evidence sets), the compact-table
root launch declines, and pclean_ensure_density reallocates the nb / logl / atd tables with a new stride.
tests/test_long_cells_cpu.py shows that a scorer on the wrong branch would change the oracle's sweep on most rows.

Not covered: long strings under latent_dummy_correction=True (the elem_bytes branches of the two dummy-correction
kernels)."""
import copy

import numpy as np
import pytest

import helpers
import long_cell_program as lcp
from pclean_amd import _lib
from pclean_amd import inference as inf
from pclean_amd._lib import HipContext, InferConfig
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.trace import Trace
from test_gpu_edges import _oracle_sweep

pytestmark = pytest.mark.gpu

CONFIGS = [(True, 2), (False, 4)]  # (MH instead of PG, particles)


def _same_sweep(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: choices differ on rows {np.flatnonzero((a[0] != b[0]).any(axis=0))[:8]}"
    assert np.array_equal(a[1], b[1]), f"{what}: chosen particle differs"
    assert np.array_equal(a[2], b[2]), f"{what}: logml differs on rows {np.flatnonzero(a[2] != b[2])[:8]}"


def _check_tables(eng, oracle, lw):
    """note's table holds distances above 255 (16-bit), name's does not; both are the oracle's"""
    sym, off, _, _ = lw.pool.arrays()
    ids = lcp.pair_ids(lw)
    for f in ("name", "note"):
        pid, odom, ldom = ids[f]
        got = eng.hip.get_pair_table(pid, len(odom), len(ldom))
        assert np.array_equal(got, oracle.pair_table(sym, off, odom.id_array(), ldom.id_array(), eng.dist_mode)), f
        assert (got.max() > 255) == (f == "note")


# (tile, latent rows, the instantiation of the generic enumeration that scores the sweep).  pclean_launch_enum: workgroups
# of 1 024 threads up to 1 024 items (120 rows), of 256 beyond (1 080 rows); the recomputing kernel from 20 401 candidates
# (20 400 latent rows and the new-row candidate).  A threshold that moves: move the shape, do not loosen the assertion.
VARIANTS = [(1, None, "lds_1024"), (9, None, "lds_256"), (1, 20400, "big_1024")]


@pytest.mark.parametrize("tile,n_latent,root", VARIANTS, ids=[v[2] for v in VARIANTS])
def test_observed_sweep_reads_the_16bit_table(oracle, tile, n_latent, root):
    """pclean_sweep under MH and under PG with 4 particles == the oracle's sweep (choices, chosen particle, logml); the
    compact-table root launch did not run (root_launches: nothing), the generic enumeration did, in the named
    instantiation; forcing the generic kernels changes nothing."""
    S = lcp.long_cell_setup(tile=tile, n_latent=n_latent)
    lw, obs, tr = S["lw"], S["obs"], S["trace"]
    eng = Engine(lw, obs, dist_mode=_lib.DIST_DL)
    try:
        _check_tables(eng, oracle, lw)
        eng.upload_trace(tr)
        world = helpers.mirror_world(oracle, lw, obs, tr, eng)
        for mh, P in CONFIGS:
            what = f"{root}, {'MH' if mh else 'PG'} {P}"
            cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
            eng.hip.root_launches(reset=True)
            eng.hip.enum_launches(reset=True)
            got = eng.sweep(tr, cfg, 11, 0)
            rl, el = eng.hip.root_launches(), eng.hip.enum_launches()
            ran = {k for k, v in el.items() if v}
            print(f"[{what}] enum launches {sorted(ran)}, root launches {sorted(k for k, v in rl.items() if v)}")
            assert not any(rl.values()), f"{what}: the compact-table root launch ran on a 16-bit table: {rl}"
            assert ran == {root}, f"{what}: ran {sorted(ran)}"
            want = _oracle_sweep(oracle, world, InferConfig(1, P, 1, 1, int(mh), 50, 100), 11, 0, tr.cur)
            _same_sweep(got[:3], want, what)
            assert np.isfinite(want[2]).all()
            eng.hip.force_generic(True)
            forced = eng.sweep(tr, cfg, 11, 0)
            eng.hip.force_generic(False)
            _same_sweep(forced[:3], got[:3], what + ", generic kernels forced")
            print(f"[{what}] {int((got[0][0] != tr.cur[0]).sum())} of {obs.shape[1]} rows change their referent")
    finally:
        eng.close()


def test_latent_sweep_reads_the_16bit_table(oracle):
    """pclean_sweep_latent on Ent, evidence aggregated in LDS and by the global sort: the same sweep, and the oracle's"""
    from pclean_amd.inference import build_evidence, latent_current_choices
    S = lcp.long_cell_setup()
    lw, obs, tr = S["lw"], S["obs"], S["trace"]
    eng = Engine(lw, obs, dist_mode=_lib.DIST_DL)
    try:
        eng.upload_trace(tr)
        eng.hip.set_active_rows(0, -1)
        world = helpers.mirror_world(oracle, lw, obs, tr, eng)
        pl = lw.latent_plans["Ent"]
        live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "Ent")
        assert len(live) == lcp.N_ENT and np.diff(ev_off).min() == lcp.ROWS_PER
        for mh, P in CONFIGS:
            cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
            excl = latent_current_choices(lw, tr, "Ent", live, cfg)
            args = (11, 0, pl["block_id"], pl["roots"], live, ev_off, ev_rows, ev_ctx, excl, len(pl["nodes"]))
            want = world.sweep_latent(InferConfig(1, P, 1, 1, int(mh), 50, 100), *args)
            for sort in (False, True):
                eng.hip.global_evidence_sort(sort)
                eng.hip.enum_launches(reset=True)
                got = eng.hip.sweep_latent(cfg.as_c(), *args)
                ran = {k for k, v in eng.hip.enum_launches().items() if v}
                eng.hip.global_evidence_sort(False)
                print(f"[latent, mh={mh}, global sort={sort}] enum launches {sorted(ran)}")
                assert np.array_equal(got[0], want[0]), (mh, sort, "chosen particle")
                assert np.array_equal(got[1], want[1]), (mh, sort, "sampled values")
            assert ran and all(k.endswith("_ev") for k in ran), ran
    finally:
        eng.close()


@pytest.mark.parametrize("uniform_names", [False, True], ids=["names_string_prior", "names_uniform"])
def test_two_iterations_of_run_inference_end_in_the_oracles_trace(oracle, monkeypatch, uniform_names):
    """initialize_trace + two run_inference iterations (observed sweeps with the device commit enabled, latent sweeps of
    Ent) on the device == the same run on the oracle engine.  With name ~ StringPrior every sweep creates rows that hold the
    name's ProposalDummyValue (its atoms carry next to no prior mass), which the device commit refuses: those sweeps are
    committed on the host from the device's outputs.  With name ~ ChooseUniformly the sweeps are committed on the
    device and the following sweeps read the tables from the device-resident state."""
    from oracle_engine import OracleEngine
    from test_gpu_commit import _same_state
    monkeypatch.setattr(inf, "DEVICE_COMMIT", True)
    S = lcp.long_cell_setup(uniform_names=uniform_names)
    lw, obs = S["lw"], S["obs"]
    cfg = InferenceConfig(2, 4)
    out, committed = [], []
    eng = Engine(lw, obs, dist_mode=_lib.DIST_DL)
    commit = eng.sweep_commit_device

    def counted(*a, **k):  # (eng._dc does not outlive a reload of the engine: the lowered model grows with drawn dummy names)
        r = commit(*a, **k)
        committed.append(r is not None)
        return r
    monkeypatch.setattr(eng, "sweep_commit_device", counted)
    try:
        for e in (eng, OracleEngine(oracle, lw, obs, cached=True)):
            tr = Trace(lw, obs.shape[1], 3)
            inf.initialize_trace(e, tr, cfg, 5, max_batch=64)
            inf.run_inference(e, tr, cfg, 5)
            tr.check_consistency()
            out.append(copy.deepcopy(tr))
        print(f"[run_inference] sweeps committed on the device: {sum(committed)} of {len(committed)}; "
              f"{getattr(eng, '_dc_why', '')}")
    finally:
        eng.close()
    _same_state(out[0], out[1], "run_inference, device against the oracle engine")
    assert len(committed) == 2, "an observed sweep did not go through the device commit"
    # (a commit may also be refused for capacity: at least one of the two succeeds; with dummy names none does)
    assert any(committed) == uniform_names, f"committed on the device: {committed}"
    assert 2 <= out[0].tables["Ent"].n_live <= 3 * lcp.N_ENT


def test_density_tables_grow_with_the_long_table(oracle):
    """A context that builds name's table first has its density tables sized for 64 symbols; note's table then reallocates
    them with another stride.  It gives the sweep of a context that built them in the opposite order, and the tables agree
    with the oracle's AddTypos density at the new lengths."""
    S = lcp.long_cell_setup()
    lw, obs, tr = S["lw"], S["obs"], S["trace"]
    ids = lcp.pair_ids(lw)
    sym, off, _, _ = lw.pool.arrays()
    hip = HipContext(0)
    try:
        hip.load_strings(sym, off)
        hip.build_pair_table(ids["name"][0], ids["name"][1].id_array(), ids["name"][2].id_array(), 1)
        assert hip.get_density_tables()[2] == 64
        hip.build_pair_table(ids["note"][0], ids["note"][1].id_array(), ids["note"][2].id_array(), 1)
        mr, md, ml, nb, logl = hip.get_density_tables()
        assert ml >= 300 and md == ml and nb.shape == (mr + 1, md + 1)
        for Lw, d in ((300, 300), (257, 1), (64, 0)):
            l = nb[(Lw + 4) // 5, d]
            l -= logl[Lw] * d
            l -= 1.629048269010741 * d
            assert l == pytest.approx(oracle.add_typos(d, Lw), rel=1e-14, abs=1e-14), (Lw, d)
    finally:
        hip.close()
    sweeps = []
    order = list(lw.pair_id.items())
    first = {v[0]: k for k, v in ids.items()}
    try:
        for items in (order, order[::-1]):
            lw.pair_id = dict(items)
            eng = Engine(lw, obs, dist_mode=_lib.DIST_DL)
            try:
                assert eng.hip.get_density_tables()[2] >= 300
                eng.upload_trace(tr)
                sweeps.append((first[items[0][1][0]], eng.sweep(tr, InferenceConfig(1, 4), 11, 0)[:3]))
            finally:
                eng.close()
    finally:
        lw.pair_id = dict(order)
    assert {s[0] for s in sweeps} == {"name", "note"}
    _same_sweep(sweeps[0][1], sweeps[1][1], "tables built name first / note first")


# ---- the flat twins: own blocks over the long vocabulary ---------------------------------------------------------------------
def _definition_bound(want):
    """tests/test_gpu_own_product.py: _against_definition's bound (terms through the library's fp64 tables within 1e-10, the
    sum rounding at most 8 times at the magnitude of the result)"""
    return 1e-10 + 8 * np.finfo(np.float64).eps * np.abs(want)


def _own_checks(eng, tr, S, K, want, leaves, want_variant, seed=11, sweep=3, P=4):
    """score_own against the literal definition `want` [n][K] and its draws against the scores' inverse CDF; own_marginals
    against the definition on the scores; sweep_own: a row that moved holds the probe's draw of its chosen particle"""
    import own_marginal_program as omp
    from test_gpu_own_choice import _draws_from_scores, _site
    n = S["n_rows"]
    rows = np.arange(n, dtype=np.int32)
    eng.hip.set_active_rows(0, n)
    lse, sc, dr = eng.hip.score_own(0, 0, rows, seed=seed, sweep=sweep, n_draws=P, n_cand=K, want_scores=True)
    assert eng.hip.get_own_stats().variants == want_variant, "another own-block kernel ran"
    assert np.array_equal(np.isneginf(sc), np.isneginf(want)) and np.isfinite(lse).all()
    fin = np.isfinite(want)
    err = np.abs(sc[fin] - want[fin]) / _definition_bound(want[fin])
    print(f"[definition] {int(fin.sum())} finite scores, largest error / bound {float(err.max()):.3g}")
    assert (err <= 1.0).all()
    assert np.array_equal(dr, _draws_from_scores(eng.hip, sc, rows, seed, _site(0, 0), sweep, P)), "draws differ from the scores' inverse CDF"
    fixw = lambda d: eng.hip.debug_detmath(d)[2]  # noqa: E731
    want_opt, want_prob, u, U = omp.marginal_twin(sc, fixw, 3)
    got = eng.hip.own_marginals(0, 0, 3, n)
    assert np.array_equal(got[0], want_opt) and np.array_equal(got[1].view(np.uint64), want_prob.view(np.uint64))
    # the sweep: rows of the first half start with a value
    rng = np.random.default_rng(5)
    start = np.full((len(leaves), n), -1, dtype=np.int32)
    for li, k in enumerate(leaves):
        start[li, :n // 2] = rng.integers(k, size=n // 2)
    tr.own = start.copy()
    chosen, logml = eng.sweep_own(tr, InferenceConfig(1, P), seed, sweep)
    vals = tr.own.copy()
    assert np.isfinite(logml).all()
    joint = vals[0] if len(leaves) == 1 else vals[0] * leaves[1] + vals[1]
    kept = (np.arange(n) < n // 2) & (chosen == 0)
    assert np.array_equal(vals[:, kept], start[:, kept])
    assert (~kept).sum() >= n // 2 and np.array_equal(joint[~kept], dr[np.arange(n), chosen][~kept])
    return sc, lse


def test_flat_own_choice_over_the_long_vocabulary():
    """note ~ ChooseProportionally(notes, p); note_obs ~ AddTypos(note): pclean_score_own, pclean_own_marginals and
    pclean_sweep_own read the 16-bit table (own_block.hip's three load branches); scores against the literal interpreter's
    densities on the strings, and bit for bit against the twin's new-row leaf"""
    import own_choice_program as ocp
    import own_marginal_program as omp
    from pclean_amd.model import LoweredModel
    S = lcp.flat_long()
    K, n = len(S["choices"]["note"]), S["n_rows"]
    p = np.random.default_rng(31).dirichlet(np.ones(K))
    want = np.array([sc for sc, _ in omp.exact_rows(S, {"p": p}, "note")])
    lw, obs = ocp.lower(S)
    eng = Engine(lw, obs, dist_mode=1)
    T = lcp.flat_long_twin(S)
    lwt = LoweredModel(T["model"], T["query"], T["dirty"])
    engt = Engine(lwt, lwt.encode_observations(T["dirty"]), dist_mode=1)
    try:
        (pid, odom, ldom), = lw.pair_id.values()
        assert eng.hip.get_pair_table(pid, len(odom), len(ldom)).max() > 255
        tr = Trace(lw, n, 0)
        tr.params[("Obs", "p")].value = p
        eng.upload_trace(tr)
        sc, lse = _own_checks(eng, tr, S, K, want, [K], 1)
        trt = Trace(lwt, n, 0)
        trt.params[("A", "p")].value = p
        engt.upload_trace(trt)
        lse_t, sc_t, _ = engt.hip.score_node(0, 1, np.arange(n, dtype=np.int32), seed=11, sweep=3, n_draws=1, n_cand=K, want_scores=True)
        assert np.array_equal(sc.view(np.uint64), sc_t.view(np.uint64)), "scores differ from the twin's leaf"
        assert np.array_equal(lse.view(np.uint64), lse_t.view(np.uint64)), "lse differs from the twin's leaf"
    finally:
        eng.close()
        engt.close()


def test_flat_product_leaf_indexed_by_the_long_choice():
    """a ~ ChooseProportionally(notes, pa); b ~ ChooseProportionally(names, theta, index="a"): the product leaf whose index
    column reads the 16-bit table, against own_product_program.exact_matrix and the twin's product leaf"""
    import own_product_program as opp
    S = lcp.flat_long_product()
    na, nb, n = len(S["A"]), len(S["B"]), S["n_rows"]
    pa, th = opp.draw_params(S, 5)
    want = opp.exact_matrix(S, pa, th, np.arange(n))
    lw, obs = opp.lower(S)
    eng = Engine(lw, obs, dist_mode=1)
    lwt, obst, leaf = opp.twin(S)
    engt = Engine(lwt, obst, dist_mode=1)
    try:
        assert max(int(eng.hip.get_pair_table(pid, len(od), len(ld)).max()) for pid, od, ld in lw.pair_id.values()) > 255
        tr = Trace(lw, n, 0)
        tr.params[("Obs", "pa")].value, tr.params[("Obs", "theta")].value = np.asarray(pa, np.float64), np.asarray(th, np.float64)
        eng.upload_trace(tr)
        sc, lse = _own_checks(eng, tr, S, na * nb, want, [na, nb], 4)  # (4: the product leaf)
        trt = Trace(lwt, n, 0)
        trt.params[("Doc", "deg_p")].value, trt.params[("Doc", "theta")].value = np.asarray(pa, np.float64), np.asarray(th, np.float64)
        engt.upload_trace(trt)
        lse_t, sc_t, _ = engt.hip.score_node(leaf[0], leaf[1], np.arange(n, dtype=np.int32), seed=11, sweep=3, n_draws=1,
                                             n_cand=na * nb, want_scores=True)
        assert np.array_equal(sc.view(np.uint64), sc_t.view(np.uint64)), "scores differ from the twin's product leaf"
        assert np.array_equal(lse.view(np.uint64), lse_t.view(np.uint64)), "lse differs from the twin's product leaf"
    finally:
        eng.close()
        engt.close()
