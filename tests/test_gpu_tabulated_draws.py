"""The tabulated likelihood terms (FormatName, ExpandOnShortVersion) through the device's sweeps against EXACT posteriors.

tests/test_gpu_tabulated_terms.py holds the per-candidate scores bit for bit against a restatement in the lowering's own
shape (T and class bytes); nothing there holds a DRAW.  Here posterior_exact.tab_draw_program is swept on the device and
every draw, new-row record and logml is held against the closed forms of tests/posterior_exact.py, whose pi comes from
oracle/literal.py on the strings themselves: a sweep that skipped the missing-observation column, exchanged two classes,
dropped -log(n) or read the class byte one column off fails these cases (tests/test_posterior_draws_cpu.py samples each
case under exactly those mutations) while the candidate it wrongs is merely less likely, not impossible.

Two sizes (posterior_exact.PROGRAMS_TAB): 300 latent rows, and 1090 with dead rows below the high-water mark — at 1024
candidates and more a node without tabulated terms takes the compact-table root path, and only the routing guards of
eval.hip keep the class bytes of a tabulated node from being read as edit distances; every case asserts the generic path
(root stats fast == 0), one contrast case that the same program with AddTypos terms in their place reports fast == 1.
At 1090 rows enum_node_kernel's candidate loop runs several chunks and candidate_score_batch its masked lanes.  Latent
sweeps (sweep_latent, build_evidence) run A's own choice against evidence sets of up to 62 rows, 60 of them without any
observation (the multiplicity-times-T branch of candidate_score_ev with the missing key).  A mixed sweep puts a second,
independent AddTypos block of 1100 rows next to the tabulated one: generic and compact-table roots in one pclean_sweep.
run_inference runs on tests/tabulated_program.py (StringPrior choices, dummy values) with the commit on the device and on
the host; after it the class tables and densities of the possibly grown domains equal the restatement.

Not covered: exact posteriors of rows that can draw a ProposalDummyValue below a tabulated term (tab_draw_program's root
class holds a single ChooseUniformly choice, which has none) and the empty name (see tab_draw_program)."""
import copy
import time

import numpy as np
import pytest

import posterior_exact as pe
import tabulated_program as tp
from pclean_amd import _lib
from pclean_amd import inference as inf
from pclean_amd.engine import Engine, InferenceConfig, class_density_rows
from pclean_amd.trace import Trace

pytestmark = pytest.mark.gpu

S_SWEEPS = pe.S_GPU


@pytest.fixture(scope="module", params=list(pe.PROGRAMS_TAB))
def prog(request):
    S = pe.tab_draw_program(**pe.PROGRAMS_TAB[request.param])
    t = S["trace"].tables["A"]
    if request.param == "large":
        assert t.n >= 1024 and ((t.n + 15) & ~15) % 64 != 0 and not t.live[:t.n].all()
    rc, rows = pe.RowConditionals(S), pe.check_rows(S)
    for i in rows:
        rc.block0(int(i))  # (memoised: the cases share the exact conditionals)
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        eng.upload_trace(S["trace"])
        yield request.param, S, rc, rows, eng, {}
    finally:
        eng.close()


@pytest.mark.parametrize("P,mh", pe.TAB_PARTICLES, ids=[f"P{p}{'-MH' if m else ''}" for p, m in pe.TAB_PARTICLES])
def test_tabulated_draws_follow_exact_posterior(prog, P, mh):
    name, S, rc, rows, eng, _ = prog
    t0 = time.perf_counter()
    res, dev, n_new = pe.one_block_case(eng, S, rc, rows, P, mh, S_SWEEPS, seed=7001 + P)
    rs = eng.hip.get_root_stats()
    print(f"\n[{name} P={P}{' MH' if mh else ''}] path fast={rs.fast} items={rs.n_items} candidates={rs.n_cand} terms={rs.n_terms}; "
          f"{pe.describe(res)}; logml deviation {dev:.3f} of its bound; {n_new} new-row records; {time.perf_counter() - t0:.1f} s")
    assert rs.fast == 0 and rs.n_terms == 3, "a node with tabulated terms left the generic kernels"
    assert rs.n_cand == S["trace"].tables["A"].n
    assert n_new > 0 or P == 1
    assert res["p"] > pe.ALPHA, pe.describe(res)
    assert dev <= 1.0
    if P == 1:
        assert res["df"] == 0 and not np.isinf(res["G"])


def test_addtypos_terms_in_their_place_take_the_fast_root():
    """the contrast that gives `fast == 0` above its meaning: the large program with name_obs and long_obs declared as
    AddTypos terms on the same references — same table, rows and observations — is routed to the compact-table path"""
    S = pe.tab_draw_program(**pe.PROGRAMS_TAB["large"], as_typos=True)
    assert not S["lw"].class_pairs
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        eng.upload_trace(S["trace"])
        eng.sweep(S["trace"], InferenceConfig(1, 2), 3, 0)
        rs = eng.hip.get_root_stats()
    finally:
        eng.close()
    assert rs.fast == 1 and rs.n_terms == 3 and rs.n_cand == S["trace"].tables["A"].n


@pytest.mark.parametrize("name", list(pe.PROGRAMS_TAB))
def test_tabulated_draws_without_current_referent(name):
    """cur = -1 on the flat rows and on every third initial row: no retained particle, the output is pi"""
    S = pe.tab_draw_program(**pe.PROGRAMS_TAB[name])
    free = pe.tab_free_rows(S)
    pe.free_rows(S, free)
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        eng.upload_trace(S["trace"])
        res, dev, _ = pe.one_block_case(eng, S, pe.RowConditionals(S), free, 3, False, S_SWEEPS, seed=17)
        rs = eng.hip.get_root_stats()
    finally:
        eng.close()
    print(f"\n[{name} cur=-1 P=3, {len(free)} rows] path fast={rs.fast}; {pe.describe(res)}; logml deviation {dev:.3f} of its bound")
    assert rs.fast == 0
    assert res["p"] > pe.ALPHA, pe.describe(res)
    assert dev <= 1.0


def test_tabulated_spread_rows(prog):
    """the initial rows (about twenty candidates of the initial class, CRP counts and -log(n) apart), SPREAD_SWEEPS sweeps"""
    name, S, rc, _, eng, _ = prog
    rows = pe.tab_spread_rows(S)
    assert len(rows) >= 20
    t0 = time.perf_counter()
    res, dev, _ = pe.one_block_case(eng, S, rc, rows, pe.SPREAD_P, False, pe.SPREAD_SWEEPS, seed=2424)
    print(f"\n[{name} initial rows x{len(rows)}, P={pe.SPREAD_P}, S={pe.SPREAD_SWEEPS}] {pe.describe(res)}; {time.perf_counter() - t0:.1f} s")
    assert eng.hip.get_root_stats().fast == 0
    assert res["p"] > pe.ALPHA, pe.describe(res)
    assert dev <= 1.0


@pytest.mark.parametrize("P,mh", pe.TAB_LATENT, ids=[f"P{p}{'-MH' if m else ''}" for p, m in pe.TAB_LATENT])
def test_tabulated_latent_draws_follow_exact_posterior(prog, P, mh):
    """sweep_latent of A's own choice against LatentProposal's pi: every FormatName / ExpandOnShortVersion / AddTypos
    observation of every referring row, the missing ones of the first two scored; the hub's evidence set holds 60 rows
    without any observation"""
    name, S, rc, _, eng, memo = prog
    if "latent" not in memo:
        live, ev_off, ev_rows, ev_ctx, excl = pe.latent_setup(S)
        assert int((ev_off[1:] - ev_off[:-1]).max()) > 60
        memo["latent"] = pe.latent_exact(S, rc, live, ev_off, ev_rows, np.arange(len(live)))
    eng.hip.set_profiling(True)
    t0 = time.perf_counter()
    try:
        res = pe.latent_case(eng, S, rc, P, mh, S_SWEEPS, seed=616 + P, every=1, exact=memo["latent"])
        prof = eng.hip.get_profile()
    finally:
        eng.hip.set_profiling(False)
    print(f"\n[{name} latent P={P}{' MH' if mh else ''}] phases {sorted(prof)}; {pe.describe(res)}; {time.perf_counter() - t0:.1f} s")
    assert prof, "no latent kernel was recorded"
    assert res["p"] > pe.ALPHA, pe.describe(res)


def test_mixed_sweep_generic_and_fast_roots():
    """The large program with a second, independent block `b ~ B; w ~ AddTypos(b.z)` over 1100 rows; rows without a current
    referent in either block, P = 3.  No particle is retained, so in block 0 every particle draws its referent from pi0
    and carries the weight Z0 — the same for all of them, whatever was drawn; resampling between the blocks therefore
    picks ancestors independently of their values, and block 1, which reads nothing of block 0, draws every particle's
    referent from pi1 with the weight Z0 + Z1, again the same for all.  The final pick is uniform and independent of the
    values: each block's marginal output is its own pi (and logml = Z0 + Z1).  One G-test per block; block 0 must report
    the generic path and block 1 the compact-table one, in the same pclean_sweep."""
    S = pe.tab_draw_program(**pe.TAB_MIXED)
    assert S["trace"].tables["B"].n >= 1024
    free = pe.tab_free_rows(S)
    pe.free_rows(S, free, blocks=(0, 1))
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        eng.upload_trace(S["trace"])
        t0 = time.perf_counter()
        (res0, res1), dev = pe.mixed_case(eng, S, pe.RowConditionals(S), free, 3, S_SWEEPS, seed=99)
        rs0 = eng.hip.get_root_stats()  # (root stats describe the timed block: 0 by default)
        eng.hip.set_timed_block(1)
        eng.sweep(S["trace"], InferenceConfig(1, 3), 99, S_SWEEPS)
        rs1 = eng.hip.get_root_stats()
    finally:
        eng.close()
    print(f"\n[mixed, {len(free)} rows, P=3] block 0 fast={rs0.fast} ({rs0.n_cand} candidates): {pe.describe(res0)}\n"
          f"block 1 fast={rs1.fast} ({rs1.n_cand} candidates): {pe.describe(res1)}; logml deviation {dev:.3f} of its bound; "
          f"{time.perf_counter() - t0:.1f} s")
    assert rs0.fast == 0 and rs0.n_cand == S["trace"].tables["A"].n
    assert rs1.fast == 1 and rs1.n_cand == S["trace"].tables["B"].n
    assert res0["p"] > pe.ALPHA, pe.describe(res0)
    assert res1["p"] > pe.ALPHA, pe.describe(res1)
    assert dev <= 1.0


def test_run_inference_on_the_tabulated_program(monkeypatch):
    """run_inference (observed and latent sweeps, relowering when a dummy's string joins a domain) on
    tests/tabulated_program.py, two iterations of 5 particles, committed on the device and on the host"""
    from test_gpu_commit import _same_state
    from test_gpu_tabulated_terms import _has_impossible_term
    out = []
    for dev in (True, False):
        monkeypatch.setattr(inf, "DEVICE_COMMIT", dev)
        S = tp.setup()
        lw, obs = S["lw"], S["obs"]
        sizes = {k: len(d) for k, d in lw.latent_dom.items()}
        eng = Engine(lw, obs, dist_mode=1)
        try:
            tr = Trace(lw, obs.shape[1], 3)
            cfg = InferenceConfig(2, 5)
            inf.initialize_trace(eng, tr, cfg, 5, max_batch=32)
            inf.run_inference(eng, tr, cfg, 5)
            tr.check_consistency()
            lw2 = eng.lw
            grown = {k: (sizes[k], len(d)) for k, d in lw2.latent_dom.items() if len(d) != sizes.get(k)}
            print(f"\n[run_inference, device commit {dev}] " + (f"domains grew: {grown}" if grown else "no domain grew in the two iterations"))
            cols, _ = tr.tables["Person"].view()
            nd, kd = lw2.latent_dom[("Person", "name")], lw2.latent_dom[("Person", "nick")]
            cn, ck = lw2.colidx["Person"]["name"], lw2.colidx["Person"]["nick"]
            for i, r in enumerate(tr.cur[0]):
                name, nick = nd.string(cols[cn, r]), kd.string(cols[ck, r])
                assert not _has_impossible_term(S, name, nick, i), (i, name, nick)
            assert lw2.class_pairs
            for pid, (rule, cls, T) in tp.term_tables(lw2).items():
                _, odom, ldom, options = lw2.class_pairs[pid]
                assert np.array_equal(eng.hip.get_pair_table(pid, len(odom), len(ldom)), cls), pid
                strings = [ldom.string(v) for v in range(len(ldom))]
                counts = eng.hip.count_short_versions(lw2.pool.add_all(options), ldom.id_array()) if options is not None else None
                assert np.array_equal(class_density_rows(rule, strings, options, counts), T), pid
            out.append(copy.deepcopy(tr))
        finally:
            eng.close()
    _same_state(out[0], out[1], "run_inference on the tabulated program, device vs host commit")
