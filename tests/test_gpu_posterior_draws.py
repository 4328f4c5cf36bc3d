"""The device sweep's draws against EXACT posteriors (tests/posterior_exact.py: the literal interpreter's scores and
the closed forms of one batched sweep).  Parity with the oracle cannot show that what both compute samples the right
distribution; these cases can: a mis-weighted retained particle, an inverted MH ratio, a Philox counter without the
sweep index or a draw off by one fail them while every parity test stays green.

One frozen trace per program, S sweeps with sweep_idx = 0..S-1 and nothing committed: S independent draws per row,
pooled over rows into one G-test per case; logml of the first sweep against the exact log-marginal within the
quantisation bound of include/pclean_detmath.h.  Programs (posterior_exact.PROGRAMS): draw_program below 1024 latent
rows (the generic enum_node_kernel) and above (the fast root path: three-term pre-filter, fk_root_wave_kernel,
the flat rows re-run by the overflow kernel, lazy draws of the last block), with dead rows below the high-water mark
and kpad % 64 != 0.  Cases: every particle count at an edge of the DISPATCH_PMAX buckets; a spread-row case with
SPREAD_SWEEPS draws per row (the power to see a 0.1-nat shift of a near candidate, which the all-row cases at S_GPU
do not have); rows without a current referent (cur = -1, no retained particle); latent sweeps of A's own choice
against its evidence sets (latent.hip's own final pick and MH ratio); MH over two dependent blocks; PG with 3, 9 and
33 particles over the same two blocks, where the particles end with unequal weights and the final pick must be
proportional to them (posterior_exact.pg_two_blocks), with and without current referents.
tests/test_posterior_draws_cpu.py samples each of these cases with NumPy under mutations: the power self-test.

Not covered: rows that can draw a ProposalDummyValue (the weight correction changes the kernel: the programs have
none), and the hospital workload itself (helpers.truth_workload): its nested new rows have no enumerable closed form
here, so the two-block cases run on draw_program's two-block stand-in with the same dependence (block 1 reads block
0's value through a JuliaNode).  Resampling that fires inside a sweep (three or more blocks, or prior proposals) and
apply_ancestors_kernel stay pinned to the oracle only; tests/test_gpu_particle_primitives.py pins the primitive they
call to an exact restatement."""
import numpy as np
import pytest

import posterior_exact as pe
from pclean_amd.engine import Engine

pytestmark = pytest.mark.gpu

S_SWEEPS = pe.S_GPU
FAST = {"generic": 0, "fast": 1}


@pytest.fixture(scope="module", params=list(pe.PROGRAMS))
def prog(request):
    spec = dict(pe.PROGRAMS[request.param], fast=FAST[request.param])
    S = pe.draw_program(**pe.PROGRAMS[request.param])
    t = S["trace"].tables["A"]
    if spec["fast"]:
        assert t.n >= 1024 and ((t.n + 15) & ~15) % 64 != 0 and not t.live[:t.n].all()
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        eng.upload_trace(S["trace"])
        yield request.param, spec, S, pe.RowConditionals(S), pe.check_rows(S), eng
    finally:
        eng.close()


@pytest.mark.parametrize("P,mh", pe.PARTICLES, ids=[f"P{p}{'-MH' if m else ''}" for p, m in pe.PARTICLES])
def test_device_draws_follow_exact_posterior(prog, P, mh):
    name, spec, S, rc, rows, eng = prog
    res, dev, n_new = pe.one_block_case(eng, S, rc, rows, P, mh, S_SWEEPS, seed=9001 + P)
    rs = eng.hip.get_root_stats()
    print(f"\n[{name} P={P}{' MH' if mh else ''}] path fast={rs.fast} groups={rs.n_groups} settled={rs.resolved_groups} "
          f"overflow={rs.overflow_items} lazy={rs.lazy_entries} kpad={rs.kpad}; {pe.describe(res)}; "
          f"logml deviation {dev:.3f} of its bound")
    assert rs.fast == spec["fast"], "the case missed its kernel path"
    if spec["fast"]:
        assert rs.kpad % 64 != 0 and rs.overflow_items > 0 and (rs.lazy_entries > 0 or P == 1)
        assert rs.overflow_items < rs.n_items  # (the flat rows only: every other row stays on the wave kernel)
        # (resolved_groups stays 0: settling groups before the scan is opt-in, PCLEAN_RESOLVE_GROUPS, not the default)
    assert n_new > 0 or P == 1  # the new-row branch was drawn and its records filled
    assert res["p"] > pe.ALPHA, pe.describe(res)
    assert dev <= 1.0
    if P == 1:
        assert res["df"] == 0 and not np.isinf(res["G"])


@pytest.fixture(scope="module")
def two_block():
    """the two-block program, its literal conditionals (computed once for the MH and the PG cases) and its engine"""
    S = pe.draw_program(**pe.TWO_BLOCK)
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        eng.upload_trace(S["trace"])
        yield S, pe.RowConditionals(S), pe.two_block_rows(S), eng
    finally:
        eng.close()


def test_device_two_block_mh_follows_closed_form(two_block):
    """MH (P = 2) over two blocks, block 1 reading block 0's value through a JuliaNode: q(t) a(t) + [t == s] (1 - sum q a)
    with block 0 on the fast root path"""
    S, rc, rows, eng = two_block
    res = pe.two_block_case(eng, S, rc, rows, S_SWEEPS, seed=77)
    rs = eng.hip.get_root_stats()
    print(f"\n[two blocks MH] block 0 path fast={rs.fast}; {pe.describe(res)}")
    assert rs.fast == 1
    assert res["p"] > pe.ALPHA, pe.describe(res)


@pytest.mark.parametrize("P", pe.TWO_BLOCK_PG)
def test_device_two_block_pg_follows_closed_form(two_block, P):
    """PG with P > 2 over the same two blocks: the particles end with unequal weights exp(Z1(x_p)) and the final pick is
    proportional to them (posterior_exact.pg_two_blocks) — the normal state of a hospital sweep"""
    S, rc, rows, eng = two_block
    res = pe.two_block_case(eng, S, rc, rows, S_SWEEPS, seed=1300 + P, P=P, mh=False)
    rs = eng.hip.get_root_stats()
    print(f"\n[two blocks PG P={P}] block 0 path fast={rs.fast}; {pe.describe(res)}")
    assert rs.fast == 1
    assert res["p"] > pe.ALPHA, pe.describe(res)


def test_device_two_block_pg_without_current_referent():
    """cur = -1 in both blocks: no retained particle, P q(t) z(t0) E[1 / (z(t0) + S_{P-1})]"""
    S = pe.draw_program(**pe.TWO_BLOCK)
    rows = pe.two_block_free_rows(S)
    assert len(rows) >= 40
    pe.free_rows(S, rows, blocks=(0, 1))
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        eng.upload_trace(S["trace"])
        res = pe.two_block_case(eng, S, pe.RowConditionals(S), rows, S_SWEEPS, seed=1400, P=3, mh=False)
        rs = eng.hip.get_root_stats()
    finally:
        eng.close()
    print(f"\n[two blocks PG cur=-1 P=3] block 0 path fast={rs.fast}; {pe.describe(res)}")
    assert rs.fast == 1
    assert res["p"] > pe.ALPHA, pe.describe(res)


def test_device_spread_rows_have_power(prog):
    """the rows with a near candidate, SPREAD_SWEEPS sweeps: the case whose power the self-test measures"""
    name, spec, S, rc, _, eng = prog
    rows = pe.spread_rows(S, rc)
    assert len(rows) >= 20
    res, dev, _ = pe.one_block_case(eng, S, rc, rows, pe.SPREAD_P, False, pe.SPREAD_SWEEPS, seed=4242)
    print(f"\n[{name} spread rows x{len(rows)}, P={pe.SPREAD_P}, S={pe.SPREAD_SWEEPS}] {pe.describe(res)}")
    assert res["p"] > pe.ALPHA, pe.describe(res)


@pytest.mark.parametrize("name", list(pe.PROGRAMS))
def test_device_draws_without_current_referent(name):
    """cur = -1 (initialize_trace): no retained particle, the output is pi for every P"""
    S = pe.draw_program(**pe.PROGRAMS[name])
    tr, kind = S["trace"], S["kind"]
    t = tr.tables["A"]
    free = [i for i in range(len(kind)) if (kind[i] == "flat" and i % 2 == 0) or (kind[i] == "peaked" and i % 3 == 0)]
    for i in free:
        t.counts[tr.cur[0, i]] -= 1
        tr.cur[0, i] = -1
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        eng.upload_trace(tr)
        res, dev, _ = pe.one_block_case(eng, S, pe.RowConditionals(S), np.array(free), 3, False, S_SWEEPS, seed=7)
        rs = eng.hip.get_root_stats()
    finally:
        eng.close()
    print(f"\n[{name} cur=-1 P=3] path fast={rs.fast}; {pe.describe(res)}; logml deviation {dev:.3f} of its bound")
    assert rs.fast == FAST[name]
    assert res["p"] > pe.ALPHA, pe.describe(res)
    assert dev <= 1.0


@pytest.mark.parametrize("P,mh", [(2, False), (2, True), (9, False), (33, False)], ids=["P2-PG", "P2-MH", "P9", "P33"])
def test_device_latent_draws_follow_exact_posterior(prog, P, mh):
    """sweep_latent of A's own choice: the chosen particle is uniform (PG) / accepted with 0.5 / (1e-10 + 0.5) (MH),
    particle 0 keeps the current value, any other draws from LatentProposal's pi"""
    name, spec, S, rc, _, eng = prog
    eng.hip.set_profiling(True)
    try:
        res = pe.latent_case(eng, S, rc, P, mh, S_SWEEPS, seed=515 + P, every=1)
        prof = eng.hip.get_profile()
    finally:
        eng.hip.set_profiling(False)
    print(f"\n[{name} latent P={P}{' MH' if mh else ''}] phases {sorted(prof)}; {pe.describe(res)}")
    assert prof, "no latent kernel was recorded"
    assert res["p"] > pe.ALPHA, pe.describe(res)
