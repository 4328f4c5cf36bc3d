"""Every launch variant of the generic enumeration (pclean_launch_enum, enum_kernels.hip) against the CPU oracle, bit for
bit, at shapes chosen for the launch ladder's thresholds (tests/enum_variants_program.py names them), with
pclean_debug_enum_launches saying which kernel instantiation each call ran:

  enum_node_kernel<256|1024, EV>      scores kept in LDS; both sides of its per-thread / batched scoring switch (n > BT)
  enum_node_big_kernel<256|1024, EV>  three recomputing passes
  enum_scores_kernel<EV>              the scores-first kernel of a split launch; both sides of 64 / 65 items, of 4 095 /
                                      4 096 candidates and, with evidence sets, of 2 047 / 2 048
  (enum_product_kernel's four instantiations: tests/test_gpu_product_kernel.py)

through the leaf (score_node(0, 1)), the reference slot with its new-row candidate (score_node(0, 0, excl=cur)) and
evidence sets (sweep_latent on A's plan, with and without PCLEAN_NO_FAST_EV=1).  The data keep the posteriors flat
(tests/test_enum_variants_cpu.py checks that on the oracle alone; the same conditions are asserted here on the oracle's
output before anything is compared): near-deterministic draws would hide a wrong prefix or a wrong owning lane.

Left out on purpose: enum_node_big_kernel<256, EV> (needs more than 65 536 latent items with evidence sets); the
chunking of launches beyond kMaxBlocks = 4 M items; PCLEAN_BIG_FEW_ITEMS, PCLEAN_BIG_FROM and PCLEAN_NO_WIDE_ENUM (read
once per process)."""
import time

import numpy as np
import pytest

import enum_variants_program as evp
import helpers
from pclean_amd._lib import InferConfig
from pclean_amd.engine import Engine, InferenceConfig

pytestmark = pytest.mark.gpu

MOVED = ("a threshold of pclean_launch_enum moved: move this shape to the new threshold (tests/enum_variants_program.py), "
         "do not loosen the assertion")


class Rig:
    """engine + mirrored oracle world of one program"""

    def __init__(self, oracle, S):
        self.S = S
        self.eng = Engine(S["lw"], S["obs"], dist_mode=0)
        try:
            self.eng.upload_trace(S["trace"])
            self.world = evp.oracle_world(oracle, helpers, S, self.eng)
        except Exception:
            self.eng.close()
            raise
        self.hip = self.eng.hip

    def close(self):
        self.eng.close()

    def counted(self, generic, call):
        """call() with the counters reset; returns (result, names of the slots that launched)"""
        self.hip.force_generic(generic)
        try:
            self.hip.enum_launches(reset=True)
            out = call()
            ran = {k for k, v in self.hip.enum_launches().items() if v > 0}
        finally:
            self.hip.force_generic(False)
        return out, ran


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: lse differs"
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), f"{what}: candidate scores differ"
    assert np.array_equal(got[2], want[2]), f"{what}: draws differ"


@pytest.mark.parametrize("n_options", sorted(evp.LEAF_SHAPES))
def test_leaf_variants(oracle, n_options):
    n_rows, calls = evp.LEAF_SHAPES[n_options]
    S = evp.leaf_program(n_options)
    rig = Rig(oracle, S)
    try:
        first = np.arange(64, dtype=np.int32)
        assert (evp.diversity(evp.oracle_leaf(rig.world, S, first, evp.N_DRAWS)[2]) >= 3).sum() >= 16
        for items, call, n_draws, slots in calls:
            what = f"{n_options} options, {items} items, {call}, {n_draws} draws"
            rows = np.arange(items, dtype=np.int32)
            sc = call == "scores"
            t0 = time.time()
            got, ran = rig.counted(not sc, lambda: rig.hip.score_node(0, 1, rows, seed=1, sweep=2, n_draws=n_draws,
                                                                     n_cand=n_options, want_scores=sc))
            dflt = rig.hip.score_node(0, 1, rows, seed=1, sweep=2, n_draws=n_draws, n_cand=n_options)
            t1 = time.time()
            # (the oracle on a fixed sample of the 65 537 rows: its draws are keyed by the row id)
            sample = rows if items <= 2048 else evp.big_sample(items)
            want = evp.oracle_leaf(rig.world, S, sample, n_draws, want_scores=sc)
            print(f"[{what}] ran {sorted(ran)}; device {t1 - t0:.2f} s, oracle on {len(sample)} rows {time.time() - t1:.2f} s")
            assert ran == slots, f"{what}: ran {sorted(ran)}, expected {sorted(slots)} — {MOVED}"
            assert np.isfinite(want[0]).all()
            same([None if a is None else a[sample] for a in got], want, what)
            same(dflt, (got[0], None, got[2]), what + ", default path against the generic kernels")
    finally:
        rig.close()


@pytest.mark.parametrize("n_latent,items,slots", evp.FK_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in evp.FK_SHAPES])
def test_reference_slot_variants(oracle, n_latent, items, slots):
    S = evp.fk_program(n_latent)
    rig = Rig(oracle, S)
    try:
        what = f"{n_latent} latent rows, {items} items"
        rows = evp.fk_items(n_latent, items)
        excl = S["trace"].cur[0, rows]
        want = evp.oracle_fk(rig.world, S, rows, excl)
        assert (evp.diversity(want[2]) >= 2).sum() * 4 >= items
        assert (want[2] < 0).any(), "the oracle never draws the new-row candidate"
        assert (want[2] == excl[:, None]).any(), "the oracle never keeps the current referent"

        def call():
            return rig.hip.score_node(0, 0, rows, excl=excl, seed=1, sweep=2, n_draws=evp.N_DRAWS, n_cand=n_latent + 1)
        got, ran = rig.counted(True, call)
        print(f"[{what}] ran {sorted(ran)}")
        assert ran == slots, f"{what}: ran {sorted(ran)}, expected {sorted(slots)} — {MOVED}"
        same(got, want, what)
        same(call(), got, what + ", compact-table path against the generic kernels")
    finally:
        rig.close()


@pytest.mark.parametrize("n_options,n_latent,must,must_not", evp.EV_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in evp.EV_SHAPES])
def test_evidence_set_variants(oracle, monkeypatch, n_options, n_latent, must, must_not):
    from pclean_amd.inference import build_evidence, latent_current_choices
    S = evp.ev_program(n_options, n_latent)
    lw, tr = S["lw"], S["trace"]
    rig = Rig(oracle, S)
    try:
        rig.hip.set_active_rows(0, -1)
        pl = lw.latent_plans["A"]
        live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "A")
        n_ev = np.diff(ev_off)
        assert len(live) == n_latent and n_ev.min() >= 1 and n_ev.max() > 64
        ran_all = set()
        for P, mh in evp.EV_CONFIGS:
            what = f"{n_options} options, {n_latent} latent rows, P = {P}"
            cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
            excl = latent_current_choices(lw, tr, "A", live, cfg)
            args = (9, 1, pl["block_id"], pl["roots"], live, ev_off, ev_rows, ev_ctx, excl, len(pl["nodes"]))
            want = rig.world.sweep_latent(InferConfig(1, P, 1, 1, int(mh), 50, 100), *args)
            assert (want[1][:, 0] != tr.tables["A"].cols[0, live]).sum() * 4 >= n_latent
            monkeypatch.setenv("PCLEAN_NO_FAST_EV", "1")
            got, ran = rig.counted(False, lambda: rig.hip.sweep_latent(cfg.as_c(), *args))
            monkeypatch.delenv("PCLEAN_NO_FAST_EV")
            print(f"[{what}] with PCLEAN_NO_FAST_EV ran {sorted(ran)}")
            ran_all |= ran
            assert not (must_not & ran), f"{what}: ran {sorted(ran)}, expected none of {sorted(must_not)} — {MOVED}"
            assert not any(not k.endswith("_ev") for k in ran), f"{what}: a launch without evidence sets ({sorted(ran)})"
            assert np.array_equal(got[0], want[0]), f"{what}, generic kernels: chosen particle"
            assert np.array_equal(got[1], want[1]), f"{what}, generic kernels: sampled values"
            fast = rig.hip.sweep_latent(cfg.as_c(), *args)
            assert np.array_equal(fast[0], want[0]), f"{what}, default path: chosen particle"
            assert np.array_equal(fast[1], want[1]), f"{what}, default path: sampled values"
        # (a launch holds the rows that take a fresh particle: of 1 100 rows all under MH with 2 particles, ~5/6 with 6)
        assert must <= ran_all, f"{n_options} options, {n_latent} latent rows: ran {sorted(ran_all)}, expected {sorted(must)} — {MOVED}"
    finally:
        rig.close()
