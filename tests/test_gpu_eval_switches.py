"""The switches of eval_node (eval.hip) that no other test sets.  Each one takes the evaluation of a plan node along another
path that the code's comments promise to be bit-identical.  Read once per process:

  PCLEAN_NO_GROUP_GATE=1     the new-row branch of a compact-table reference slot is gated and evaluated per item
                             (gate_new_kernel, sub_items_kernel), not per group of identical rows (group_gate_kernel);
  PCLEAN_NO_COARSE_LEAF=1    cacheable option lists are enumerated, not drawn from the per-observed-value coarse prefix;
  PCLEAN_NO_FAST_OVERFLOW=1  the rows that overflow the survivor cap are counted, read back and re-run by the generic kernel
                             (no device list, no overflow_lds_kernel);
  PCLEAN_NO_EV_LIST=1        ... of an evidence-set scan: counted and re-run as a list of their own, no indirect launch;
  PCLEAN_LAZY_SPLIT=1        large groups are cut into pieces although the launch leaves lazy lists.

One fresh process per variant runs three workloads and prints one SHA-256 apiece over the sweeps' outputs and the committed
states (the technique of test_gpu_sweep_switches.py); every variant must print the digests of the process without switches.
PCLEAN_GATE_MIN=1 is set in every process, the default one included: the new-row gate takes lists of any length.

  * truth20: helpers.truth_workload(5000, 1100, 11) at 20 particles, three sweeps from the generator's state: block 0's slot
    has 1 100 candidates (the compact tables) and open children (the gate); lists are grouped from 4 096 items on, so
    the groups are made before the new-row branch;
  * t3: the program of shape t3 of root_variants_program at 6 particles, three sweeps: one block, so its root leaves lazy
    lists; cap rows overflow the survivor list; 100 twin rows are one large group.  Without the slack rows (their cut-off
    comes from the CPU model of the ladder, which this test has no use for) and with 2 600 entities: 4 096 rows and more;
  * ev2048: enum_variants_program.ev_program(2048, 50), sweep_latent on A's plan under both EV_CONFIGS: an option list of
    2 048 rows scored against evidence sets (the evidence scan).

A profiled further sweep (not digested) names the phases a process went through (pclean_get_profile), with the timed root's
statistics (get_root_stats) and the launch counters (root_launches, enum_launches) of that sweep.  The default process must
show the paths the switches turn off; a switched process must show the path it moved to wherever a phase or a statistic
can tell, or the comparison would compare a path with itself."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ["PCLEAN_NO_GROUP_GATE", "PCLEAN_NO_COARSE_LEAF", "PCLEAN_NO_FAST_OVERFLOW", "PCLEAN_NO_EV_LIST", "PCLEAN_LAZY_SPLIT"]
WORKLOADS = ["truth20", "t3", "ev2048"]

SCRIPT = r'''
import hashlib, sys
import numpy as np
sys.path[:0] = [ROOT, ROOT + "/tests"]
import enum_variants_program as evp
import helpers
import root_variants_program as rvp
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import _after_commit, build_evidence, latent_current_choices
from pclean_amd.parallel import Comm, exchange_and_commit

def digest_state(h, tr):
    h.update(np.ascontiguousarray(tr.cur).tobytes())
    for c in sorted(tr.tables):
        t = tr.tables[c]
        h.update(np.ascontiguousarray(t.counts[:t.n]).tobytes())
        h.update(np.ascontiguousarray(t.cols[:, :t.n]).tobytes())

def digest_outputs(h, out):
    choice, chosen, logml, new_rows = out
    for a in (choice, chosen, logml):
        h.update(np.ascontiguousarray(a).tobytes())
    for b in sorted(new_rows):
        h.update(np.ascontiguousarray(new_rows[b][0]).tobytes())
        h.update(np.ascontiguousarray(new_rows[b][1]).tobytes())

def report(name, h, hip, profiled):
    hip.set_profiling(True)
    hip.root_launches(reset=True)
    hip.enum_launches(reset=True)
    profiled()
    prof, rs, en = hip.get_profile(), hip.get_root_stats(), hip.enum_launches()
    stats = dict(pre_scored=rs.pre_scored, overflow_items=rs.overflow_items, n_groups=rs.n_groups, fast=rs.fast,
                 overflow_lds=hip.root_launches()["overflow_lds"], lazy=hip.root_launches()["lazy"], generic=sum(en.values()))
    print("DIGEST", name, h.hexdigest(), ",".join("%s:%d" % (k, prof[k][1]) for k in sorted(prof)),
          ",".join("%s:%d" % (k, stats[k]) for k in sorted(stats)))

def run(name, lw, obs, tr, P, **kw):
    eng = Engine(lw, obs, **kw)
    h = hashlib.sha256()
    try:
        cfg = InferenceConfig(1, P)
        eng.hip.set_timed_block(0)
        for sweep in range(3):
            eng.upload_trace(tr)
            out = eng.sweep(tr, cfg, 77, sweep)
            stats = eng.sweep_stats(tr)
            digest_outputs(h, out)
            exchange_and_commit(tr, eng.lw, Comm(), 0, out[0], stats, out[3], sweep_idx=sweep)
            _after_commit(eng, tr, 77)
            digest_state(h, tr)
        eng.upload_trace(tr)
        report(name, h, eng.hip, lambda: eng.sweep(tr, cfg, 77, 3))
    finally:
        eng.close()

def run_latent(name, S):
    lw, tr = S["lw"], S["trace"]
    eng = Engine(lw, S["obs"], dist_mode=0)
    h = hashlib.sha256()
    try:
        eng.upload_trace(tr)
        eng.hip.set_active_rows(0, -1)
        pl = lw.latent_plans["A"]
        live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "A")
        calls = []
        for P, mh in evp.EV_CONFIGS:
            cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
            excl = latent_current_choices(lw, tr, "A", live, cfg)
            calls.append((cfg.as_c(), 9, 1, pl["block_id"], pl["roots"], live, ev_off, ev_rows, ev_ctx, excl, len(pl["nodes"])))
        for sweep in range(2):
            for args in calls:
                for a in eng.hip.sweep_latent(*args)[:2]:
                    h.update(np.ascontiguousarray(a).tobytes())
        report(name, h, eng.hip, lambda: [eng.hip.sweep_latent(*args) for args in calls])
    finally:
        eng.close()

dirty, clean, lw, obs, tr = helpers.truth_workload(5000, 1100, 11)
run("truth20", lw, obs, tr, 20)
S = rvp.program(3, 3, tuple(k for k in rvp.ALL if k != "slack"), n_ent=2600)
assert S["obs"].shape[1] >= 4096
run("t3", S["lw"], S["obs"], S["trace"], 6, dist_mode=0)
run_latent("ev2048", evp.ev_program(2048, 50))
'''


def _run(extra_env):
    """One fresh process under a time limit: {workload: (digest, {phase: recorded intervals}, {statistic: value})}; a
    non-zero exit status stops the test."""
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    env["PCLEAN_GATE_MIN"] = "1"
    env.update(extra_env)
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    res = {}
    for line in out.stdout.splitlines():
        if line.startswith("DIGEST"):
            _, name, digest, phases, stats = line.split()
            res[name] = (digest,) + tuple({p.split(":")[0]: int(p.split(":")[1]) for p in part.split(",")} for part in (phases, stats))
    assert sorted(res) == sorted(WORKLOADS), out.stdout[-3000:]
    return res


@pytest.fixture(scope="module")
def defaults():
    return _run({})


def _show(what, res, capsys):
    with capsys.disabled():
        for w in WORKLOADS:
            print(f"\n[eval switches] {what}, {w}: {res[w][0]} | {res[w][1]} | {res[w][2]}")


def test_the_defaults_take_the_paths_the_switches_turn_off(defaults, capsys):
    _show("defaults", defaults, capsys)
    _, ph, st = defaults["truth20"]
    # block 0's slot: groups before the new-row branch, gated by group_gate_kernel (which scores the current referents);
    # the new rows' cacheable option lists are drawn from the coarse prefix
    assert ph.get("gate_new_branch", 0) >= 1 and st["pre_scored"] == 1 and st["fast"] == 1, (ph, st)
    assert ph.get("option_list_coarse_draw", 0) >= 1, ph
    _, ph, st = defaults["t3"]
    # cap rows: a device list of the overflowed items, re-run by overflow_lds_kernel; the root leaves lazy lists
    assert ph.get("overflow_rerun", 0) >= 1 and st["overflow_items"] > 0 and st["overflow_lds"] >= 1, (ph, st)
    assert st["fast"] == 1 and st["lazy"] >= 1, st
    _, ph, st = defaults["ev2048"]
    # the evidence scan, each with the indirect re-run of the items it could not settle behind it
    assert ph.get("evidence_option_scan", 0) >= 1 and ph.get("overflow_rerun", 0) == ph["evidence_option_scan"], ph


def _expect_path(switch, res, defaults):
    if switch == "PCLEAN_NO_GROUP_GATE":  # still gated, per item: no referent scores for the group descriptors
        _, ph, st = res["truth20"]
        assert ph.get("gate_new_branch", 0) >= 1 and st["pre_scored"] == 0 and st["fast"] == 1, (ph, st)
    elif switch == "PCLEAN_NO_COARSE_LEAF":  # the option lists are enumerated instead
        (_, ph, st), (_, ph0, st0) = res["truth20"], defaults["truth20"]
        assert "option_list_coarse_draw" not in ph and st["generic"] > st0["generic"], (ph, st, st0)
    elif switch == "PCLEAN_NO_FAST_OVERFLOW":  # the same items, after a count, by the generic kernel
        (_, ph, st), (_, ph0, st0) = res["t3"], defaults["t3"]
        assert ph.get("overflow_rerun", 0) >= 1 and st["overflow_items"] == st0["overflow_items"], (ph, st, st0)
        assert st["overflow_lds"] == 0 and st["generic"] > st0["generic"], (st, st0)
    elif switch == "PCLEAN_NO_EV_LIST":  # a re-run only behind the scans that left items, not behind every scan
        ph, ph0 = res["ev2048"][1], defaults["ev2048"][1]
        assert ph.get("evidence_option_scan", 0) == ph0["evidence_option_scan"], (ph, ph0)
        assert ph.get("overflow_rerun", 0) < ph0["overflow_rerun"], (ph, ph0)
    elif switch == "PCLEAN_LAZY_SPLIT":  # the twin rows' group in pieces, lazy lists all the same
        st, st0 = res["t3"][2], defaults["t3"][2]
        assert st["n_groups"] > st0["n_groups"] and st["lazy"] >= 1, (st, st0)


@pytest.mark.parametrize("switch", SWITCHES)
def test_a_switch_alone_leaves_the_evaluations_bit_identical(switch, defaults, capsys):
    res = _run({switch: "1"})
    _show(f"{switch}=1", res, capsys)
    assert {w: res[w][0] for w in WORKLOADS} == {w: defaults[w][0] for w in WORKLOADS}
    _expect_path(switch, res, defaults)
