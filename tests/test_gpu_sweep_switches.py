"""The switches of pclean_sweep (sweep.hip) that no other test sets.  Each one takes the sweep along another path that the
code's comments promise to be bit-identical (same Philox counters, same fp64 additions in the same order).  Read once per
process:

  PCLEAN_EAGER_NEW=1              every NEW slot of the last block is sampled before the final choice (no lazy lists, no
                                  fused final choice);
  PCLEAN_NO_PARTIAL_EAGER=1       ... where a dummy can be drawn, for every row instead of the flagged rows (no split final);
  PCLEAN_NO_FUSED_FINAL=1         particle_update_kernel + final_choice_kernel instead of particle_update_final_kernel;
  PCLEAN_ALWAYS_RESAMPLE=1        maybe_resample_kernel after the first block too (equal weights: it keeps every particle);
  PCLEAN_NO_PU_STAGE=1            particle_update_kernel reads the row-major draws directly, no LDS staging;
  PCLEAN_NO_COMPACT_PREFETCH=1    the later blocks' root tables refresh on the main stream, inside their own blocks;
  PCLEAN_LATE_COMPACT_PREFETCH=1  the side stream starts once block 0's kernels are queued, not at the first wait.

One fresh process per variant runs three workloads and prints one SHA-256 apiece over three sweeps' outputs (referents,
chosen particles, logml, new-row records) and the committed states, the technique of test_gpu_sweep_tail.py; every variant
must print the digests of the process without switches:

  * dummy_program.people_program(64) from an empty table at 5 and at 33 particles (PMAX 8 and 64; one block whose dummy
    can be drawn for some rows only: the fused, the split and the eager final choice are all within the switches' reach);
  * helpers.truth_workload(2000, 40, 11) at 20 particles from the generator's state: two blocks, context items, a
    resampling step, LDS staging.

A profiled fourth sweep (not digested) names the phases a process went through (pclean_get_profile): where a switch moves
work from one phase to another (new_row_sampling / new_row_sampling_chosen, resample) the switched process must show it, or
the comparison would compare a path with itself.  The other switches change launches inside one phase (the separate final
choice, the staging, the side stream): for them the digests are the whole check."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ["PCLEAN_EAGER_NEW", "PCLEAN_NO_PARTIAL_EAGER", "PCLEAN_NO_FUSED_FINAL", "PCLEAN_ALWAYS_RESAMPLE",
            "PCLEAN_NO_PU_STAGE", "PCLEAN_NO_COMPACT_PREFETCH", "PCLEAN_LATE_COMPACT_PREFETCH"]
WORKLOADS = ["people5", "people33", "truth20"]

SCRIPT = r'''
import hashlib, sys
import numpy as np
sys.path[:0] = [ROOT, ROOT + "/tests"]
import dummy_program as dp
import helpers
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import _after_commit
from pclean_amd.parallel import Comm, exchange_and_commit
from pclean_amd.trace import Trace

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

def run(name, lw, obs, tr, P):
    eng = Engine(lw, obs)
    h = hashlib.sha256()
    try:
        cfg = InferenceConfig(1, P)
        for sweep in range(3):
            eng.upload_trace(tr)
            out = eng.sweep(tr, cfg, 77, sweep)
            stats = eng.sweep_stats(tr)
            digest_outputs(h, out)
            exchange_and_commit(tr, eng.lw, Comm(), 0, out[0], stats, out[3], sweep_idx=sweep)
            _after_commit(eng, tr, 77)
            digest_state(h, tr)
        eng.upload_trace(tr)
        eng.hip.set_profiling(True)
        eng.sweep(tr, cfg, 77, 3)
        prof = eng.hip.get_profile()
        print("DIGEST", name, h.hexdigest(), ",".join("%s:%d" % (k, prof[k][1]) for k in sorted(prof)))
    finally:
        eng.close()

for P in (5, 33):
    m, q, dirty, lw, obs = dp.people_program(64)
    run("people%d" % P, lw, obs, Trace(lw, obs.shape[1], 0), P)
dirty, clean, lw, obs, tr = helpers.truth_workload(2000, 40, 11)
run("truth20", lw, obs, tr, 20)
'''


def _run(extra_env):
    """One fresh process under a time limit: {workload: (digest, {phase: recorded intervals})}; a non-zero exit status stops
    the test."""
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    env.update(extra_env)
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + SCRIPT], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    res = {}
    for line in out.stdout.splitlines():
        if line.startswith("DIGEST"):
            _, name, digest, phases = line.split()
            res[name] = (digest, {p.split(":")[0]: int(p.split(":")[1]) for p in phases.split(",")})
    assert sorted(res) == sorted(WORKLOADS), out.stdout[-3000:]
    return res


@pytest.fixture(scope="module")
def defaults():
    return _run({})


def test_the_defaults_take_the_fused_and_the_lazy_paths(defaults, capsys):
    """what the switches below turn off is on without them"""
    with capsys.disabled():
        for w in WORKLOADS:
            print(f"\n[sweep switches] defaults, {w}: {defaults[w][0]} | {defaults[w][1]}")
    for w in ("people5", "people33"):
        ph = defaults[w][1]
        # one block whose dummy a few rows can draw: the split final choice (flagged rows sampled eagerly, the others' chosen
        # particles afterwards), nothing to resample
        assert ph.get("new_row_sampling", 0) >= 1 and ph.get("dummy_value_weights", 0) >= 1 and "resample" not in ph, ph
        assert ph.get("new_row_sampling_chosen", 0) >= 1, ph
    ph = defaults["truth20"][1]
    # two blocks: equal weights behind block 0 (no resampling step), block 1 fused with the final choice (nothing sampled
    # before it, the chosen particles' new rows behind it)
    assert "resample" not in ph and "new_row_sampling" not in ph and ph.get("new_row_sampling_chosen", 0) >= 1, ph
    assert ph.get("ctx_items", 0) >= 1 and ph.get("particle_update", 0) == 2, ph


def _expect_path(switch, res, defaults):
    people, truth = res["people33"][1], res["truth20"][1]
    if switch == "PCLEAN_EAGER_NEW":  # every NEW slot before the final choice: nothing left for the chosen particles
        assert truth.get("new_row_sampling", 0) >= 1 and "new_row_sampling_chosen" not in truth, truth
        assert people.get("new_row_sampling", 0) >= 1 and "new_row_sampling_chosen" not in people, people
    elif switch == "PCLEAN_NO_PARTIAL_EAGER":  # the dummy's rows are not told apart: as eager for the people program
        assert people.get("new_row_sampling", 0) >= 1 and "new_row_sampling_chosen" not in people, people
        assert truth == defaults["truth20"][1], (truth, defaults["truth20"][1])  # (no dummy there: nothing changes)
    elif switch == "PCLEAN_ALWAYS_RESAMPLE":  # behind block 0 of two
        assert truth.get("resample", 0) == 1, truth


@pytest.mark.parametrize("switch", SWITCHES)
def test_a_switch_alone_leaves_the_sweeps_bit_identical(switch, defaults, capsys):
    res = _run({switch: "1"})
    with capsys.disabled():
        for w in WORKLOADS:
            print(f"\n[sweep switches] {switch}=1, {w}: {res[w][0]} | {res[w][1]}")
    assert {w: res[w][0] for w in WORKLOADS} == {w: defaults[w][0] for w in WORKLOADS}
    _expect_path(switch, res, defaults)
