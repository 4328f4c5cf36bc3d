"""The tail of the observed sweep (sweep.hip): finalize_tail_kernel — every block's finalize pass in one launch over
(workgroup, block), which also lists the rows whose chosen particle proposed a NEW referent, a workgroup walking a contiguous
range of 256-row tiles with one LDS histogram for all of them — against the launches it replaces.  Switches, read once per
process:

  PCLEAN_NO_FUSED_FINALIZE=1  chosen_new_kernel + one finalize_block_kernel per block (the parent's launches);
  PCLEAN_TAIL_WGS=<n>         workgroups per block of finalize_tail_kernel (1: one workgroup walks every tile; 3: the 47 tiles
                              of 12 000 rows split 16 / 16 / 15, a ragged last tile included);
  PCLEAN_NO_HIST=1            plain global atomics instead of the LDS histogram (as before).

Every result is a function of the row alone (integer sums; list positions that nobody reads as an order): all variants must
leave bit-identical outputs — one SHA-256 per fresh process over three sweeps' outputs (referents, chosen particles, logml,
new-row records) and the committed states, the technique of test_gpu_static_groups.py; a process that exits with a non-zero
status stops the test.

  * helpers.truth_workload(12000, 150, 11) from its own initialisation in batches of 4096, swept whole;
  * a 1 000-row table swept in windows of one row (Engine.sweep(lo, lo + 1) at rows 0, 256, 257, 999) and of 257 rows
    (observed_sweep(batch_rows=257): 257, 257, 257, 229);
  * the same three sweeps of the 12 000-row table through inference.observed_sweep with the device-resident commit, as
    bench.py runs it.

PCLEAN_TRACE_SYNC=1 shows the path a process took ("[pclean tail] ..." lines): the default process must have listed a chosen
NEW row through finalize_tail_kernel, the switched process must report the parent's kernels — or the comparison would
compare a path with itself."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = {"PCLEAN_NO_FUSED_FINALIZE": "1"}

PRELUDE = r'''
import hashlib, sys
import numpy as np
sys.path[:0] = [ROOT, ROOT + "/tests"]
import helpers
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import initialize_trace, observed_sweep
from pclean_amd.parallel import Comm, exchange_and_commit
from pclean_amd.trace import Trace

def digest_state(h, tr):
    h.update(np.ascontiguousarray(tr.cur).tobytes())
    for c in sorted(tr.tables):
        t = tr.tables[c]
        h.update(np.ascontiguousarray(t.counts[:t.n]).tobytes())

def digest_outputs(h, out):
    choice, chosen, logml, new_rows = out
    for a in (choice, chosen, logml):
        h.update(np.ascontiguousarray(a).tobytes())
    for b in sorted(new_rows):
        h.update(np.ascontiguousarray(new_rows[b][0]).tobytes())
        h.update(np.ascontiguousarray(new_rows[b][1]).tobytes())

def whole_sweeps(eng, tr, cfg, h):
    for sweep in range(3):
        eng.upload_trace(tr)
        out = eng.sweep(tr, cfg, 77, sweep)
        stats = eng.sweep_stats(tr)
        digest_outputs(h, out)
        exchange_and_commit(tr, eng.lw, Comm(), 0, out[0], stats, out[3])
        digest_state(h, tr)
'''

SCRIPT_WHOLE = PRELUDE + r'''
dirty, clean, lw, obs, _ = helpers.truth_workload(12000, 150, 11)
eng = Engine(lw, obs)
h = hashlib.sha256()
try:
    cfg = InferenceConfig(1, 20)
    tr = Trace(lw, obs.shape[1], 5)
    initialize_trace(eng, tr, cfg, 5, max_batch=4096)
    whole_sweeps(eng, tr, cfg, h)
    print("DIGEST", h.hexdigest(), {c: int(t.n_live) for c, t in tr.tables.items()})
finally:
    eng.close()
'''

SCRIPT_WINDOWS = PRELUDE + r'''
dirty, clean, lw, obs, _ = helpers.truth_workload(1000, 20, 11)
eng = Engine(lw, obs)
h = hashlib.sha256()
try:
    cfg = InferenceConfig(1, 20)
    tr = Trace(lw, obs.shape[1], 5)
    initialize_trace(eng, tr, cfg, 5, max_batch=4096)
    eng.upload_trace(tr)
    for lo in (0, 256, 257, 999):
        digest_outputs(h, eng.sweep(tr, cfg, 78, 0, lo, lo + 1))
    for sweep in range(3):
        changed = observed_sweep(eng, tr, cfg, 77, sweep, batch_rows=257)
        h.update(str(int(changed)).encode())
        digest_state(h, tr)
    print("DIGEST", h.hexdigest(), {c: int(t.n_live) for c, t in tr.tables.items()})
finally:
    eng.close()
'''

SCRIPT_DEVICE_COMMIT = PRELUDE + r'''
dirty, clean, lw, obs, _ = helpers.truth_workload(12000, 150, 11)
eng = Engine(lw, obs)
h = hashlib.sha256()
try:
    cfg = InferenceConfig(1, 20)
    tr = Trace(lw, obs.shape[1], 5)
    initialize_trace(eng, tr, cfg, 5, max_batch=4096)
    assert eng.enable_device_commit(tr), getattr(eng, "_dc_why", "")
    for sweep in range(3):
        changed = observed_sweep(eng, tr, cfg, 77, sweep)
        h.update(str(int(changed)).encode())
    digest_state(h, tr)
    print("DIGEST", h.hexdigest(), {c: int(t.n_live) for c, t in tr.tables.items()})
finally:
    eng.close()
'''

TAIL = re.compile(r"^\[pclean tail\] (.*)$", re.M)
LISTED = re.compile(r"(\d+) chosen NEW rows listed by (finalize_tail_kernel|chosen_new_kernel)")


def _run(script, extra_env):
    """One fresh process under a time limit; the test stops at the first non-zero exit status."""
    env = dict(os.environ)
    for k in list(PARENT) + ["PCLEAN_TAIL_WGS", "PCLEAN_NO_HIST"]:
        env.pop(k, None)
    env.update(extra_env)
    env["PCLEAN_TRACE_SYNC"] = "1"
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + script], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("DIGEST")][-1]
    tail = TAIL.findall(out.stderr)
    info = {
        "listed": [(int(a), b) for a, b in LISTED.findall(out.stderr)],
        "fused_finalize": any(t.startswith("finalize_tail_kernel:") for t in tail),
        "per_block_finalize": any(t.startswith("finalize_block_kernel:") for t in tail),
        "tiles_per_wg": sorted({t.split("at most ")[1] for t in tail if t.startswith("finalize_tail_kernel:")}),
    }
    return line.split()[1], line, info


def _compare(script, variants, capsys, tag):
    digests, infos = {}, {}
    for name, env in variants.items():
        digests[name], line, infos[name] = _run(script, env)
        i = infos[name]
        with capsys.disabled():
            print(f"\n[sweep tail, {tag}] {name}: {line} | chosen NEW {sorted(set(i['listed']))[:6]} | fused finalize "
                  f"{i['fused_finalize']} ({i['tiles_per_wg']})")
    assert len(set(digests.values())) == 1, digests
    return infos


def _check_default(i):
    assert i["fused_finalize"] and not i["per_block_finalize"], i
    assert i["listed"] and all(by == "finalize_tail_kernel" for _, by in i["listed"]), i["listed"]
    assert any(c > 0 for c, _ in i["listed"]), i["listed"]  # a chosen NEW row was listed there


def _check_parent(i):
    assert i["per_block_finalize"] and not i["fused_finalize"], i
    assert i["listed"] and all(by == "chosen_new_kernel" for _, by in i["listed"]), i["listed"]


def test_whole_sweeps_are_bit_identical_across_the_tail_paths(capsys):
    infos = _compare(SCRIPT_WHOLE, {
        "default": {},
        "per-block finalize": PARENT,
        "one workgroup": {"PCLEAN_TAIL_WGS": "1"},
        "three workgroups": {"PCLEAN_TAIL_WGS": "3"},
        "no histogram": {"PCLEAN_NO_HIST": "1"},
    }, capsys, "12 000 rows")
    _check_default(infos["default"])
    _check_parent(infos["per-block finalize"])
    # 47 tiles: one workgroup walks them all, three walk 16 / 16 / 15
    assert any(t.startswith("47 tiles") for t in infos["one workgroup"]["tiles_per_wg"]), infos["one workgroup"]["tiles_per_wg"]
    assert any(t.startswith("16 tiles") for t in infos["three workgroups"]["tiles_per_wg"]), infos["three workgroups"]["tiles_per_wg"]
    _check_default(infos["no histogram"])


def test_windows_of_257_rows_and_of_one_row_match_the_parents_launches(capsys):
    infos = _compare(SCRIPT_WINDOWS, {"default": {}, "per-block finalize": PARENT}, capsys, "1 000 rows in windows")
    _check_default(infos["default"])
    _check_parent(infos["per-block finalize"])
    # (a window of one row, and the 257-row windows' second tile of one row: one tile per workgroup)
    assert infos["default"]["tiles_per_wg"] == ["1 tiles per workgroup"], infos["default"]["tiles_per_wg"]


def test_observed_sweep_with_the_device_commit_matches_the_parents_launches(capsys):
    infos = _compare(SCRIPT_DEVICE_COMMIT, {"default": {}, "per-block finalize": PARENT}, capsys, "device-resident commit")
    _check_default(infos["default"])
    _check_parent(infos["per-block finalize"])
