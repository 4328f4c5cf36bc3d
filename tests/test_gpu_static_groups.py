"""Block 0's grouping from the static tuple order (eval.hip: make_item_groups_static) against the paths it replaces.

The observed sweep groups the rows of its first block by (observed tuple, current referent).  By default the groups now come
from a per-table static order of the rows, split by referent in every sweep; PCLEAN_NO_STATIC_GROUPS=1 restores the hash
table, PCLEAN_SORT_GROUPS=1 the radix sort, PCLEAN_NO_DEDUP=1 no grouping at all.  A group may be split, never merged, and
every result is a function of the item alone: all of them must leave bit-identical outputs (one SHA-256 over the chosen
referents, chosen particles, log marginal likelihood estimates, new-row records and the committed state of three sweeps +
commits, one fresh process per variant — the technique of test_gpu_determinism.py).

  * the determinism workload (helpers.truth_workload(40000, 400, 11)) swept whole;
  * the same workload with every sweep cut into windows (observed_sweep(batch_rows=...)): four windows (every one gets a
    cached order of its own) and nine (more than the cache holds: the last window falls back to the hash table);
  * a state whose referent is NOT a function of the observed tuple: eight distinct observed rows repeated 2000 times, the
    rows of one tuple spread over 41 referents — in stretches of the static order one referent per row (tiles of many
    classes), in others runs of 30 rows per referent (classes longer than 2 split_m = 24, cut into pieces); every tuple
    segment is far longer than a wavefront.

PCLEAN_TRACE_SYNC=1 (it only prints the blocking points) shows which grouping a process went through: the default processes
must have been through the static path — and, with nine windows, must have reported a window that the cache did not take
— or the comparison would compare a path with itself."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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

def whole_sweeps(eng, tr, cfg, h):
    for sweep in range(3):
        eng.upload_trace(tr)
        choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 77, sweep)
        stats = eng.sweep_stats(tr)
        for a in (choice, chosen, logml):
            h.update(np.ascontiguousarray(a).tobytes())
        for b in sorted(new_rows):
            h.update(np.ascontiguousarray(new_rows[b][0]).tobytes())
            h.update(np.ascontiguousarray(new_rows[b][1]).tobytes())
        exchange_and_commit(tr, eng.lw, Comm(), 0, choice, stats, new_rows)
        digest_state(h, tr)
'''

SCRIPT_WHOLE = PRELUDE + r'''
dirty, clean, lw, obs, _ = helpers.truth_workload(40000, 400, 11)
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
dirty, clean, lw, obs, _ = helpers.truth_workload(40000, 400, 11)
eng = Engine(lw, obs)
h = hashlib.sha256()
try:
    cfg = InferenceConfig(1, 20)
    tr = Trace(lw, obs.shape[1], 5)
    initialize_trace(eng, tr, cfg, 5, max_batch=4096)
    n = obs.shape[1]
    for sweep in range(3):
        changed = observed_sweep(eng, tr, cfg, 77, sweep, batch_rows=n // WINDOWS)
        h.update(str(int(changed)).encode())
        digest_state(h, tr)
    print("DIGEST", h.hexdigest(), {c: int(t.n_live) for c, t in tr.tables.items()})
finally:
    eng.close()
'''

SCRIPT_MANY_REFERENTS = PRELUDE + r'''
from pclean_amd import experiments as ex
from pclean_amd.model import LoweredModel
from pclean_amd.synth import synth_hospital
base, _, _ = synth_hospital(8, 8, 23)
REP = 2000
n = 8 * REP
rows = np.arange(n)
dirty = {c: np.asarray(v, dtype=object)[rows % 8] for c, v in base.items()}
poss = ex.possibilities_of(dirty)
m = ex.hospital_model(poss)
q = ex.hospital_query(m)
lw = LoweredModel(m, q, dirty)
obs = lw.encode_observations(dirty)
# the rows of one observed tuple (row % 8) over 41 latent variants: in every other stretch of 64 rows of the tuple one
# variant per row, elsewhere runs of 30 rows per variant; a variant takes every clean column from a base row of its own
k = rows // 8
variant = np.where((k // 64) % 2 == 0, (k // 30) % 41, k % 41)
rng = np.random.default_rng(3)
by_path = [{}, {}]
ocls = m.classes[q.cls]
for col, ref in q.cleanmap.items():
    if "." not in ref:
        continue
    head, rest = ref.split(".", 1)
    bi = 0 if head == "hosp" else 1
    src = rng.integers(0, 8, 41)  # base row the variants take this column from
    pick = src[variant] if bi == 0 else rows % 8
    by_path[bi][rest] = list(np.asarray(base[col], dtype=object)[pick])
tr = Trace.from_clean_values(lw, by_path, n, 5)
eng = Engine(lw, obs)
h = hashlib.sha256()
try:
    cfg = InferenceConfig(1, 20)
    n_ref = int(tr.tables["Hospital"].n_live)
    assert n_ref >= 16, n_ref  # (many referents per observed tuple: what this state is for)
    whole_sweeps(eng, tr, cfg, h)
    print("DIGEST", h.hexdigest(), n_ref, {c: int(t.n_live) for c, t in tr.tables.items()})
finally:
    eng.close()
'''


def _run(script, extra_env):
    """One fresh process under a time limit; the test stops at the first non-zero exit status."""
    env = dict(os.environ)
    env.update(extra_env)
    env["PCLEAN_TRACE_SYNC"] = "1"
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + script], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("DIGEST")][-1]
    paths = {p for p in ("make_item_groups_static:", "make_item_groups_hash:", "window not cached") if p in out.stderr}
    return line.split()[1], line, paths


def _compare(script, variants, capsys, tag):
    digests, paths = {}, {}
    for name, env in variants.items():
        digests[name], line, paths[name] = _run(script, env)
        with capsys.disabled():
            print(f"\n[static groups, {tag}] {name}: {line} | grouping: {sorted(paths[name])}")
    assert len(set(digests.values())) == 1, digests
    assert "make_item_groups_static:" in paths["default"], paths
    assert "make_item_groups_static:" not in paths["hash table"], paths
    return paths


def test_whole_sweeps_are_bit_identical_across_the_groupings(capsys):
    _compare(SCRIPT_WHOLE, {"default": {}, "hash table": {"PCLEAN_NO_STATIC_GROUPS": "1"},
                            "sorted groups": {"PCLEAN_SORT_GROUPS": "1"}, "no grouping": {"PCLEAN_NO_DEDUP": "1"}},
             capsys, "whole sweeps")


@pytest.mark.parametrize("windows", [4, 9])
def test_windowed_sweeps_match_the_hash_table(capsys, windows):
    script = SCRIPT_WINDOWS.replace("WINDOWS", str(windows))
    paths = _compare(script, {"default": {}, "hash table": {"PCLEAN_NO_STATIC_GROUPS": "1"}}, capsys, f"{windows} windows")
    # nine windows are more than the cache holds: the last one goes through the hash table; four all fit
    assert ("window not cached" in paths["default"]) == (windows == 9), paths


def test_many_referents_per_tuple_match_the_hash_table(capsys):
    _compare(SCRIPT_MANY_REFERENTS, {"default": {}, "hash table": {"PCLEAN_NO_STATIC_GROUPS": "1"}}, capsys, "many referents per tuple")
