"""The device commit's launch sequences against each other and against the host commit (pclean_amd/csrc/commit.hip):
  * default: phase A (pcc_prepare_block's four steps) as chip-wide launches, then one workgroup per plan (or one workgroup
    for plans that share tables) for the capacity verdict and phase B;
  * PCLEAN_COMMIT_NARROW=1: phase A inside the commit kernel, both cross-workgroup barriers;
  * PCLEAN_COMMIT_ONE_WG=1: the one-workgroup kernel, everything inside it.
The switches are read once per process, so every run is a fresh child process that sweeps and commits through
inference._sweep_window and prints one JSON line: per sweep a SHA-256 over the pulled state (table columns, counts, live
flags, free lists, high-water marks, current referents, row origins), the commit summaries (fallback, n_changed, n_records,
n_distinct) and, from the host side of the same sweep, the sizes of the classes of identical new-row records.

Observed on an MI355X (n_records / n_distinct per plan [Hospital, Measure], the same on the three sequences):
  synthetic (40 000 rows, 2 500 hospitals, three measures merged into a fourth), sweep 0: records [0, 3869], distinct
    [0, 360], the largest class 1118 records (15 workgroups of the wide kernels); sweeps 1-3: [0, 181..189], all distinct;
    with a scratch of 256 records sweep 0 is refused (PCC_FB_RECORDS: records [0, 3869], distinct [0, 0]);
  hospital, 500 rows: [1, 12..16] per sweep; its first commit without spare rows is refused (PCC_FB_CAPACITY: [1, 14]);
  hospital, windows of 16 rows: [0, 1], then five sweeps with [0, 0];   rents, 2 000 rows (one plan): [352..377].
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREP_WG = 256  # PCC_PREP_WG of commit.hip: the workgroup size of the wide phase-A kernels



def synthetic_program():
    """tests/test_gpu_commit.py's synthetic program: 40 000 rows, 2 500 hospitals"""
    from pclean_amd import experiments as ex
    from pclean_amd.engine import InferenceConfig
    from pclean_amd.model import LoweredModel
    from pclean_amd.synth import synth_hospital
    dirty, clean, latent = synth_hospital(40000, 2500, 7)
    (dirty, clean), _ = ex.shuffle_rows([dirty, clean], 7)
    m = ex.hospital_model(ex.possibilities_of(dirty))
    lw = LoweredModel(m, ex.hospital_query(m), dirty)
    return lw, lw.encode_observations(dirty), InferenceConfig(1, 6)


def merge_measures(tr, lw):
    """The latent rows of the three most referenced of the 28 measures are deleted and their observed rows refer to the
    fourth: a consistent state in which the next sweep proposes, for each of the three, one new row from more than a
    thousand observed rows at once — a few large classes of identical new-row records."""
    import numpy as np
    bi = min((b for b, blk in enumerate(lw.blocks) if not blk.get("score")), key=lambda b: tr.tables[lw.blocks[b]["root_class"]].n_live)
    cname = lw.blocks[bi]["root_class"]
    t = tr.tables[cname]
    order = np.argsort(-t.counts[:t.n], kind="stable")
    top, other = np.sort(order[:3]), int(order[3])
    rows = np.isin(tr.cur[bi], top)
    tr.cur[bi, rows] = other
    t.counts[other] += int(rows.sum())
    t.counts[top] = 0
    tr.delete_rows_bulk(cname, top)
    tr.check_consistency()


def state_digest(tr):
    import hashlib
    import numpy as np
    h = hashlib.sha256()
    for c in sorted(tr.tables):
        t = tr.tables[c]
        h.update(np.asarray([t.n] + [int(r) for r in t.free], np.int64).tobytes())
        h.update(np.ascontiguousarray(t.live[:t.n]).tobytes())
        h.update(np.ascontiguousarray(t.counts[:t.n]).tobytes())
        h.update(np.ascontiguousarray(t.cols[:, :t.n]).tobytes())
    h.update(np.ascontiguousarray(tr.cur).tobytes())
    h.update(repr(sorted(tr.row_origin.items())).encode())
    return h.hexdigest()


SCRIPT = r'''
import copy, json, os, sys
import numpy as np
sys.path[:0] = [ROOT, ROOT + "/tests"]
import helpers
import test_gpu_commit_wide as W
from pclean_amd import _lib
from pclean_amd import inference as inf
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.parallel import Comm
from pclean_amd.trace import Trace

case, mode, n_sweeps = sys.argv[1], sys.argv[2], int(sys.argv[3])
tr, max_batch = None, 64
if case in ("hospital", "windows", "capacity"):
    S = helpers.hospital_setup(n_rows=500)
    lw, obs, cfg = S["lw"], S["obs"], InferenceConfig(1, 8)
elif case in ("synthetic", "records"):
    (lw, obs, cfg), max_batch = W.synthetic_program(), 4096
else:
    R = helpers.rents_setup(n_rows=2000)
    lw, obs, tr, cfg = R["lw"], R["obs"], R["trace"], InferenceConfig(1, 4)

inf.DEVICE_COMMIT = mode != "host"
eng = Engine(lw, obs, dist_mode=_lib.DIST_DL)
out = {"sweeps": []}
try:
    if tr is None:
        tr = Trace(lw, obs.shape[1], 1)
        was, inf.DEVICE_COMMIT = inf.DEVICE_COMMIT, False
        inf.initialize_trace(eng, tr, cfg, 11, max_batch=max_batch)
        inf.DEVICE_COMMIT = was
    if case in ("synthetic", "records"):
        W.merge_measures(tr, lw)
        eng._slack_min = lambda cname, t: 512  # room for the first commit's rows: it is to run on the device, not be refused
    if case == "capacity":  # no spare rows at all: the first commit that creates a row is refused
        assert eng.enable_device_commit(tr)
        eng._capacity = lambda cname, t: t.n
        eng._slack_min = lambda cname, t: 0
        for c in eng._dc["tables"]:
            eng._uploaded_shape.pop(c, None)
            eng._dc["cap"].pop(c, None)
        for t in tr.tables.values():
            t.free = []
    nb, n = len(lw.blocks), obs.shape[1]
    summaries, classes = [], []

    def device_state():
        st = [eng.hip.commit_pull_table(lw.table_id[c]) for c in eng._dc["tables"]]
        return [a for s in st for a in s[:5]] + [eng.hip.get_cur(nb, n)]

    def summary(s):
        return {"fallback": int(s.fallback), "n_changed": int(s.n_changed), "n_records": [int(x) for x in s.n_records[:nb]],
                "n_distinct": [int(x) for x in s.n_distinct[:nb]]}
    for name in ("commit_device", "commit_device_dist"):
        def wrap(f):
            def g(*a):
                s = f(*a)
                summaries.append(summary(s))
                return s
            return g
        setattr(eng.hip, name, wrap(getattr(eng.hip, name)))
    if case in ("capacity", "records"):  # a refused commit leaves the device state as it was
        plain = eng.sweep_commit_device
        def checked(trace, *a, **k):
            if trace._dev is None:
                eng.upload_trace(trace)
                eng._sync_cur(trace)
            before = device_state()
            r = plain(trace, *a, **k)
            if r is None:
                after = device_state()
                assert len(before) == len(after) and all(np.array_equal(x, y) for x, y in zip(before, after)), "refused commit modified the device state"
                summaries[-1]["untouched"] = True
            return r
        eng.sweep_commit_device = checked
    plain_xc = inf.exchange_and_commit
    def spy(trace, lw_, comm, lo, choice, stats, new_rows, *a, **k):
        cl = {}
        for bi, (rows, vals) in new_rows.items():
            _, cnt = np.unique(np.asarray(vals)[:, 1:], axis=0, return_counts=True)
            cl[int(bi)] = {"k": int(len(rows)), "distinct": int(len(cnt)), "largest": int(cnt.max())}
        classes.append(cl)
        return plain_xc(trace, lw_, comm, lo, choice, stats, new_rows, *a, **k)
    inf.exchange_and_commit = spy
    for sweep in range(n_sweeps):
        n_s, n_c = len(summaries), len(classes)
        # (windows: sixteen rows per sweep, few enough for sweeps without any new-row record)
        b0, b1 = (16 * sweep, 16 * sweep + 16) if case == "windows" else (0, n)
        changed = inf._sweep_window(eng, tr, cfg, 42, sweep, b0, b1, Comm())
        out["sweeps"].append({"changed": int(changed), "digest": W.state_digest(tr), "summary": summaries[n_s] if len(summaries) > n_s else None,
                              "classes": classes[n_c] if len(classes) > n_c else None})
    tr.check_consistency()
    out["dc"] = {k: int(eng._dc[k]) for k in ("commits", "fallbacks")} if eng._dc else None
    print("RESULT", json.dumps(out))
finally:
    eng.close()
'''

PATHS = {"default": {}, "narrow": {"PCLEAN_COMMIT_NARROW": "1"}, "one_wg": {"PCLEAN_COMMIT_ONE_WG": "1"}}
_cache = {}


def _run(case, mode, n_sweeps, path="default", extra=None):
    """one child process; the result is computed once and shared by the tests that need it"""
    key = (case, mode, n_sweeps, path, tuple(sorted((extra or {}).items())))
    if key not in _cache:
        env = dict(os.environ)
        for k in ("PCLEAN_COMMIT_NARROW", "PCLEAN_COMMIT_ONE_WG", "PCLEAN_COMMIT_KCAP", "PCLEAN_FORCE_DIST"):
            env.pop(k, None)
        env.update(PATHS[path])
        env.update(extra or {})
        p = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + SCRIPT, case, mode, str(n_sweeps)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (key, p.stderr[-3000:])
        line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1]
        _cache[key] = json.loads(line[len("RESULT "):])
        print(f"\n[commit wide] {case} {mode} {path}: " + "; ".join(
            f"sweep {i}: changed {s['changed']} {s['summary']} {s['classes']}" for i, s in enumerate(_cache[key]["sweeps"])))
    return _cache[key]


def _digests(r):
    return [(s["changed"], s["digest"]) for s in r["sweeps"]]


def _counts(r):
    return [s["summary"] and (s["summary"]["fallback"], s["summary"]["n_records"], s["summary"]["n_distinct"],
                              None if s["summary"]["fallback"] else s["summary"]["n_changed"]) for s in r["sweeps"]]


@pytest.mark.parametrize("case", ["hospital", "synthetic", "rents"])
def test_three_paths_and_the_host_commit_give_one_result(case):
    """4 sweeps, each followed by its commit: state digests and summaries are the same on the three launch sequences, and
    the default one equals the host commit (the device summaries' record counts equal the host's own grouping)"""
    runs = {path: _run(case, "device", 4, path) for path in PATHS}
    host = _run(case, "host", 4)
    for path in ("narrow", "one_wg"):
        assert _digests(runs[path]) == _digests(runs["default"]), (case, path)
        assert _counts(runs[path]) == _counts(runs["default"]), (case, path)
    assert _digests(runs["default"]) == _digests(host), case
    assert runs["default"]["dc"]["commits"] > runs["default"]["dc"]["fallbacks"], runs["default"]["dc"]
    for dev, ref in zip(runs["default"]["sweeps"], host["sweeps"]):
        if dev["summary"]["fallback"] & 1:  # (more records than the scratch holds: nothing further was counted)
            continue
        for bi, cl in ref["classes"].items():
            assert dev["summary"]["n_records"][int(bi)] == cl["k"] and dev["summary"]["n_distinct"][int(bi)] == cl["distinct"], (dev, ref)


def test_the_shapes_at_which_the_wide_kernels_can_go_wrong():
    """synthetic (40 000 rows, 2 500 hospitals, initialised in batches of <= 4096): a commit whose records span several
    workgroups of the wide kernels and fall into few, large classes that contend for one hash slot each; sweeps with no
    record in one plan, and in neither.  (Preconditions of the comparison above: without them it would be vacuous.)"""
    dev, host = _run("synthetic", "device", 4), _run("synthetic", "host", 4)
    ok = False
    for d, h in zip(dev["sweeps"], host["sweeps"]):
        for bi, cl in h["classes"].items():
            if d["summary"]["fallback"] == 0 and cl["k"] >= 2 * PREP_WG and 4 * cl["distinct"] <= cl["k"] and cl["largest"] > 64:
                assert d["summary"]["n_records"][int(bi)] == cl["k"]
                ok = True
    assert ok, [h["classes"] for h in host["sweeps"]]
    # no record in one plan, some in the other
    recs = [s["summary"]["n_records"] for s in dev["sweeps"] if not s["summary"]["fallback"]]
    assert any(min(r) == 0 and max(r) > 0 for r in recs), recs
    # no record in either plan: sweeps over windows of sixteen rows of the 500-row hospital table
    win = {path: _run("windows", "device", 8, path) for path in PATHS}
    recs = [s["summary"]["n_records"] for s in win["default"]["sweeps"] if not s["summary"]["fallback"]]
    assert any(max(r) == 0 for r in recs), recs
    host_win = _run("windows", "host", 8)
    for path in PATHS:
        assert _digests(win[path]) == _digests(host_win), path
        assert _counts(win[path]) == _counts(win["default"]), path


@pytest.mark.parametrize("case,extra,bit", [("capacity", {}, 4), ("records", {"PCLEAN_COMMIT_KCAP": "256"}, 1)])
def test_refusals_leave_the_tables_untouched(case, extra, bit):
    """a table without spare rows (PCC_FB_CAPACITY) / a record scratch of 256 entries (PCC_FB_RECORDS): the refused commit
    leaves tables, counts and referents bit-identical on the device (checked in the child around the call), its summary's
    n_records / n_distinct equal the narrow sequence's (they were timing-dependent there before the early exit read
    fallback_in), and the run goes on through the host commit to the same states"""
    runs = {path: _run(case, "device", 4, path, extra) for path in ("default", "narrow")}
    refused = [s["summary"] for s in runs["default"]["sweeps"] if s["summary"] and s["summary"]["fallback"] & bit]
    assert refused and all(s.get("untouched") for s in refused), runs["default"]["sweeps"]
    assert _counts(runs["default"]) == _counts(runs["narrow"])
    assert _digests(runs["default"]) == _digests(runs["narrow"])
    if case == "records":
        assert any(max(s["n_records"]) > 256 for s in refused), refused
        assert runs["default"]["dc"]["commits"] > runs["default"]["dc"]["fallbacks"], runs["default"]["dc"]
    assert _digests(runs["default"]) == _digests(_run("capacity" if case == "capacity" else "synthetic", "host", 4))


def test_the_gathered_form_equals_the_plain_device_commit(monkeypatch):
    """pclean_commit_device_dist on a one-rank communicator (moved rows and records packed, all-gathered, merged; the wide
    launches read the gathered blocks) == the plain device commit, sweep after sweep, on the synthetic case (this process:
    no switch set, the default sequence)"""
    import copy

    from pclean_amd import _lib
    from pclean_amd import inference as inf
    from pclean_amd.engine import Engine
    from pclean_amd.parallel import Comm
    from pclean_amd.trace import Trace
    for k in PATHS["narrow"].keys() | PATHS["one_wg"].keys():
        assert k not in os.environ
    lw, obs, cfg = synthetic_program()
    plain, dist = Engine(lw, obs, dist_mode=_lib.DIST_DL), Engine(lw, obs, dist_mode=_lib.DIST_DL)
    try:
        a = Trace(lw, obs.shape[1], 1)
        inf.initialize_trace(plain, a, cfg, 11, max_batch=4096)
        merge_measures(a, lw)
        b = copy.deepcopy(a)
        for t in list(a.tables.values()) + list(b.tables.values()):
            t.cols_dirty = True
        plain._slack_min = dist._slack_min = lambda cname, t: 512
        dist.hip.comm_init(1, 0, dist.hip.comm_unique_id())
        dist._dev_comm = True
        monkeypatch.setenv("PCLEAN_FORCE_DIST", "1")
        n = obs.shape[1]
        for sweep in range(3):
            ca = inf._sweep_window(plain, a, cfg, 42, sweep, 0, n, Comm())
            cb = inf._sweep_window(dist, b, cfg, 42, sweep, 0, n, Comm())
            assert ca == cb and state_digest(a) == state_digest(b), (sweep, ca, cb)
        assert getattr(dist, "_dc_dist", False) and dist._dc["commits"] == plain._dc["commits"] >= 3, (dist._dc, plain._dc)
        assert dist._dc["fallbacks"] == plain._dc["fallbacks"] == 0, (dist._dc, plain._dc)
    finally:
        plain.close()
        dist.close()
