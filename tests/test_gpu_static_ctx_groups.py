"""Context items grouped from the static tuple order (eval.hip: make_item_groups_static_ctx) against the paths it replaces.

The Measure block's items carry a context (the State of the hospital a particle chose): item i < N is row i with particle
0's context, the further distinct contexts of a row are extra items behind them.  By default the primary items are now
classed by (ctx, referent) inside the tiles of the static tuple order — wave tiles by ballots, the long tiles of segments
longer than a wavefront through a table in LDS — and every extra item is a group of one.  PCLEAN_NO_STATIC_CTX_GROUPS=1
sends the lists with a context back to the hash table, PCLEAN_NO_STATIC_GROUPS=1 every list, PCLEAN_NO_DEDUP=1 groups
nothing.  A group may be split, never merged, and every result is a function of the item alone: all variants must leave the
same SHA-256 over three sweeps' outputs and committed states (the technique, prelude and planted state of
test_gpu_static_groups.py; one fresh process per variant under a time limit, the test stops at the first non-zero status).

  * helpers.truth_workload(12000, 150, 11) after its own initialisation in batches of 4096 rows (the same path with no
    current referent), swept whole, and as two windows of 6000 rows;
  * the many-referents state: 8 observed tuples x 2000 rows over 41 hospital variants that take their columns, State
    included, from base rows of their own — every tuple segment is longer than a long tile (1024 positions) and is cut, the
    rows of one tuple carry many contexts, and the particles of a row disagree about the context: extra items.

PCLEAN_TRACE_SYNC=1 shows the path: the default process must report a context list on the static path (on the planted state
with long tiles and extra items), the PCLEAN_NO_STATIC_CTX_GROUPS process none — or a path would be compared with itself.
The truth workload itself has no long tile to report at 12000 rows: the Measure block's observed tuple includes the
state-average column, (state, measure) pairs of a few rows each, so no segment of it is longer than a wavefront.

Group count (whole sweeps of the truth workload, root statistics of the Measure block): no segment there is longer than a
long tile and shorter segments are never split, so the tiles find exactly the classes of the primary items, and the
default's count is those classes plus its extra items.  The hash table classes ALL items, so an extra item whose key another
item has joins that item's group there: hash <= default <= hash + extras with 20 particles (measured: sweep 0 has 1786
extras, the default 4807 groups, the hash table 3463 — "hash + extras" exactly would need every extra's key to be unique).
The exact comparison is made where there are no extras: a sweep with ONE particle, default == hash."""
import os
import re
import subprocess
import sys

import pytest

from test_gpu_static_groups import PRELUDE, SCRIPT_MANY_REFERENTS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT_TRUTH_WHOLE = PRELUDE + r'''
dirty, clean, lw, obs, _ = helpers.truth_workload(12000, 150, 11)
eng = Engine(lw, obs)
h = hashlib.sha256()
try:
    cfg = InferenceConfig(1, 20)
    tr = Trace(lw, obs.shape[1], 5)
    initialize_trace(eng, tr, cfg, 5, max_batch=4096)
    eng.hip.set_timed_block(len(lw.blocks) - 1)  # the Measure block: its root's statistics below
    for sweep in range(3):
        print("SWEEP", sweep, file=sys.stderr, flush=True)
        eng.upload_trace(tr)
        choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 77, sweep)
        print("NGROUPS", sweep, int(eng.hip.get_root_stats().n_groups), int(eng.hip.get_root_stats().n_items), flush=True)
        stats = eng.sweep_stats(tr)
        for a in (choice, chosen, logml):
            h.update(np.ascontiguousarray(a).tobytes())
        for b in sorted(new_rows):
            h.update(np.ascontiguousarray(new_rows[b][0]).tobytes())
            h.update(np.ascontiguousarray(new_rows[b][1]).tobytes())
        exchange_and_commit(tr, eng.lw, Comm(), 0, choice, stats, new_rows)
        digest_state(h, tr)
    # one more sweep with ONE particle (nothing committed): no row has a second context, no extra items
    print("SWEEP", 3, file=sys.stderr, flush=True)
    eng.upload_trace(tr)
    eng.sweep(tr, InferenceConfig(1, 1), 77, 3)
    print("NGROUPS", 3, int(eng.hip.get_root_stats().n_groups), int(eng.hip.get_root_stats().n_items), flush=True)
    print("DIGEST", h.hexdigest(), {c: int(t.n_live) for c, t in tr.tables.items()})
finally:
    eng.close()
'''

SCRIPT_TRUTH_WINDOWS = PRELUDE + r'''
dirty, clean, lw, obs, _ = helpers.truth_workload(12000, 150, 11)
eng = Engine(lw, obs)
h = hashlib.sha256()
try:
    cfg = InferenceConfig(1, 20)
    tr = Trace(lw, obs.shape[1], 5)
    initialize_trace(eng, tr, cfg, 5, max_batch=4096)
    n = obs.shape[1]
    for sweep in range(3):
        changed = observed_sweep(eng, tr, cfg, 77, sweep, batch_rows=n // 2)
        h.update(str(int(changed)).encode())
        digest_state(h, tr)
    print("DIGEST", h.hexdigest(), {c: int(t.n_live) for c, t in tr.tables.items()})
finally:
    eng.close()
'''

VARIANTS = {"default": {}, "context lists on the hash table": {"PCLEAN_NO_STATIC_CTX_GROUPS": "1"},
            "hash table": {"PCLEAN_NO_STATIC_GROUPS": "1"}, "no grouping": {"PCLEAN_NO_DEDUP": "1"}}

STATIC_LINE = re.compile(r"\[pclean static groups\] block (\d+) node (\d+): primary items (\d+), extra items (\d+), "
                         r"groups (\d+), long tiles (\d+)( \(context list\))?")


def _run(script, extra_env):
    """One fresh process under a time limit; the test stops at the first non-zero exit status."""
    env = dict(os.environ)
    env.update(extra_env)
    env["PCLEAN_TRACE_SYNC"] = "1"
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", "ROOT = %r\n" % ROOT + script], env=env,
                         capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    digest = [l for l in out.stdout.splitlines() if l.startswith("DIGEST")][-1]
    ngroups = {int(l.split()[1]): int(l.split()[2]) for l in out.stdout.splitlines() if l.startswith("NGROUPS")}
    # the static path's reports, by sweep (the lines before the first "SWEEP" belong to the initialisation: key -1)
    reports, sweep = [], -1
    for l in out.stderr.splitlines():
        if l.startswith("SWEEP "):
            sweep = int(l.split()[1])
        m = STATIC_LINE.search(l)
        if m:
            reports.append(dict(sweep=sweep, block=int(m.group(1)), node=int(m.group(2)), primary=int(m.group(3)),
                                extra=int(m.group(4)), groups=int(m.group(5)), long_tiles=int(m.group(6)), ctx=m.group(7) is not None))
    names = {p for p in ("make_item_groups_static_ctx:", "make_item_groups_static:", "make_item_groups_hash:") if p in out.stderr}
    return dict(digest=digest.split()[1], line=digest, ngroups=ngroups, reports=reports, names=names)


def _compare(script, capsys, tag):
    runs = {}
    for name, env in VARIANTS.items():
        r = runs[name] = _run(script, env)
        ctx = [x for x in r["reports"] if x["ctx"]]
        with capsys.disabled():
            print(f"\n[static ctx groups, {tag}] {name}: {r['line']} | read-backs: {sorted(r['names'])} | context lists on the static "
                  f"path: {len(ctx)}, long tiles {sorted({x['long_tiles'] for x in ctx})}, extra items {[x['extra'] for x in ctx][:12]}"
                  f" | Measure root groups {r['ngroups']}")
    assert len({r["digest"] for r in runs.values()}) == 1, {k: r["digest"] for k, r in runs.items()}
    # no path is compared with itself
    d = runs["default"]
    assert "make_item_groups_static_ctx:" in d["names"], d["names"]
    assert any(x["ctx"] for x in d["reports"]), d["reports"]
    nc = runs["context lists on the hash table"]
    assert not any(x["ctx"] for x in nc["reports"]) and "make_item_groups_static_ctx:" not in nc["names"], nc["reports"]
    assert "make_item_groups_static:" in nc["names"] and "make_item_groups_hash:" in nc["names"], nc["names"]  # (block 0 stays static)
    ht = runs["hash table"]
    assert not ht["reports"] and not ht["names"] & {"make_item_groups_static_ctx:", "make_item_groups_static:"}, ht["names"]
    assert not runs["no grouping"]["reports"], runs["no grouping"]["reports"]
    return runs


def test_truth_workload_whole_sweeps_and_group_count(capsys):
    runs = _compare(SCRIPT_TRUTH_WHOLE, capsys, "truth workload, whole sweeps")
    d, ht = runs["default"], runs["hash table"]
    last = max(x["block"] for x in d["reports"])
    assert sorted(d["ngroups"]) == [0, 1, 2, 3] and sorted(ht["ngroups"]) == [0, 1, 2, 3], (d["ngroups"], ht["ngroups"])
    for sweep in range(4):
        root = [x for x in d["reports"] if x["sweep"] == sweep and x["ctx"] and x["block"] == last and x["node"] == 0]
        assert len(root) == 1, root
        extra = root[0]["extra"]
        with capsys.disabled():
            print(f"[static ctx groups, group count] sweep {sweep}: default {d['ngroups'][sweep]} groups (static path reported "
                  f"{root[0]['groups']}, {extra} extra items, {root[0]['long_tiles']} long tiles), hash table {ht['ngroups'][sweep]}")
        assert root[0]["groups"] == d["ngroups"][sweep], (root, d["ngroups"])
        # default = classes of the primary items + extras; hash table = classes of ALL items: at least those of the primary
        # items, and one more for every extra whose key no other item has
        assert ht["ngroups"][sweep] <= d["ngroups"][sweep] <= ht["ngroups"][sweep] + extra, (sweep, d["ngroups"], ht["ngroups"], root)
    # one particle: no extras, and the counts are equal — the tiles split no class of this table
    assert [x["extra"] for x in d["reports"] if x["sweep"] == 3 and x["ctx"]] == [0], d["reports"]
    assert d["ngroups"][3] == ht["ngroups"][3], (d["ngroups"], ht["ngroups"])


def test_truth_workload_two_windows(capsys):
    runs = _compare(SCRIPT_TRUTH_WINDOWS, capsys, "truth workload, two windows")
    assert any(x["ctx"] and x["primary"] == 6000 for x in runs["default"]["reports"]), runs["default"]["reports"]
    assert any(x["ctx"] and x["primary"] == 4096 for x in runs["default"]["reports"]), runs["default"]["reports"]  # (the initialisation)


def test_many_referents_long_tiles_and_extra_items(capsys):
    runs = _compare(SCRIPT_MANY_REFERENTS, capsys, "many referents per tuple")
    ctx = [x for x in runs["default"]["reports"] if x["ctx"]]
    assert any(x["long_tiles"] > 0 for x in ctx), ctx
    assert any(x["extra"] > 0 for x in ctx), ctx
    # 8 tuple segments of 2000 positions: two long tiles each, in the Measure block as in block 0
    assert any(x["long_tiles"] == 16 for x in ctx), ctx
