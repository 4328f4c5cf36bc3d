"""The memo of option-list marginals (eval.hip: eval_node_lse, memo_lookup_kernel, memo_insert_kernel) call by call, bit for
bit against the CPU oracle, with pclean_debug_memo_stats saying which path every call took.  tests/memo_program.py has the
programs and the three row lists (FIRST, AGAIN = the same rows, SHIFTED = half of them + as many new rows);
tests/test_memo_program_cpu.py checks on the oracle alone that the inputs can tell a broken memo from a sound one.

Every comparison covers the log-marginal, the candidate scores (the new-row candidate's column first: it IS the memo's
value plus a constant) and the draws of score_node on the reference slot above the open option list.  Two programs have
another reference, and why:

  * tab: the frozen oracle does not know tabulated terms.  The reference is the same context without the memo: the leaf
    evaluated directly (score_node on the leaf never enters eval_node_lse; the counters confirm it) and handed to the slot
    as `snew`.  The direct evaluation itself is tied to a float64 restatement (test_memo_program_cpu.tab_leaf_marginals)
    within posterior_exact.logml_bound.
  * two: each of its blocks against the oracle, and the whole sequence against a process with PCLEAN_NO_MEMO=1.

Variants that need an environment switch (PCLEAN_MEMO_CAP, PCLEAN_NO_MEMO) run in a fresh child process under a time
limit; a non-zero exit status fails the test, and no child is started twice for one result."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers
import memo_program as mp
import posterior_exact as pe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 60  # seconds: imports, two or three engines, a few dozen calls of some milliseconds, the oracle beside them


@pytest.fixture(scope="module")
def programs():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = mp.two() if name == "two" else mp.PROGRAMS[name]()
        return cache[name]
    return get


def reference(rig, V, rows):
    """what device(V, rows) must return, bit for bit"""
    if V["name"] != "tab":
        return rig.want(V, rows)
    rig.hip.memo_stats(reset=True)
    leaf = rig.device_leaf(V, rows)
    assert rig.hip.memo_stats()["calls"] == 0, "the direct evaluation of the leaf went through the memo"
    return rig.device(V, rows, snew=leaf)


# ---- miss, hit, partial ------------------------------------------------------------------------------------------------------
def miss_hit_partial(rig, V, label):
    """FIRST, AGAIN, SHIFTED, AGAIN on a fresh table of view V; returns the counters of the four calls"""
    first, again, shifted = mp.FIRST, mp.AGAIN, mp.SHIFTED
    n = len(first)
    slot_alone = rig.slot_alone_launches(V, first)
    want = {k: reference(rig, V, rows) for k, rows in mp.LISTS.items()}
    stored0 = rig.hip.memo_stats()["stored"]  # (other nodes' tables: the counter sums over the context)
    out = []

    got, st, launches = rig.counted(V, first)
    print(f"[{label}] first: {st}, {launches} launches ({slot_alone} for the slot alone)")
    mp.same(got, want["first"], f"{label}, first")
    n_keys = len(set(mp.keys_of(V, first)))
    assert st["calls"] == 1 and st["lookups"] == n and st["misses"] == n and st["resets"] == 1, st
    # every distinct tuple is stored; two items with one tuple may take two slots
    assert n_keys <= st["stored"] - stored0 <= n, (st, stored0, n_keys)
    assert launches > slot_alone
    out.append(st)

    got, st, launches = rig.counted(V, again)
    print(f"[{label}] again: {st}, {launches} launches")
    mp.same(got, want["again"], f"{label}, again")
    assert st["calls"] == 1 and st["lookups"] == n and st["misses"] == 0 and st["resets"] == 0, st
    assert launches == slot_alone, "every item was a hit, yet the leaf was enumerated"
    assert st["stored"] == out[0]["stored"]
    out.append(st)

    got, st, launches = rig.counted(V, shifted)
    print(f"[{label}] shifted: {st}, {launches} launches")
    mp.same(got, want["shifted"], f"{label}, shifted")
    n_new = mp.expected_misses(V, shifted, [first])
    assert 0 < n_new < n
    assert st["calls"] == 1 and st["lookups"] == n and st["misses"] == n_new and st["resets"] == 0, (st, n_new)
    assert launches > slot_alone
    out.append(st)

    got, st, launches = rig.counted(V, again)
    mp.same(got, want["again"], f"{label}, again after shifted")
    assert st["misses"] == 0 and launches == slot_alone, st
    got, st, launches = rig.counted(V, shifted)
    mp.same(got, want["shifted"], f"{label}, shifted again")
    assert st["misses"] == 0 and launches == slot_alone, st
    out.append(st)
    return out


@pytest.mark.parametrize("name", ["cols2", "cols3", "cols6", "ctx2", "tab"])
def test_miss_hit_partial(oracle, programs, name):
    S = programs(name)
    rig = mp.Rig(oracle, helpers, S)
    try:
        if name == "tab":  # the memo-free device reference against the float64 restatement
            from test_memo_program_cpu import tab_leaf_marginals
            leaf, z = rig.device_leaf(S, mp.FIRST), tab_leaf_marginals(oracle, S, mp.FIRST)
            assert all(abs(a - b) <= pe.logml_bound(S["n_options"], b) for a, b in zip(leaf.tolist(), z.tolist()))
        miss_hit_partial(rig, S, name)
    finally:
        rig.close()


def test_seven_columns_stay_off_the_memo(oracle, programs):
    """seven key values do not fit the stored key: no call on the memo path, results the oracle's all the same"""
    S = programs("cols7")
    rig = mp.Rig(oracle, helpers, S)
    try:
        for what, rows in mp.LISTS.items():
            got, st, launches = rig.counted(S, rows)
            mp.same(got, rig.want(S, rows), f"cols7, {what}")
            assert st == dict(calls=0, lookups=0, misses=0, resets=0, stored=0), st
            assert launches > rig.slot_alone_launches(S, rows)
    finally:
        rig.close()


def test_two_nodes_keep_two_tables(oracle, programs):
    """two open leaves whose tuples coincide as integers: the entries of one never answer the other"""
    S = programs("two")
    rig = mp.Rig(oracle, helpers, S)
    try:
        v0, v1 = S["views"]
        assert mp.keys_of(v0, mp.FIRST) == mp.keys_of(v1, mp.FIRST)
        a = miss_hit_partial(rig, v0, "two, block 0")  # (its `first` asserts a full round of misses ...)
        b = miss_hit_partial(rig, v1, "two, block 1")  # (... and so does this one, with block 0's table full of equal keys)
        assert b[0]["stored"] - a[3]["stored"] >= len(set(mp.keys_of(v1, mp.FIRST)))
        want0, want1 = rig.want(v0, mp.FIRST), rig.want(v1, mp.FIRST)
        assert (want0[1][:, -1] != want1[1][:, -1]).mean() > 0.9, "the two leaves' marginals must differ under equal keys"
    finally:
        rig.close()


# ---- resets the version must catch ---------------------------------------------------------------------------------------------
def _reset_round(rig, V, label):
    """after a change of what the marginals depend on: FIRST equals the re-mirrored oracle, one more wipe, every item a miss"""
    rig.mirror()
    want = reference(rig, V, mp.FIRST)
    got, st, _ = rig.counted(V, mp.FIRST)
    print(f"[{label}] {st}")
    n = len(mp.FIRST)
    stale = int((got[0] != want[0]).sum())
    assert st["resets"] == 1 and st["misses"] == st["lookups"] == n, f"{label}: {st}; {stale} of {n} marginals stale"
    mp.same(got, want, label)
    got, st, _ = rig.counted(V, mp.AGAIN)
    mp.same(got, want, label + ", again")
    assert st["resets"] == 0 and st["misses"] == 0, st


@pytest.mark.parametrize("name", ["cols3", "ctx2", "tab"])
def test_resets_the_version_must_catch(oracle, programs, name):
    from pclean_amd import _lib
    S = programs(name)
    lw = S["lw"]
    rig = mp.Rig(oracle, helpers, S)
    try:
        eng, hip = rig.eng, rig.hip
        got, st, _ = rig.counted(S, mp.FIRST)
        before = reference(rig, S, mp.FIRST)
        mp.same(got, before, f"{name}, first")
        assert st["misses"] == st["lookups"] == len(mp.FIRST)

        # other option log-probabilities, the same values
        logp = mp.other_option_logp(S)
        hip.set_options(lw.option_id[S["leaf_attr"]], lw.option_values[S["leaf_attr"]], logp)
        eng.option_logp[S["leaf_attr"]] = logp
        _reset_round(rig, S, f"{name}, set_options")

        # the pair tables of the leaf's AddTypos terms in the other distance mode
        terms = lw.block_arrays(S["block"])[1][S["leaf_terms"]]
        typo = {int(t["pair_table"]) for t in terms if t["dens_kind"] == _lib.DENS_ADD_TYPOS}
        for key, (pid, odom, ldom) in lw.pair_id.items():
            if pid in typo:
                hip.build_pair_table(pid, odom.id_array(), ldom.id_array(), _lib.DIST_DL)
        eng.dist_mode = _lib.DIST_DL  # (every AddTypos table of these programs belongs to the leaf or to its slot)
        for key, (pid, odom, ldom) in lw.pair_id.items():
            if pid not in typo:
                hip.build_pair_table(pid, odom.id_array(), ldom.id_array(), _lib.DIST_DL)
        _reset_round(rig, S, f"{name}, build_pair_table")

        if name == "tab":  # other class densities
            from test_memo_program_cpu import other_class_density
            hip.set_class_density(*other_class_density(S))
            _reset_round(rig, S, f"{name}, set_class_density")

        if name == "ctx2":  # other contents under the same fn-table id
            fid, fn = mp.other_fn_table(S)
            hip.set_fn_table(fid, fn)
            rig.fns[fid] = fn
            _reset_round(rig, S, f"{name}, set_fn_table")

        # the same plan with another max_typos on one term of the leaf
        arrs = mp.other_max_typos(S)
        hip.load_block(S["block"], *arrs)
        rig.blocks[S["block"]] = arrs
        _reset_round(rig, S, f"{name}, load_block")

        after = reference(rig, S, mp.FIRST)
        assert (after[0] != before[0]).mean() > 0.5
    finally:
        rig.close()


# ---- changes that must not reset but must stay right ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cols3", "ctx2"])
def test_other_observations_and_another_window_keep_the_table(oracle, programs, name):
    S = programs(name)
    rig = mp.Rig(oracle, helpers, S)
    try:
        n = len(mp.FIRST)
        got, st, _ = rig.counted(S, mp.FIRST)
        mp.same(got, rig.want(S, mp.FIRST), f"{name}, first")
        assert st["misses"] == n
        # other observations of the same domains: the rows of the table in another order
        perm = np.random.default_rng(1).permutation(S["obs"].shape[1])
        rig.obs = np.ascontiguousarray(S["obs"][:, perm])
        rig.hip.load_columns(rig.obs)
        rig.mirror()
        got, st, _ = rig.counted(S, mp.FIRST)
        print(f"[{name}] other observations: {st}")
        mp.same(got, rig.want(S, mp.FIRST), f"{name}, other observations")
        # the key is the values: an item misses iff its tuple (with the ctx value of its position) was not stored before
        seen = set(mp.keys_of(S, mp.FIRST))
        n_new = sum(k not in seen for k in mp.keys_of(S, mp.FIRST, rig.obs))
        assert st["resets"] == 0 and st["lookups"] == n and st["misses"] == n_new, (st, n_new)
        assert 0 < n_new < n
        # a window that does not start at row 0
        rig.hip.load_columns(S["obs"])
        rig.obs = S["obs"]
        rig.mirror()
        lo = 1152
        rig.hip.set_active_rows(lo, S["obs"].shape[1] - lo)
        rig.row_lo = lo
        seen = set(mp.keys_of(S, mp.FIRST)) | set(mp.keys_of(S, mp.FIRST, np.ascontiguousarray(S["obs"][:, perm])))
        got, st, _ = rig.counted(S, mp.FIRST)
        print(f"[{name}] window from row {lo}: {st}")
        mp.same(got, rig.want(S, mp.FIRST), f"{name}, window from row {lo}")
        n_new = sum(k not in seen for k in mp.keys_of(S, mp.FIRST + lo))
        assert st["resets"] == 0 and st["lookups"] == n and st["misses"] == n_new, (st, n_new)
        assert 0 < n_new < n
    finally:
        rig.close()


# ---- child processes --------------------------------------------------------------------------------------------------------------
SCRIPT = r'''
import hashlib, json, sys
import numpy as np
sys.path[:0] = [ROOT, ROOT + "/tests", ROOT + "/oracle"]
import oracle
import helpers
import memo_program as mp

oracle.build()
mode = sys.argv[1]
h = hashlib.sha256()

def digest(out):
    for a in out:
        h.update(np.ascontiguousarray(a).tobytes())

def lists(name, V, rig, calls):
    """the calls in turn, each against the oracle; one STATS line apiece"""
    for what in calls:
        rows = mp.LISTS[what]
        got, st, launches = rig.counted(V, rows)
        digest(got)
        mp.same(got, rig.want(V, rows), name + ", " + what)
        st["keys"] = len(set(mp.keys_of(V, rows)))
        print("STATS", name, what, json.dumps(st), flush=True)

if mode == "lists":
    for name in sys.argv[2:]:
        S = mp.PROGRAMS[name]()
        rig = mp.Rig(oracle, helpers, S)
        try:
            lists(name, S, rig, ["first", "again", "again", "shifted", "again"])
        finally:
            rig.close()
elif mode == "two":
    S = mp.two()
    rig = mp.Rig(oracle, helpers, S)
    try:
        for what in ["first", "again", "shifted", "again"]:
            for V in S["views"]:
                lists(V["name"], V, rig, [what])
    finally:
        rig.close()
elif mode == "sweeps":
    from pclean_amd.engine import Engine, InferenceConfig
    from pclean_amd.inference import _after_commit
    from pclean_amd.parallel import Comm, exchange_and_commit
    for name in sys.argv[2:]:
        S = mp.PROGRAMS[name]()
        lw, tr = S["lw"], S["trace"]
        eng = Engine(lw, S["obs"], dist_mode=0)
        try:
            cfg = InferenceConfig(1, 3)
            for sweep in range(3):
                if sweep == 2:  # a parameter move: other log-probabilities for the leaf's options
                    logp = mp.other_option_logp(S)
                    eng.hip.set_options(lw.option_id[S["leaf_attr"]], lw.option_values[S["leaf_attr"]], logp)
                    eng.option_logp[S["leaf_attr"]] = logp
                eng.upload_trace(tr)
                eng.hip.memo_stats(reset=True)
                choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 77, sweep)
                st = eng.hip.memo_stats()
                stats = eng.sweep_stats(tr)
                digest((choice, chosen, logml))
                for b in sorted(new_rows):
                    digest(new_rows[b])
                exchange_and_commit(tr, eng.lw, Comm(), 0, choice, stats, new_rows, sweep_idx=sweep)
                _after_commit(eng, tr, 77)
                h.update(np.ascontiguousarray(tr.cur).tobytes())
                for c in sorted(tr.tables):
                    t = tr.tables[c]
                    h.update(np.ascontiguousarray(t.counts[:t.n]).tobytes())
                    h.update(np.ascontiguousarray(t.cols[:, :t.n]).tobytes())
                print("STATS", name, "sweep%d" % sweep, json.dumps(st), flush=True)
        finally:
            eng.close()
print("DIGEST", h.hexdigest())
'''


def run_child(args, env_extra):
    """one fresh process under a time limit: ([(name, call, counters)], digest); a non-zero exit status fails the test"""
    env = dict(os.environ)
    for k in ("PCLEAN_NO_MEMO", "PCLEAN_MEMO_CAP", "PCLEAN_NO_DEDUP", "PCLEAN_NO_GATE"):
        env.pop(k, None)
    env.update(env_extra)
    out = subprocess.run([sys.executable, "-c", "ROOT = %r\n" % ROOT + SCRIPT] + list(args), env=env, capture_output=True,
                         text=True, timeout=CHILD_TIMEOUT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    stats, dig = [], None
    for line in out.stdout.splitlines():
        if line.startswith("STATS "):
            _, name, call, js = line.split(" ", 3)
            stats.append((name, call, json.loads(js)))
        elif line.startswith("DIGEST "):
            dig = line.split()[1]
    assert dig is not None, out.stdout[-3000:]
    return stats, dig


@pytest.mark.parametrize("cap", [4096, 64])
def test_saturation(cap, capsys):
    """PCLEAN_MEMO_CAP: with 4 096 entries inserts stop at the fill limit (half the capacity, checked by every inserting
    thread before it probes: the threads in flight when the limit is crossed may still land); with 64 the table has fewer
    slots than one launch has threads, and lookups and inserts end on the probe limit.  The results stay the oracle's (the
    child compares every call); a table that takes no more entries keeps what it has.  In a table this full a lookup walks
    past many entries: the families of tests/memo_program.py (keys that agree in two words of the stored key and differ in
    the third: cols6 in the last word, cols3 in the second) are what a lookup comparing less than the whole key trips over —
    in the default table of 2^21 slots two such keys never meet."""
    stats, _ = run_child(["lists", "cols3", "cols6", "ctx2"], {"PCLEAN_MEMO_CAP": str(cap)})
    with capsys.disabled():
        for s in stats:
            print(f"\n[saturation, cap {cap}] {s}")
    for name in ("cols3", "cols6", "ctx2"):
        first, again, again2, shifted, again3 = [st for n, _, st in stats if n == name]
        n = first["lookups"]
        assert n == len(mp.FIRST) and first["misses"] == n and first["resets"] == 1
        assert first["keys"] > cap, "the list must hold more keys than the table has slots (test_memo_program_cpu.py)"
        assert cap // 2 <= first["stored"] <= cap, first
        for st in (again, again2, shifted, again3):
            assert st["calls"] == 1 and st["lookups"] == n and st["resets"] == 0, st
            assert st["stored"] == first["stored"], "a table at its fill limit took or lost entries"
        assert 0 < again["misses"] < n, again
        assert again2["misses"] == again["misses"] == again3["misses"], (again, again2, again3)
        assert n - again["misses"] >= first["stored"] // 2, "fewer hits than half the stored entries"
        assert 0 < shifted["misses"] <= n


def test_memo_cap_outside_its_range_is_ignored():
    """not a power of two: the default capacity, every key of FIRST stored"""
    stats, _ = run_child(["lists", "cols2"], {"PCLEAN_MEMO_CAP": "100"})
    first, again = stats[0][2], stats[1][2]
    assert first["stored"] >= first["keys"] and again["misses"] == 0


def test_two_nodes_against_a_process_without_the_memo():
    stats, dig = run_child(["two"], {})
    stats0, dig0 = run_child(["two"], {"PCLEAN_NO_MEMO": "1"})
    assert dig == dig0
    assert all(st["calls"] == 0 and st["stored"] == 0 for _, _, st in stats0)
    by = {(n, c): st for n, c, st in stats}
    n = len(mp.FIRST)
    # block 1's first call finds block 0's table full of the same integers and must miss every item
    assert by[("two/0", "first")]["misses"] == n and by[("two/1", "first")]["misses"] == n
    assert by[("two/1", "first")]["stored"] >= 2 * by[("two/1", "first")]["keys"]
    assert by[("two/0", "again")]["misses"] == 0 and by[("two/1", "again")]["misses"] == 0
    assert by[("two/0", "shifted")]["misses"] == by[("two/1", "shifted")]["misses"] > 0


def test_through_sweeps(capsys):
    """ctx2 and tab, three sweep + commit rounds with a move of the option log-probabilities before the third: one digest over
    outputs and committed state, default against PCLEAN_NO_MEMO=1 alone"""
    stats, dig = run_child(["sweeps", "ctx2", "tab"], {})
    stats0, dig0 = run_child(["sweeps", "ctx2", "tab"], {"PCLEAN_NO_MEMO": "1"})
    with capsys.disabled():
        for s in stats:
            print(f"\n[sweeps] {s}")
    assert dig == dig0
    assert all(st["calls"] == 0 for _, _, st in stats0)
    for name in ("ctx2", "tab"):
        s0, s1, s2 = [st for n, _, st in stats if n == name]
        assert s0["calls"] >= 1 and s0["lookups"] > 0 and s0["misses"] == s0["lookups"], s0
        assert s1["calls"] >= 1 and s1["misses"] < s1["lookups"] and s1["resets"] == 0, s1
        assert s2["calls"] >= 1 and s2["resets"] >= 1 and s2["misses"] > 0, s2
