"""CPU side of pclean_amd.tally: the tie rule of the per-cell consensus restated in NumPy (`mode_support`, the reference
of tests/test_gpu_tally.py), the reconstruction plans of the three shipped programs, the run_inference hook, and the
seed of the GPU relower test (strings drawn for chosen dummies join the domains BETWEEN two tally.add calls)."""
import numpy as np
import pytest

import helpers
from pclean_amd import tally as tl

# flights run of the relower test (tests/test_gpu_tally.py::test_relower_translates_kept_snapshots): prior proposals choose
# the TimePrior dummy in every iteration (data-driven proposals do so during the first iteration only, for every seed tried)
RELOWER_SEED, RELOWER_ITERS, RELOWER_PARTICLES = 1, 4, 4


def relower_config():
    from pclean_amd.engine import InferenceConfig
    return InferenceConfig(RELOWER_ITERS, RELOWER_PARTICLES, rejuv_frequency=500, use_dd_proposals=False)


def mode_support(snapshots):
    """snapshots [S][M], oldest first -> (mode[M], support[M]): the most frequent value of every cell and the number of
    snapshots that hold it; among equally frequent values the one whose LATEST occurrence is the most recent wins.
    Cell by cell, straight from the definition."""
    snaps = np.asarray(snapshots)
    s_n, m = snaps.shape
    mode = np.zeros(m, dtype=np.int32)
    support = np.zeros(m, dtype=np.int32)
    for i in range(m):
        col = snaps[:, i].tolist()
        count, latest = {}, {}
        for s, v in enumerate(col):
            count[v] = count.get(v, 0) + 1
            latest[v] = s
        best = max(count, key=lambda v: (count[v], latest[v]))
        mode[i], support[i] = best, count[best]
    return mode, support


CASES = [
    ("one snapshot", [[7, -1, 3]], [7, -1, 3], [1, 1, 1]),
    ("all equal", [[4, 4], [4, 4], [4, 4]], [4, 4], [3, 3]),
    ("2-2 tie, the newer value wins", [[1, 9], [2, 8], [1, 8], [2, 9]], [2, 9], [2, 2]),
    ("2-2-1 tie", [[5], [6], [7], [5], [6]], [6], [2]),
    ("2-2-1 tie, the single value newest", [[5], [6], [5], [6], [7]], [6], [2]),
    ("negative ids", [[-1, -2], [-2, -2], [-1, 0], [3, 0]], [-1, 0], [2, 2]),
    ("a value only in the oldest slot", [[9, 9], [1, 2], [1, 3]], [1, 3], [2, 1]),
    ("all distinct: the newest", [[1], [2], [3], [4]], [4], [1]),
    ("majority beats recency", [[3], [3], [3], [8], [9]], [3], [3]),
]


@pytest.mark.parametrize("name,snaps,mode,support", CASES, ids=[c[0] for c in CASES])
def test_mode_support_cases(name, snaps, mode, support):
    got = mode_support(np.array(snaps, dtype=np.int32))
    assert got[0].tolist() == mode and got[1].tolist() == support
    # the host twin that tallies the host-only columns follows the same rule
    twin = tl.mode_support(np.array(snaps, dtype=np.int64))
    assert twin[0].tolist() == mode and twin[1].tolist() == support


def test_host_twin_equals_restatement_on_random_ties():
    rng = np.random.default_rng(4)
    for s_n in (1, 2, 3, 5, 16, 32):
        snaps = rng.choice(np.array([-2, -1, 0, 3, 11], dtype=np.int32), size=(s_n, 500))
        a, b = mode_support(snaps), tl.mode_support(snaps)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_plan_hospital_serves_every_column():
    S = helpers.hospital_setup(n_rows=40)
    plan = tl.ReconPlan(S["lw"])
    assert sorted(plan.columns) == sorted(S["query"].cleanmap) and len(plan.columns) == 15
    assert plan.kinds["Stateavg"] == "fn" and [c for c, k in plan.kinds.items() if k == "fn"] == ["Stateavg"]
    assert plan.host_strings == [] and plan.numeric == []
    blocks = [rc.block for rc in plan.cols if rc.kind == 0]
    assert blocks == sorted(blocks)  # one block's columns follow each other: its referent is read once
    # the function table is indexed [earlier slot's value][later slot's value] and covers both domains
    rc = plan.cols[plan.columns.index("Stateavg")]
    fn = S["lw"].fn_tables[rc.fn_table]
    assert rc.block < rc.block_b and rc.map_len == int(fn.max()) + 1
    for rc in plan.cols:
        assert 0 <= rc.map_off and rc.map_off + rc.map_len <= len(plan.id_map)


def test_plan_rents_is_mixed():
    S = helpers.rents_setup(n_rows=60)
    plan = tl.ReconPlan(S["lw"])
    assert sorted(plan.columns) == ["County", "CountyKey", "State"]
    rest = sorted(set(S["query"].cleanmap) - set(plan.columns))
    assert sorted(plan.host_strings + plan.numeric) == rest and len(plan.numeric) == 1 and len(plan.host_strings) >= 1


def test_plan_flights_serves_every_column():
    S = helpers.flights_setup()
    plan = tl.ReconPlan(S["lw"])
    assert sorted(plan.columns) == sorted(S["query"].cleanmap) and len(plan.columns) == 6
    assert set(plan.kinds.values()) == {"path"}


def test_truth_ids_make_inequality_an_id_test():
    index = {"a": 0, "b": 1}
    d = ["a", "x", "x", None, "b", "y", None]
    c = ["a", "x", "z", "a", None, "b", None]
    d_id, c_id = tl.truth_ids(index, d, c)
    assert d_id.tolist() == [0, -3, -3, -4, 1, -3, -4]
    assert c_id.tolist() == [0, -3, -5, 0, -6, 1, -6]
    ne = np.array([x != y for x, y in zip(d, c)])
    assert np.array_equal((d_id != c_id) & (d_id != -4), ne & np.array([x is not None for x in d]))


def test_keep_is_validated_before_anything_else():
    for keep in (0, 33, -1):
        with pytest.raises(ValueError):
            tl.CellTally(None, None, keep=keep)


def test_run_inference_hook_and_relower_seed(oracle):
    """run_inference accepts tally=None, calls tally.add after every iteration it >= tally_from — and for the GPU relower
    test's run (the oracle engine is the GPU path bit for bit) strings drawn for chosen dummies rebuild the pool between
    the first and the last add, in a way that moves ids (the old strings are no prefix of the new pool)."""
    from oracle_engine import OracleEngine
    from pclean_amd import inference as inf
    from pclean_amd.trace import Trace
    from test_flights_cpu import flights_setup
    dirty, clean, lw, obs = flights_setup()
    eng = OracleEngine(oracle, lw, obs)
    tr = Trace(lw, obs.shape[1], RELOWER_SEED)
    cfg = relower_config()
    inf.initialize_trace(eng, tr, cfg, RELOWER_SEED, max_batch=512)

    class Recorder:
        def __init__(self):
            self.pools = []

        def add(self, trace):
            self.pools.append(list(lw.pool.strings))

    rec = Recorder()
    inf.run_inference(eng, tr, cfg, RELOWER_SEED, tally=rec)
    assert len(rec.pools) == RELOWER_ITERS
    first, last = rec.pools[0], rec.pools[-1]
    assert len(last) > len(first) and last[:len(first)] != first
    two, late = relower_config(), Recorder()
    two.num_iters = 2
    inf.run_inference(eng, tr, two, RELOWER_SEED + 1, tally=late, tally_from=1)
    assert len(late.pools) == 1
    inf.run_inference(eng, tr, two, RELOWER_SEED + 2, tally=None)
