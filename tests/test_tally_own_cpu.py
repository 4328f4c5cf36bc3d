"""CPU side of the device tally's own choices, numeric columns and row bound: analysis.evaluate_accuracy_up_to against a
row-by-row restatement of the reference's evaluate_accuracy_up_to (analysis.jl:90-143) written out here, its agreement with
accuracy_counts at n = N, the shape of the rents plan with and without own=True, and the counts of missing room types
and damaged rents in the prefixes the GPU tests use (tests/test_gpu_tally_own.py)."""
import math

import numpy as np
import pytest

import helpers
from pclean_amd import analysis
from pclean_amd import experiments as ex
from pclean_amd import tally as tl


def N_CASES(n):
    return [0, 1, 257, n]


def restated_up_to(lw, trace, dirty, clean, n_up_to):
    """analysis.jl:90-143, cell by cell: `ours` is the cleaned row for the first n_up_to rows and `nothing` after.  Cells
    compare as the reference compares them: strings as strings, the numeric column as numbers (missing = None)."""
    ids = analysis.reconstructed_pool_ids(lw, trace)
    n = trace.cur.shape[1]
    strings = lw.pool.strings
    cleanmap = lw.query.cleanmap

    def ours_cell(col, i):
        v = ids[col]
        if isinstance(v, tuple):
            return float(v[1][i])  # (NaN where the rent is missing: equals nothing, as a missing cell in the reference)
        return strings[v[i]] if v[i] >= 0 else None

    def same(a, b, numeric):
        if a is None or b is None:
            return False
        if numeric:
            return float(a) == float(b)
        return a == b

    errors = changed = cleaned = missing = imputed = imputed_ok = 0
    for i in range(n):
        have = i < n_up_to
        for col in clean:
            if col not in dirty:
                continue
            d, c = dirty[col][i], clean[col][i]
            numeric = col in cleanmap and isinstance(ids[col], tuple)
            if d is None:
                if col in cleanmap and c is not None:
                    if have:
                        imputed += 1
                    missing += 1
                    if have and same(ours_cell(col, i), c, numeric):
                        imputed_ok += 1
                continue
            if (float(d) != float(c) if (numeric and c is not None) else d != c):
                errors += 1
            if col in cleanmap and have:
                o = ours_cell(col, i)
                if not same(o, d, numeric):
                    changed += 1
                    if same(o, c, numeric):
                        cleaned += 1
    num = cleaned + imputed_ok
    precision = num / (changed + imputed) if changed + imputed else float("nan")
    recall = num / (errors + missing) if errors + missing else float("nan")
    f1 = 2.0 / (1 / precision + 1 / recall) if num > 0 else 0.0
    return (dict(f1=f1, errors=errors, changed=changed, cleaned=cleaned, precision=precision, recall=recall, imputed=imputed,
                 correctly_imputed=imputed_ok), missing)


def _same_result(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k] == b[k] or (isinstance(a[k], float) and math.isnan(a[k]) and math.isnan(b[k])), (k, a[k], b[k])


@pytest.fixture(scope="module")
def states(oracle):
    from oracle_engine import OracleEngine
    from pclean_amd import inference as inf
    from pclean_amd.engine import InferenceConfig
    from pclean_amd.model import LoweredModel
    from pclean_amd.trace import Trace
    H = helpers.hospital_setup()
    dirty, clean = ex.rents_data()
    dirty = {c: v[:2000] for c, v in dirty.items()}
    clean = {c: v[:2000] for c, v in clean.items()}
    m = ex.rents_model(dirty)
    lw = LoweredModel(m, ex.rents_query(m), dirty)
    obs = lw.encode_observations(dirty)
    tr = Trace(lw, obs.shape[1], 0)
    cfg = InferenceConfig(1, 2, use_mh_instead_of_pg=True, rejuv_frequency=500)
    inf.initialize_trace(OracleEngine(oracle, lw, obs, cached=True), tr, cfg, 0, max_batch=512)
    return {"hospital": (H["lw"], H["trace"], H["dirty"], H["clean"]), "rents": (lw, tr, dirty, clean)}


@pytest.mark.parametrize("name", ["hospital", "rents"])
def test_evaluate_accuracy_up_to_equals_restatement(states, name):
    lw, tr, dirty, clean = states[name]
    n_rows = tr.cur.shape[1]
    assert n_rows == {"hospital": 1000, "rents": 2000}[name]
    for n in N_CASES(n_rows):
        want, want_missing = restated_up_to(lw, tr, dirty, clean, n)
        got = analysis.evaluate_accuracy_up_to(lw, tr, dirty, clean, n)
        _same_result(got, want)
        six = analysis.accuracy_counts_up_to(lw, tr, dirty, clean, n)
        assert six.dtype == np.int64 and six.shape == (6,)
        assert six.tolist() == [want["errors"], want["changed"], want["cleaned"], want["imputed"], want["correctly_imputed"],
                                want_missing]
    # the cases are not empty: something is damaged, changed and (rents) missing, and the bound matters
    full = analysis.accuracy_counts_up_to(lw, tr, dirty, clean, n_rows)
    part = analysis.accuracy_counts_up_to(lw, tr, dirty, clean, 257)
    assert full[0] > 0 and full[1] > part[1] > 0 and full[0] == part[0] and full[5] == part[5]
    if name == "rents":
        assert full[3] > part[3] > 0 and analysis.accuracy_counts_up_to(lw, tr, dirty, clean, 0)[1:5].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("name", ["hospital", "rents"])
def test_up_to_all_rows_is_accuracy_counts(states, name):
    lw, tr, dirty, clean = states[name]
    n_rows = tr.cur.shape[1]
    six = analysis.accuracy_counts_up_to(lw, tr, dirty, clean, n_rows)
    assert np.array_equal(six[:5], analysis.accuracy_counts(lw, tr, dirty, clean)) and six[5] == six[3]
    _same_result(analysis.evaluate_accuracy_up_to(lw, tr, dirty, clean, n_rows), analysis.evaluate_accuracy(lw, tr, dirty, clean))
    assert np.array_equal(analysis.accuracy_counts_up_to(lw, tr, dirty, clean, n_rows + 5), six)


def test_plan_rents_with_own_choices_serves_every_column():
    S = helpers.rents_setup(n_rows=60)
    lw = S["lw"]
    plan = tl.ReconPlan(lw, own=True)
    assert len(plan.columns) == 5 and sorted(plan.columns) == sorted(S["query"].cleanmap)
    assert plan.host_strings == [] and plan.numeric == [] and plan.device_numeric == ["Monthly Rent"]
    assert plan.kinds["Room Type"] == "own" and plan.kinds["Monthly Rent"] == "num"
    assert [plan.kinds[c] for c in plan.columns] == ["path", "path", "path", "own", "num"]
    own = plan.cols[plan.columns.index("Room Type")]
    assert (own.block, own.col) == (0, lw.locals[0].index("br")) and own.map_len == 5
    assert np.array_equal(plan.id_map[own.map_off:own.map_off + own.map_len], lw.latent_dom[("Obs", "br")].id_array())
    num = plan.cols[plan.columns.index("Monthly Rent")]
    assert (num.block, num.table, num.col, num.map_len) == (lw.gauss_block, 0, 0, 0)
    assert plan.local_blocks == [0]
    # the default plan is what it was
    old = tl.ReconPlan(lw)
    assert sorted(old.columns) == ["County", "CountyKey", "State"] and old.host_strings and old.numeric
    assert old.device_numeric == [] and old.local_blocks == [] and set(old.kinds.values()) == {"path"}
    assert [(c.kind, c.block, c.table, c.col, c.map_off, c.map_len) for c in old.cols] == \
           [(c.kind, c.block, c.table, c.col, c.map_off, c.map_len) for c in plan.cols[:3]]


def test_rents_prefixes_hold_the_cases_the_gpu_tests_need():
    dirty, clean = ex.rents_data()
    for n, n_room, n_rent in ((257, 24, 4), (2000, 207, 24)):
        room = sum(v is None for v in dirty["Room Type"][:n])
        rent = sum(d is not None and c is not None and float(d) != float(c)
                   for d, c in zip(dirty["Monthly Rent"][:n], clean["Monthly Rent"][:n]))
        assert (room, rent) == (n_room, n_rent)
        assert not any(v is None for v in dirty["Monthly Rent"][:n])
