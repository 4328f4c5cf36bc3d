"""GPU tests of the device tally's own choices and numeric columns (CellTally(..., own=True), PCLEAN_RECON_OWN / _NUM in
csrc/recon.hip) and of the row-bounded counters (evaluate_accuracy_up_to): reconstruction, values, counters, ring and
consensus against analysis.py on rents, on rents with a non-linear Transformation and on the AddNoise program.  String
columns and counters are compared as integers, numeric columns bit for bit (their float64 viewed as int64, NaN included).
tests/test_tally_own_cpu.py checks on the CPU that the row prefixes used here hold missing room types and damaged rents."""
import numpy as np
import pytest

import addnoise_program as ap
import helpers
from pclean_amd import _lib, analysis
from pclean_amd import experiments as ex
from pclean_amd import inference as inf
from pclean_amd import tally as tl
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.model import LoweredModel
from pclean_amd.tally import CellTally
from pclean_amd.trace import Trace
from test_nonlinear_transformation import nonlinear_units

pytestmark = pytest.mark.gpu

NUM = "Monthly Rent"
HOLES = [0, 63, 64, 256]          # rows whose own choices are "none yet" (-1) in the hand-set states
NO_RENT = [5, 63, 65, 130, 256]   # rows whose rent is missing in the hand-set states


def _refuse_pull(self, trace):
    raise AssertionError("Engine.pull called: the device path must not read the state back")


class no_pull:
    def __enter__(self):
        self.real, Engine.pull = Engine.pull, _refuse_pull

    def __exit__(self, *exc):
        Engine.pull = self.real


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float64
    return a.view(np.int64)


def same_table(got, want, columns):
    """`got` (device) against `want` (analysis.reconstructed_pool_ids) over `columns`"""
    for col in columns:
        if isinstance(want[col], tuple):
            assert isinstance(got[col], tuple) and got[col][0] == "numeric"
            assert np.array_equal(bits(got[col][1]), bits(want[col][1])), col
        else:
            assert got[col].dtype == np.int32 and np.array_equal(got[col], np.asarray(want[col]).astype(np.int32)), col


# ---- rents, first 2 000 rows: initialize_trace + one iteration (what tests/test_gpu_tally.py runs) ---------------------
UP_TO = [0, 1, 256, 257, 2000]


@pytest.fixture(scope="module")
def rents():
    dirty, clean = ex.rents_data()
    dirty = {c: v[:2000] for c, v in dirty.items()}
    clean = {c: v[:2000] for c, v in clean.items()}
    m = ex.rents_model(dirty)
    lw = LoweredModel(m, ex.rents_query(m), dirty)
    cfg = InferenceConfig(1, 2, use_mh_instead_of_pg=True, rejuv_frequency=500)
    obs = lw.encode_observations(dirty)
    eng = Engine(lw, obs, dist_mode=1)
    tr = Trace(lw, obs.shape[1], 0)
    inf.initialize_trace(eng, tr, cfg, 0, max_batch=512)
    tally = CellTally(eng, tr, keep=2, own=True)
    with no_pull():
        init_dev = tally.reconstruct(tr)
    init_host = analysis.reconstructed_pool_ids(lw, tr)
    inf.run_inference(eng, tr, cfg, 0)
    with no_pull():  # whatever the engine left ahead of the host arrays stays there
        dev = tally.reconstruct(tr)
        dev_counts = tally.accuracy_counts(tr, dirty, clean)
        dev_up_to = {n: (tally.accuracy_counts_up_to(tr, dirty, clean, n), tally.accuracy_up_to(tr, dirty, clean, n)) for n in UP_TO}
    st = dict(lw=lw, eng=eng, tr=tr, tally=tally, dirty=dirty, clean=clean, init_dev=init_dev, init_host=init_host, dev=dev,
              dev_counts=dev_counts, dev_up_to=dev_up_to, host=analysis.reconstructed_pool_ids(lw, tr),
              host_counts=analysis.accuracy_counts(lw, tr, dirty, clean))
    yield st
    tally.close()
    eng.close()


def test_rents_reconstruction_equals_host(rents):
    tally = rents["tally"]
    assert len(tally.columns) == 5 and sorted(tally.columns) == sorted(rents["lw"].query.cleanmap)
    assert tally.plan.host_strings == [] and tally.plan.numeric == []
    for dev, host in (("init_dev", "init_host"), ("dev", "host")):
        assert sorted(rents[dev]) == sorted(rents[host])
        same_table(rents[dev], rents[host], tally.columns)


def test_rents_counters_run_on_the_device_alone(rents):
    assert rents["dev_counts"].dtype == np.int64 and rents["dev_counts"].shape == (5,)
    assert np.array_equal(rents["dev_counts"], rents["host_counts"]), (rents["dev_counts"], rents["host_counts"])
    assert rents["host_counts"][0] > 0 and rents["host_counts"][1] > 0 and rents["host_counts"][3] > 0


def test_rents_accuracy_up_to_equals_host(rents):
    lw, tr, dirty, clean = rents["lw"], rents["tr"], rents["dirty"], rents["clean"]
    for n in UP_TO:
        six, acc = rents["dev_up_to"][n]
        want = analysis.accuracy_counts_up_to(lw, tr, dirty, clean, n)
        assert six.dtype == np.int64 and np.array_equal(six, want), (n, six, want)
        host = analysis.evaluate_accuracy_up_to(lw, tr, dirty, clean, n)
        assert sorted(acc) == sorted(host)
        for k in acc:
            assert acc[k] == host[k] or (np.isnan(acc[k]) and np.isnan(host[k])), (n, k)
    full, none = rents["dev_up_to"][2000][0], rents["dev_up_to"][0][0]
    assert np.array_equal(full[:5], rents["host_counts"]) and full[5] == full[3] > 0
    assert none[1:5].tolist() == [0, 0, 0, 0] and none[0] == full[0] and none[5] == full[5]
    assert rents["dev_up_to"][256][0][3] < full[3]


def test_hospital_accuracy_up_to_without_own_choices():
    S = helpers.hospital_setup(n_rows=257)
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        tally = CellTally(eng, S["trace"])
        for n in (0, 1, 256, 257):
            six = tally.accuracy_counts_up_to(S["trace"], S["dirty"], S["clean"], n)
            want = analysis.accuracy_counts_up_to(S["lw"], S["trace"], S["dirty"], S["clean"], n)
            assert np.array_equal(six, want), (n, six, want)
            acc = tally.accuracy_up_to(S["trace"], S["dirty"], S["clean"], n)
            host = analysis.evaluate_accuracy_up_to(S["lw"], S["trace"], S["dirty"], S["clean"], n)
            assert all(acc[k] == host[k] or (np.isnan(acc[k]) and np.isnan(host[k])) for k in host), n
        assert want[0] > 0 and want[1] > 0
        tally.close()
    finally:
        eng.close()


def test_default_tally_is_unchanged_and_shares_the_engine(rents):
    """CellTally(eng, tr) beside the own=True tally of the same engine: three columns, the mixed path's counters — and
    each tally finds its own plan in the context again after the other one ran"""
    eng, tr, dirty, clean = rents["eng"], rents["tr"], rents["dirty"], rents["clean"]
    plain = CellTally(eng, tr)
    try:
        assert len(plain.columns) == 3 and plain.plan.host_strings and plain.plan.numeric
        c_plain = plain.accuracy_counts(tr, dirty, clean)
        c_own = rents["tally"].accuracy_counts(tr, dirty, clean)
        assert np.array_equal(c_plain, c_own) and np.array_equal(c_own, rents["host_counts"])
        got = plain.reconstruct(tr)
        assert sorted(got) == sorted(plain.columns)
        same_table(got, rents["host"], plain.columns)
        same_table(rents["tally"].reconstruct(tr), rents["host"], rents["tally"].columns)
    finally:
        plain.close()


# ---- hand-set own choices ----------------------------------------------------------------------------------------------
def _hand_state(n_rows, program):
    """rents-like program on the first n_rows rows with some rents missing, latent state from the clean values
    (helpers.rents_setup); the own choices are written by hand afterwards (set_own)"""
    dirty, clean = ex.rents_data()
    # (the lowering wants the State column to be missing somewhere: a lone row is the first one whose State is; the
    # program itself — states, county names per key — is written from the first 257 rows either way)
    lo = 0 if n_rows > 1 else next(i for i, v in enumerate(dirty["State"]) if v is None)
    assert lo < 257
    program_rows = {c: list(v[:257]) for c, v in dirty.items()}
    dirty = {c: list(v[lo:lo + n_rows]) for c, v in dirty.items()}
    clean = {c: list(v[lo:lo + n_rows]) for c, v in clean.items()}
    for r in NO_RENT:
        if r < n_rows and n_rows > 1:
            dirty[NUM][r] = None
    if program == "addnoise":
        m = ap.addnoise_model(program_rows)
        q = ap.query(m)
    else:
        m = ex.rents_model(program_rows, nonlinear_units()[:2] if program == "nonlinear" else None)
        q = ex.rents_query(m)
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    n = obs.shape[1]
    name_dom, state_dom = lw.latent_dom[("County", "name")], lw.latent_dom[("County", "state")]
    names = [c if (c is not None and name_dom.get(c) >= 0) else d for c, d in zip(clean["County"], dirty["County"])]
    states = []
    for i in range(n):
        v = clean["State"][i] if clean["State"][i] is not None and state_dom.get(clean["State"][i]) >= 0 else dirty["State"][i]
        states.append(v if v is not None else state_dom.string(0))
    tr = Trace.from_clean_values(lw, {0: {"countykey": list(dirty["CountyKey"]), "name": names, "state": states}}, n, 3)
    return dict(lw=lw, obs=obs, tr=tr, dirty=dirty, clean=clean, n=n)


def set_own(S, shift=0):
    """unit = (row // (1 + shift)) % n_units, br = (row + shift) % 5, none (-1) at HOLES; returns the unit options"""
    lw, tr, n = S["lw"], S["tr"], S["n"]
    rows = np.arange(n)
    loc = tr._locals[0]
    loc[:, lw.locals[0].index("br")] = (rows + shift) % 5
    t = lw.gauss_specs[0]["t_local"]
    if t is not None:
        loc[:, t] = (rows // (1 + shift)) % len(lw.gauss_specs[0]["units"])
    loc[[r for r in HOLES if r < n]] = -1
    return np.zeros(n, dtype=np.int32) if t is None else np.maximum(loc[:, t], 0)


@pytest.mark.parametrize("program,n_rows", [("rents", 257), ("rents", 1), ("nonlinear", 257), ("addnoise", 257)])
def test_hand_set_own_choices(program, n_rows):
    S = _hand_state(n_rows, program)
    lw, tr, dirty, clean = S["lw"], S["tr"], S["dirty"], S["clean"]
    spec = lw.gauss_specs[0]
    if program == "nonlinear":
        assert spec["t_x_col"][0] == -1 and spec["t_x_col"][1] >= 0  # (the second option reads its derived column)
    if program == "addnoise":
        assert spec["t_local"] is None
    eng = Engine(lw, S["obs"], dist_mode=1)
    try:
        tally = CellTally(eng, tr, own=True)
        assert tally.plan.kinds["Room Type"] == "own" and tally.plan.kinds[NUM] == "num" and not tally.plan.host_strings
        for shift in (0, 3):  # (the second round: the tally notices that the own choices moved)
            u = set_own(S, shift)
            got = tally.reconstruct(tr)
            want = analysis.reconstructed_pool_ids(lw, tr)
            assert sorted(got) == sorted(want)
            same_table(got, want, tally.columns)
            assert got[NUM][1].shape == (n_rows,) and got["Room Type"].shape == (n_rows,)
            if n_rows > 1:
                assert np.isnan(got[NUM][1]).sum() == len(NO_RENT)
                if program != "addnoise":
                    assert (u == 0).any() and (u == 1).any()
                    x = lw.xnum[spec["x_col"]]
                    moved = ~np.isnan(x) & (u == 1)
                    assert (got[NUM][1][moved] != np.round(x[moved])).any()  # (option 1 does give another number)
            cnt = tally.accuracy_counts(tr, dirty, clean)
            assert np.array_equal(cnt, analysis.accuracy_counts(lw, tr, dirty, clean))
        if n_rows > 1:
            assert cnt[0] > 0 and cnt[1] > 0 and cnt[3] > 0
        tally.close()
    finally:
        eng.close()


# ---- ring, consensus, remap --------------------------------------------------------------------------------------------
def test_ring_wraps_with_own_choices_changed_by_hand():
    S = _hand_state(257, "rents")
    lw, tr, dirty, clean, n = S["lw"], S["tr"], S["dirty"], S["clean"], S["n"]
    eng = Engine(lw, S["obs"], dist_mode=1)
    try:
        tally = CellTally(eng, tr, keep=2, own=True)
        snaps, opts = [], []
        for shift in (0, 1, 2):
            opts.append(set_own(S, shift))
            tally.add(tr)
            snaps.append(analysis.reconstructed_pool_ids(lw, tr))
        assert tally.n_kept == 2
        ids, sup = tally.consensus()
        assert list(ids) == list(lw.query.cleanmap) == list(sup)
        table = {}
        for col in ids:
            if col == NUM:
                mode_u, want_sup = tl.mode_support(np.stack(opts[-2:]))
                want = np.round(lw.gauss_backward(np.arange(n), mode_u, 0))
                assert ids[col][0] == "numeric" and np.array_equal(bits(ids[col][1]), bits(want))
                table[col] = ("numeric", want)
            else:
                want, want_sup = tl.mode_support(np.stack([np.asarray(s[col]) for s in snaps[-2:]]))
                assert np.array_equal(ids[col], want), col
                table[col] = want.astype(np.int64)
            assert np.array_equal(sup[col], want_sup), col
        assert set(np.unique(sup[NUM])) == {1, 2} and set(np.unique(sup["Room Type"])) == {1, 2}  # ties and agreements
        acc = tally.consensus_accuracy(dirty, clean)
        assert acc == analysis.f1_from_counts(analysis.counts_given(lw, table, n, dirty, clean))
        out = analysis.consensus_table(lw, tally, dirty)
        assert out[NUM] == analysis._render_numbers(table[NUM][1]) and out[NUM + "__support"] == sup[NUM].tolist()
        assert out[NUM][NO_RENT[0]] is None and isinstance(out[NUM][1], int)
        assert out["Room Type"] == [lw.pool.strings[i] for i in ids["Room Type"]]
        tally.close()
    finally:
        eng.close()


def test_ring_remap_leaves_numeric_cells_alone():
    S = _hand_state(257, "rents")
    lw, tr = S["lw"], S["tr"]
    eng = Engine(lw, S["obs"], dist_mode=1)
    try:
        tally = CellTally(eng, tr, keep=2, own=True)
        for shift in (1, 0):
            set_own(S, shift)
            tally.add(tr)
        k = tally.columns.index(NUM)
        before, _ = eng.hip.ring_consensus(tally._ring)
        perm = np.arange(len(lw.pool.strings), dtype=np.int32)[::-1].copy()
        assert perm[1] != 1 and (before[k] == 1).any() and (before[k] == 0).any()
        eng.hip.ring_remap(tally._ring, perm)
        after, _ = eng.hip.ring_consensus(tally._ring)
        for c in range(len(tally.columns)):
            want = before[c] if c == k else np.where(before[c] >= 0, perm[np.maximum(before[c], 0)], before[c])
            assert np.array_equal(after[c], want), tally.columns[c]
        assert any(not np.array_equal(after[c], before[c]) for c in range(len(tally.columns)) if c != k)
        tally.close()
    finally:
        eng.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_set_plan_refuses_bad_own_and_numeric_columns(rents):
    eng, tally = rents["eng"], rents["tally"]
    good = {c: rc for c, rc in zip(tally.plan.columns, tally.plan.cols)}

    def variant(rc, **kw):
        new = _lib.ReconCol.from_buffer_copy(rc)
        for k, v in kw.items():
            setattr(new, k, v)
        return new

    bad = [variant(good["Room Type"], col=2), variant(good["Room Type"], col=-1),
           variant(good[NUM], col=1),                            # the node holds one Gaussian term
           variant(good[NUM], block=15), variant(good[NUM], block=99),  # a block that was never loaded, no block at all
           variant(good[NUM], kind=4)]
    for rc in bad:
        with pytest.raises(_lib.PCleanHipError, match="pclean_recon_set_plan"):
            eng.hip.recon_set_plan([rc], tally.plan.id_map)
    same_table(tally.reconstruct(rents["tr"]), rents["host"], tally.columns)  # the plan it had still stands
    # hospital: no block carries a Gaussian term
    S = helpers.hospital_setup(n_rows=257)
    eng2 = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        t2 = CellTally(eng2, S["trace"])
        base = t2.reconstruct(S["trace"])
        with pytest.raises(_lib.PCleanHipError, match="pclean_recon_set_plan"):
            eng2.hip.recon_set_plan([_lib.ReconCol(kind=_lib.RECON_NUM, block=0, table=0, col=0)], np.zeros(0, np.int32))
        again = t2.reconstruct(S["trace"])
        assert all(np.array_equal(base[c], again[c]) for c in base)
        t2.close()
    finally:
        eng2.close()
