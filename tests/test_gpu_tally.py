"""GPU tests of pclean_amd.tally / csrc/recon.hip: the consensus kernel against the NumPy restatement of its tie rule
(tests/test_tally_cpu.py::mode_support), the device reconstruction and accuracy counters against analysis.py on the three
shipped programs, the ring's wrap-around, kept snapshots across a rebuilt string pool, and no change of the sampler's
results.  Every comparison is integer equality."""
import copy

import numpy as np
import pytest

import helpers
from pclean_amd import analysis
from pclean_amd import experiments as ex
from pclean_amd import inference as inf
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.model import LoweredModel
from pclean_amd.tally import CellTally
from pclean_amd.trace import Trace
from test_tally_cpu import RELOWER_SEED, mode_support, relower_config

pytestmark = pytest.mark.gpu

M_SIZES = [1, 63, 64, 65, 255, 256, 257, 100003]
M_MAX = max(M_SIZES)
ALPHABETS = {"two": np.array([-1, 4], dtype=np.int32), "five": np.array([-2, -1, 0, 7, 1 << 20], dtype=np.int32)}


# ---- 1. the consensus kernel on synthetic input ------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet", sorted(ALPHABETS))
@pytest.mark.parametrize("S", [1, 2, 3, 5, 16, 31, 32])
def test_cell_mode_equals_restatement(hip, S, alphabet):
    rng = np.random.default_rng(1000 * S + len(alphabet))
    snaps = rng.choice(ALPHABETS[alphabet], size=(S, M_MAX))
    want_mode, want_sup = mode_support(snaps)  # once for the largest M: a cell's result depends on its own values only
    for m in M_SIZES:
        mode, sup = hip.cell_mode(snaps[:, :m])
        assert mode.shape == (m,) and sup.shape == (m,)
        assert np.array_equal(mode, want_mode[:m]) and np.array_equal(sup, want_sup[:m]), (S, m)


def test_cell_mode_all_values_distinct(hip):
    rng = np.random.default_rng(7)
    snaps = np.stack([rng.permutation(32) for _ in range(300)], axis=1).astype(np.int32) - 2  # [32][300], -2 and -1 among them
    for S in (2, 5, 16, 32):
        mode, sup = hip.cell_mode(snaps[:S])
        want = mode_support(snaps[:S])
        assert np.array_equal(mode, want[0]) and np.array_equal(sup, want[1])
        assert np.array_equal(mode, snaps[S - 1]) and (sup == 1).all()  # the newest


def test_cell_mode_refuses_zero_and_33_snapshots(hip):
    for S in (0, 33):
        with pytest.raises(ValueError):
            hip.cell_mode(np.zeros((S, 10), dtype=np.int32))
    from pclean_amd import _lib
    import ctypes as C
    out = np.zeros(10, dtype=np.int32)
    snaps = np.zeros((33, 10), dtype=np.int32)
    for S in (0, 33):  # the C entry point itself
        rc = hip.lib.pclean_cell_mode(hip.h, C.c_int32(S), C.c_int64(10), _lib._p(snaps, C.c_int32), _lib._p(out, C.c_int32),
                                      _lib._p(out, C.c_int32))
        assert rc == -1


# ---- programs: one run each, shared by the reconstruction and the counter tests ------------------------------------------
def _refuse_pull(self, trace):
    raise AssertionError("Engine.pull called: the device path must not read the state back")


def _program_state(name):
    """initialize_trace + one iteration; returns what the device path gave BEFORE anything pulled the state (with Engine.pull
    made to raise for the duration when device commits are ahead of the host arrays) and the host's answers after."""
    if name == "hospital":
        dirty, clean = ex.hospital_data()
        (dirty, clean), _ = ex.shuffle_rows([dirty, clean], 0)
        m = ex.hospital_model(ex.possibilities_of(dirty))
        lw = LoweredModel(m, ex.hospital_query(m), dirty)
        cfg, batch = InferenceConfig(1, 2, use_mh_instead_of_pg=True), 256
    elif name == "flights":
        dirty, clean = ex.flights_data()
        m = ex.flights_model(dirty)
        lw = LoweredModel(m, ex.flights_query(m), dirty)
        cfg, batch = InferenceConfig(1, 2, use_mh_instead_of_pg=True, rejuv_frequency=500), 512
    else:
        dirty, clean = ex.rents_data()
        dirty = {c: v[:2000] for c, v in dirty.items()}
        clean = {c: v[:2000] for c, v in clean.items()}
        m = ex.rents_model(dirty)
        lw = LoweredModel(m, ex.rents_query(m), dirty)
        cfg, batch = InferenceConfig(1, 2, use_mh_instead_of_pg=True, rejuv_frequency=500), 512
    obs = lw.encode_observations(dirty)
    eng = Engine(lw, obs, dist_mode=1)
    tr = Trace(lw, obs.shape[1], 0)
    inf.initialize_trace(eng, tr, cfg, 0, max_batch=batch)
    tally = CellTally(eng, tr, keep=2)
    init_dev = tally.reconstruct(tr)  # a host-committed trace, no device commit set up yet
    init_host = analysis.reconstructed_pool_ids(lw, tr, columns=tally.columns)
    inf.run_inference(eng, tr, cfg, 0)
    ahead = tr._dev is eng
    real_pull = Engine.pull
    if ahead:
        Engine.pull = _refuse_pull
    try:
        dev = tally.reconstruct(tr)
        dev_counts = tally.accuracy_counts(tr, dirty, clean) if not (tally.plan.host_strings or tally.plan.numeric) else None
    finally:
        Engine.pull = real_pull
    still_ahead = tr._dev is eng
    if dev_counts is None:
        dev_counts = tally.accuracy_counts(tr, dirty, clean)  # (the host part of a mixed plan reads the trace)
    host = analysis.reconstructed_pool_ids(lw, tr)
    host_counts = analysis.accuracy_counts(lw, tr, dirty, clean)
    again = tally.reconstruct(tr)  # the host arrays are current now
    return dict(lw=lw, eng=eng, tr=tr, tally=tally, dirty=dirty, clean=clean, ahead=ahead, still_ahead=still_ahead, dev=dev,
                host=host, dev_counts=dev_counts, host_counts=host_counts, again=again, init_dev=init_dev, init_host=init_host,
                cfg=cfg)


@pytest.fixture(scope="module")
def programs():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _program_state(name)
        return made[name]
    yield get
    for st in made.values():
        st["tally"].close()
        st["eng"].close()


# ---- 2. reconstruction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hospital", "flights", "rents"])
def test_reconstruction_equals_host(programs, name):
    st = programs(name)
    want_cols = {"hospital": 15, "flights": 6, "rents": 3}[name]
    assert len(st["tally"].columns) == want_cols
    for key, ref in (("dev", "host"), ("again", "host"), ("init_dev", "init_host")):
        for col in st["tally"].columns:
            got = st[key][col]
            assert got.dtype == np.int32 and np.array_equal(got, st[ref][col]), (name, key, col)


def test_reconstruction_reads_device_state_without_pull(programs):
    """hospital after one iteration: the sweep was committed on the device, the host arrays are behind — the reconstruction
    (and the counters) ran with Engine.pull made to raise and left the trace behind the device."""
    st = programs("hospital")
    assert st["ahead"] and st["still_ahead"]


@pytest.mark.parametrize("n_rows", [1, 257])
def test_reconstruction_row_counts(n_rows):
    """one row, and one row more than a workgroup (1000 rows: test_reconstruction_equals_host)"""
    S = helpers.hospital_setup(n_rows=n_rows)
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        tally = CellTally(eng, S["trace"])
        got = tally.reconstruct(S["trace"])
        want = analysis.reconstructed_pool_ids(S["lw"], S["trace"])
        assert sorted(got) == sorted(want)
        for col in want:
            assert got[col].shape == (n_rows,) and np.array_equal(got[col], want[col]), col
        cnt = tally.accuracy_counts(S["trace"], S["dirty"], S["clean"])
        assert np.array_equal(cnt, analysis.accuracy_counts(S["lw"], S["trace"], S["dirty"], S["clean"]))
        tally.close()
    finally:
        eng.close()


def test_rows_without_referent_yield_minus_one():
    S = helpers.hospital_setup(n_rows=257)
    lw, tr = S["lw"], S["trace"]
    eng = Engine(lw, S["obs"], dist_mode=1)
    try:
        tally = CellTally(eng, tr)
        base = tally.reconstruct(tr)
        tr2 = copy.deepcopy(tr)
        holes = np.array([0, 63, 64, 200, 256])
        tr2.cur[0, holes] = -1
        got = tally.reconstruct(tr2)
        block0 = [c for c, rc in zip(tally.plan.columns, tally.plan.cols) if rc.block == 0 or (rc.kind == 1 and rc.block_b == 0)]
        assert 0 < len(block0) < len(tally.columns)
        for col in tally.columns:
            want = base[col].copy()
            if col in block0:
                want[holes] = -1
            assert np.array_equal(got[col], want), col
        tally.close()
    finally:
        eng.close()


# ---- 3. counters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hospital", "flights", "rents"])
def test_accuracy_counts_equal_host(programs, name):
    st = programs(name)
    assert st["dev_counts"].dtype == np.int64 and st["dev_counts"].shape == (5,)
    assert np.array_equal(st["dev_counts"], st["host_counts"]), (st["dev_counts"], st["host_counts"])
    assert st["host_counts"][0] > 0 and st["host_counts"][1] > 0
    if name == "rents":  # the mixed path: device columns + own choices and the numeric column on the host
        assert st["tally"].plan.host_strings and st["tally"].plan.numeric


# ---- 4. ring and wrap-around ---------------------------------------------------------------------------------------------
def test_ring_wraps_and_consensus_equals_restatement(programs):
    st = programs("hospital")
    lw, eng = st["lw"], st["eng"]
    tr = st["tr"]
    cfg = st["cfg"]
    t3, t1 = CellTally(eng, tr, keep=3), CellTally(eng, tr, keep=1)
    try:
        with pytest.raises(ValueError):
            t3.consensus()
        snaps, kept = [], []
        for k in range(5):
            if k:
                inf.run_inference(eng, tr, cfg, 100 + k)
            t3.add(tr)
            t1.add(tr)
            kept.append(t3.n_kept)
            snaps.append(analysis.reconstructed_pool_ids(lw, tr))
        assert kept == [1, 2, 3, 3, 3] and t1.n_kept == 1
        assert any(not np.array_equal(snaps[2][c], snaps[4][c]) for c in t3.columns)  # (the samples do differ)
        ids, sup = t3.consensus()
        assert list(ids) == list(lw.query.cleanmap) == list(sup)
        for col in ids:
            want = mode_support(np.stack([s[col] for s in snaps[-3:]]))
            assert np.array_equal(ids[col], want[0]) and np.array_equal(sup[col], want[1]), col
        ids1, sup1 = t1.consensus()
        for col in ids1:
            assert np.array_equal(ids1[col], snaps[-1][col]) and (sup1[col] == 1).all()
        # the counters over a table of consensus values: keep = 1 is the last sample's F1
        acc = t1.consensus_accuracy(st["dirty"], st["clean"])
        assert acc == analysis.f1_from_counts(analysis.accuracy_counts(lw, tr, st["dirty"], st["clean"]))
        want3 = analysis.counts_given(lw, {c: ids[c].astype(np.int64) for c in ids}, tr.cur.shape[1], st["dirty"], st["clean"])
        assert t3.consensus_accuracy(st["dirty"], st["clean"]) == analysis.f1_from_counts(want3)
        table = analysis.consensus_table(lw, t3, st["dirty"])
        assert table["City"] == [lw.pool.strings[i] for i in ids["City"]] and table["City__support"] == sup["City"].tolist()
    finally:
        t3.close()
        t1.close()


def test_keep_out_of_range_raises(programs):
    st = programs("hospital")
    for keep in (0, 33):
        with pytest.raises(ValueError):
            CellTally(st["eng"], st["tr"], keep=keep)


# ---- 5. a rebuilt string pool --------------------------------------------------------------------------------------------
def test_relower_translates_kept_snapshots():
    """flights with prior proposals: every iteration chooses TimePrior dummies, their drawn strings join the domains
    (LoweredModel.relower rebuilds the pool, ids move) — between two adds (tests/test_tally_cpu.py checks the seed on the
    CPU).  The consensus equals the restatement over host reconstructions taken at the same moments, translated to the
    final pool's ids by string."""
    dirty, clean = ex.flights_data()
    m = ex.flights_model(dirty)
    lw = LoweredModel(m, ex.flights_query(m), dirty)
    obs = lw.encode_observations(dirty)
    eng = Engine(lw, obs, dist_mode=1)
    try:
        tr = Trace(lw, obs.shape[1], RELOWER_SEED)
        cfg = relower_config()
        inf.initialize_trace(eng, tr, cfg, RELOWER_SEED, max_batch=512)
        tally = CellTally(eng, tr, keep=4)

        class Both:
            def __init__(self):
                self.host = []

            def add(self, trace):
                tally.add(trace)
                self.host.append((analysis.reconstructed_pool_ids(lw, trace), list(lw.pool.strings), eng.reloads))

        both = Both()
        inf.run_inference(eng, tr, cfg, RELOWER_SEED, tally=both)
        assert len(both.host) == 4 and tally.n_kept == 4
        first, last = both.host[0][1], list(lw.pool.strings)
        assert both.host[-1][2] > both.host[0][2] and last[:len(first)] != first  # reloads between the adds moved ids
        ids, sup = tally.consensus()
        index = lw.pool.index
        for col in ids:
            stack = []
            for snap, strings, _ in both.host:
                v = np.asarray(snap[col])
                stack.append(np.array([index[strings[i]] if i >= 0 else i for i in v], dtype=np.int32))
            want = mode_support(np.stack(stack))
            assert np.array_equal(ids[col], want[0]) and np.array_equal(sup[col], want[1]), col
        acc = tally.consensus_accuracy(dirty, clean)
        want = analysis.counts_given(lw, {c: ids[c].astype(np.int64) for c in ids}, tr.cur.shape[1], dirty, clean)
        assert acc == analysis.f1_from_counts(want)
        tally.close()
    finally:
        eng.close()


# ---- 6. the sampler's results do not change ---------------------------------------------------------------------------------
def test_tally_changes_no_result():
    S = helpers.hospital_setup(n_rows=400)
    lw, obs = S["lw"], S["obs"]
    cfg = InferenceConfig(3, 2, use_mh_instead_of_pg=True)
    out = []
    for with_tally in (False, True):
        eng = Engine(lw, obs, dist_mode=1)
        try:
            tr = Trace(lw, obs.shape[1], 3)
            inf.initialize_trace(eng, tr, cfg, 3)
            tally = CellTally(eng, tr, keep=2) if with_tally else None
            inf.run_inference(eng, tr, cfg, 3, tally=tally, tally_from=1)
            if tally is not None:
                assert tally.n_kept == 2
                tally.consensus()
                tally.close()
            tr.check_consistency()
            out.append(tr)
        finally:
            eng.close()
    a, b = out
    assert np.array_equal(a.cur, b.cur)
    assert sorted(a.tables) == sorted(b.tables)
    for cname in a.tables:
        ta, tb = a.tables[cname], b.tables[cname]
        assert ta.n == tb.n and ta.free == tb.free, cname
        assert np.array_equal(ta.cols[:, :ta.n], tb.cols[:, :tb.n]) and np.array_equal(ta.counts[:ta.n], tb.counts[:tb.n]), cname
        assert np.array_equal(ta.live[:ta.n], tb.live[:tb.n]), cname
