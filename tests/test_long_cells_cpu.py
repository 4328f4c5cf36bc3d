"""tests/long_cell_program.py on the CPU oracle alone: the program has the shape tests/test_gpu_long_cells.py relies on,
and the comparison made there has the power to see a scorer that takes the 8-bit load on the 16-bit table."""
import numpy as np

import helpers
import long_cell_program as lcp
from pclean_amd._lib import InferConfig


def _world(oracle, S, note_table=None):
    lw = S["lw"]
    w = helpers.mirror_world(oracle, lw, S["obs"], S["trace"], None, dist_mode=1,
                             option_logp=helpers.option_logp_cpu(oracle, lw, S["trace"]))
    if note_table is not None:
        pid, odom, ldom = lcp.pair_ids(lw)["note"]
        w.set_pair(pid, note_table, lw.pool.lens[ldom.id_array()].astype(np.uint16))
    return w


def test_string_prior_beyond_255_is_refused_by_name():
    """why note is no StringPrior in this program: the lowering refuses max_length > 255 (the device's dummy draws)"""
    import pytest
    from pclean_amd.model import LoweredModel
    m, q, dirty = lcp.refused_program()
    with pytest.raises(NotImplementedError, match=r"Ent\.note: StringPrior lengths beyond 255 do not fit the dummy specification"):
        LoweredModel(m, q, dirty)


def test_program_shape(oracle):
    S = lcp.long_cell_setup()
    lw, tr = S["lw"], S["trace"]
    assert S["obs"].shape[1] == lcp.N_ENT * lcp.ROWS_PER and tr.tables["Ent"].n == lcp.N_ENT
    sym, off, _, _ = lw.pool.arrays()
    ids = lcp.pair_ids(lw)
    name = oracle.pair_table(sym, off, ids["name"][1].id_array(), ids["name"][2].id_array(), 1)
    note = oracle.pair_table(sym, off, ids["note"][1].id_array(), ids["note"][2].id_array(), 1)
    assert name.max() <= 255 < note.max()
    lens = lw.pool.lens[ids["note"][2].id_array()]
    assert sorted(lens[lens > 255])[:1] == [256] and lens.max() <= 310 and (lens > 255).sum() >= 5
    assert any(v is None for v in S["dirty"]["NAME"]) and any(v is None for v in S["dirty"]["NOTE"])
    # typos in the long cells: rows of the long entities whose note is neither missing nor the clean value
    damaged = [i for i, e in enumerate(S["owner"]) if e in lcp.LONG_ENTS and S["dirty"]["NOTE"][i] not in (None, S["ents"][e]["note"])]
    assert len(damaged) >= 4
    tr.check_consistency()


def test_a_scorer_on_the_wrong_load_branch_would_be_seen(oracle):
    """The oracle's sweep with the note table's bytes read as 8-bit entries (what a kernel does that takes the
    elem_bytes == 1 load on this table) differs from the right one, under MH and under PG: the comparison of
    tests/test_gpu_long_cells.py fails on such a kernel.  Truncating the distances to their low byte is seen too."""
    from test_gpu_edges import _oracle_sweep
    S = lcp.long_cell_setup()
    lw, tr = S["lw"], S["trace"]
    sym, off, _, _ = lw.pool.arrays()
    pid, odom, ldom = lcp.pair_ids(lw)["note"]
    note = oracle.pair_table(sym, off, odom.id_array(), ldom.id_array(), 1)
    for mh, P in ((1, 2), (0, 4)):
        c = InferConfig(1, P, 1, 1, mh, 50, 100)
        good = _oracle_sweep(oracle, _world(oracle, S), c, 11, 0, tr.cur)
        for what, bad_table in (("bytes", lcp.bytes_of_a_16bit_table(note)), ("low byte", note & 0xff)):
            bad = _oracle_sweep(oracle, _world(oracle, S, bad_table), c, 11, 0, tr.cur)
            rows = np.flatnonzero((good[0] != bad[0]).any(axis=0) | (good[1] != bad[1]) | (good[2] != bad[2]))
            print(f"[power, mh={mh}, {what}] {len(rows)} of {len(good[1])} rows differ")
            assert len(rows) >= 1, (mh, what)
