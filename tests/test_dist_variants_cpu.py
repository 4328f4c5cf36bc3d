"""The tables of tests/test_gpu_dist_variants.py on the oracle alone: every case builds to the shape it names, and the
strings can tell a kernel that drops the high byte of a symbol id from a right one."""
import numpy as np
import pytest

import test_gpu_dist_variants as dv


@pytest.mark.parametrize("case", dv.BITPAR, ids=[c[5] for c in dv.BITPAR])
def test_bitpar_cases_build_to_their_shape_and_see_truncated_symbols(oracle, case):
    max_la, max_lb, n_symbols, n_obs, n_lat, slot = case
    sym, off, oi, li = dv.make_case(1000 + max_la, n_symbols, max_la, max_lb, n_obs, n_lat)  # (asserts the shape)
    lens = off[1:] - off[:-1]
    # the instantiation the dispatcher's rule gives for this shape (pclean_launch_dist, restated)
    W = max(1, (max_la + 63) // 64)
    s16, o16 = n_symbols > 255, max(max_la, max_lb) > 255
    assert slot == f"osa_bitpar_{W}_s{16 if s16 else 8}_o{16 if o16 else 8}"
    assert n_symbols * W * 8 + max(max_lb, 1) * 256 * (2 if s16 else 1) <= 160 * 1024, "beyond the kernel's LDS: another kernel runs"
    assert 0 in lens[oi] or n_obs == 1
    assert len(set(oi.tolist())) < len(oi) or n_obs < 4, "no duplicate id"
    if n_symbols > 256:
        want = oracle.pair_table(sym, off, oi, li, 0)
        cut = oracle.pair_table(sym & 0xff, off, oi, li, 0)
        assert (want != cut).any(), "symbol ids cut to 8 bits give the same table: the strings do not use the high byte"


def test_near_copies_hold_the_edits_at_the_word_boundaries():
    work = list("abcdef")
    w = dv._base(np.random.default_rng(0), work, 256)
    near = dv._near(w, work)
    swaps = [next(i for i in range(256) if s[i] != w[i]) for s in near[:4]]
    assert swaps == [63, 127, 191, 254] and all(s[p + 1] == w[p] and s[p] == w[p + 1] for s, p in zip(near[:4], swaps))
    assert near[5][:255] == w[:255] and near[5][255] != w[255]          # substitution in the last position
    assert near[6][:5] == w[:5] and near[6][6:] == w[5:255]              # insertion: every later symbol one position up
    assert len(near[7]) == 255 and all(len(s) <= 256 for s in near)
