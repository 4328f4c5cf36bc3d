"""Every instantiation of the pair-table builders (pclean_launch_dist in csrc/dist_kernels.hip) against the oracle's DP,
with pclean_debug_dist_launches saying which instantiation built each table.

The dispatcher picks a kernel from the table's shape: longest observed string (max_la), longest latent string (max_lb),
number of distinct symbols of the loaded pool (n_symbols) and the distance flavour.  Each case below is built to a shape
that lands on ONE instantiation, asserts that this slot and no other was hit, and compares the whole table with
oracle.pair_table (integers: np.array_equal, no tolerance).  The last test asserts that the cases together hit all
PCLEAN_DIST_LAUNCH_SLOTS slots.

How the sizes were chosen.  The launch geometry has three boundaries: a workgroup takes 256 latent strings (fewer in the
DL kernels), a workgroup walks a chunk of 64 / 32 / 16 observed strings, and the bit-parallel kernel keeps 64 pattern
positions per word.  So n_lat is one of 1, 255, 256, 257, 300, n_obs one of 1, 64, 65, 70, and the longest observed
string sits exactly on 1, 64, 65, 128, 129, 192, 193, 255, 256.  The oracle's DP is quadratic in the string lengths, so a
table holds only a handful of strings at its class maximum (the base string, its near copies, and on the latent side the
observed near copies) and fills up with strings of 0 .. 40 symbols: a table costs the oracle well under a second.  Both
sides hold the empty string and one duplicate id.  The near copies are those of test_pair_table_long_patterns_and_dl_random:
adjacent transpositions straddling positions 63/64, 127/128 and 191/192 and at the end of the string, a substitution in
the last position, an insertion that shifts every later match by one (across the word boundaries), a deletion.  Symbol
ids are made to matter: the pool's first string holds the whole alphabet, so a character's symbol id is its position in
it, and the strings draw from ids 0, 1, 2, 255, 256, 257 and the two highest, so that with more than 256 symbols ids 0 /
256 and 1 / 257 differ only above bit 7."""
import numpy as np
import pytest

from pclean_amd._lib import HipContext, PCleanHipError
from pclean_amd.encode import StringPool

pytestmark = pytest.mark.gpu

_HIT = {}  # slot name -> the test that hit it (read by the closing test)


def _alphabet(n):
    return [chr(0x61 + k) if k < 26 else chr(0x4e00 + k) for k in range(n)]


def _working_set(alpha):
    n = len(alpha)
    return [alpha[k] for k in sorted({0, 1, 2, n - 2, n - 1} | ({255, 256, 257} & set(range(n))))]


def _base(rnd, work, n):
    """a random string of n symbols whose adjacent pairs at the word boundaries and at the end differ (so that swapping
    them is an edit)"""
    w = [work[int(k)] for k in rnd.integers(0, len(work), size=n)]
    for pos in (63, 127, 191, n - 2):
        if 0 <= pos < n - 1 and w[pos] == w[pos + 1]:
            w[pos + 1] = work[(work.index(w[pos]) + 1) % len(work)]
    return w


def _near(w, work):
    """near copies of w, none longer than w"""
    n, out = len(w), []
    other = lambda ch: work[(work.index(ch) + 1) % len(work)]
    every = list(w)
    for pos in (63, 127, 191, n - 2):
        if 0 <= pos < n - 1:
            s = list(w)
            s[pos], s[pos + 1] = s[pos + 1], s[pos]
            out.append(s)
            every[pos], every[pos + 1] = every[pos + 1], every[pos]
    out.append(every)
    if n >= 1:
        s = list(w)
        s[-1] = other(s[-1])  # substitution in the last position of the pattern
        out.append(s)
    if n >= 8:
        s = list(w)
        s.insert(5, other(s[5]))  # insertion: every later match moves one position up, across the word boundaries
        out.append(s[:n])
        s = list(w)
        del s[3]
        out.append(s)
    return out


def _mutate(rnd, s, work):
    s = list(s)
    for _ in range(int(rnd.integers(0, 3))):
        k = int(rnd.integers(0, 3))
        if k == 0 and len(s) >= 2:
            q = int(rnd.integers(0, len(s) - 1))
            s[q], s[q + 1] = s[q + 1], s[q]
        elif k == 1:
            s.insert(int(rnd.integers(0, len(s) + 1)), work[int(rnd.integers(len(work)))])
        elif s:
            s[int(rnd.integers(len(s)))] = work[int(rnd.integers(len(work)))]
    return s


def _side(rnd, work, shorts, max_len, n, extra=()):
    """n strings, the longest exactly max_len: the base string, the empty string, the base's near copies, `extra` cut to
    max_len, then mutated copies of the shared short strings; the last one repeats the first (a duplicate id)"""
    w = _base(rnd, work, max_len)
    out = [w, []] + _near(w, work) + [list(e)[:max_len] for e in extra]
    k = 0
    while len(out) < n:
        out.append(_mutate(rnd, shorts[k % len(shorts)], work)[:max_len])
        k += 1
    out = out[:n]
    if n >= 4:
        out[-1] = out[0]
    return ["".join(s) for s in out]


def make_case(seed, n_symbols, max_la, max_lb, n_obs, n_lat):
    rnd = np.random.default_rng(seed)
    alpha = _alphabet(n_symbols)
    work = _working_set(alpha)
    shorts = [[work[int(k)] for k in rnd.integers(0, len(work), size=int(rnd.integers(0, 41)))] for _ in range(120)]
    obs = _side(rnd, work, shorts, max_la, n_obs)
    lat = _side(rnd, work, shorts, max_lb, n_lat, extra=obs[:10])
    pool = StringPool()
    pool.add("".join(alpha))  # fixes the symbol ids and the pool's symbol count; in no table
    oi, li = pool.add_all(obs), pool.add_all(lat)
    sym, off, _, _ = pool.arrays()
    assert int(sym.max()) + 1 == n_symbols
    assert int(pool.lens[oi].max()) == max_la and int(pool.lens[li].max()) == max_lb
    assert len(oi) == n_obs and len(li) == n_lat
    return sym, off, oi, li


def check_table(hip, oracle, who, sym, off, oi, li, mode, expect, table_id=50):
    """build, assert the slots hit are exactly `expect`, compare with the oracle; returns the table"""
    hip.load_strings(sym, off)
    hip.dist_launches(reset=True)
    hip.build_pair_table(table_id, oi, li, mode)
    got = hip.get_pair_table(table_id, len(oi), len(li))
    hit = {k for k, v in hip.dist_launches(reset=True).items() if v}
    assert hit == set(expect), (who, sorted(hit))
    want = oracle.pair_table(sym, off, oi, li, mode)
    assert np.array_equal(got, want), (who, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
    for k in hit:
        _HIT.setdefault(k, who)
    return got


# (max_la, max_lb, n_symbols, n_obs, n_lat) -> the instantiation.  8-bit output: no string above 255; 16-bit output: an
# observed maximum of 256, or an observed maximum of at most 64 W with a latent string of 300.  The last case sits under
# the kernel's LDS ceiling: 318 symbols * 4 words * 8 bytes + 300 * 256 * 2 bytes = 163 776 of 163 840 bytes.
BITPAR = [
    (1, 40, 255, 70, 256, "osa_bitpar_1_s8_o8"),
    (64, 255, 256, 64, 257, "osa_bitpar_1_s16_o8"),
    (128, 255, 255, 70, 300, "osa_bitpar_2_s8_o8"),
    (65, 80, 256, 65, 255, "osa_bitpar_2_s16_o8"),
    (129, 140, 255, 1, 300, "osa_bitpar_3_s8_o8"),
    (192, 200, 300, 65, 1, "osa_bitpar_3_s16_o8"),
    (255, 255, 255, 70, 257, "osa_bitpar_4_s8_o8"),
    (193, 255, 300, 64, 256, "osa_bitpar_4_s16_o8"),
    (64, 300, 255, 65, 257, "osa_bitpar_1_s8_o16"),
    (40, 300, 300, 70, 256, "osa_bitpar_1_s16_o16"),
    (128, 300, 255, 64, 255, "osa_bitpar_2_s8_o16"),
    (65, 300, 256, 70, 300, "osa_bitpar_2_s16_o16"),
    (192, 300, 255, 65, 256, "osa_bitpar_3_s8_o16"),
    (129, 300, 300, 64, 257, "osa_bitpar_3_s16_o16"),
    (256, 100, 255, 65, 255, "osa_bitpar_4_s8_o16"),
    (256, 256, 256, 64, 300, "osa_bitpar_4_s16_o16"),
    (255, 300, 318, 70, 257, "osa_bitpar_4_s16_o16"),
]


@pytest.mark.parametrize("max_la,max_lb,n_symbols,n_obs,n_lat,slot", BITPAR, ids=[f"{c[5]}-la{c[0]}-lb{c[1]}-sym{c[2]}" for c in BITPAR])
def test_osa_bitpar_every_instantiation(hip, oracle, max_la, max_lb, n_symbols, n_obs, n_lat, slot):
    """osa_bitpar_kernel<W, SymT, OutT>, all 16: W from the longest observed string on both sides of every word boundary,
    SymT from 255 / 256 / 300 distinct symbols, OutT from the longest string of either side."""
    sym, off, oi, li = make_case(1000 + max_la, n_symbols, max_la, max_lb, n_obs, n_lat)
    got = check_table(hip, oracle, f"test_osa_bitpar_every_instantiation[{slot}]", sym, off, oi, li, 0, [slot])
    if slot.endswith("o16"):
        # the empty string against the longest one: a distance no byte holds
        assert int(got.max()) == max(max_la, max_lb) > 255


def test_osa_bitpar_covers_every_word_boundary_and_symbol_count():
    """the boundaries the cases above are required to hold (a table of contents, checked)"""
    assert {c[0] for c in BITPAR} >= {1, 64, 65, 128, 129, 192, 193, 255, 256}
    assert {c[2] for c in BITPAR} >= {255, 256, 300}
    assert {c[4] for c in BITPAR} >= {1, 255, 256, 257, 300} and {c[3] for c in BITPAR} >= {1, 64, 65, 70}
    assert len({c[5] for c in BITPAR}) == 16


def _tile_lds(max_la, max_lb, t=64):
    """LDS bytes of osa_tile_kernel at its smallest workgroup (pclean_launch_dist: lds_bytes)"""
    return ((3 * max_lb + 2) * t + max_la + 8) * 2


def test_osa_tile_8bit_when_the_match_masks_do_not_fit_lds(hip, oracle):
    """2 200 distinct symbols, observed strings of up to 200 (four words), latent ones of up to 255: the bit-parallel
    kernel would need 2200 * 4 * 8 + 255 * 256 * 2 = 200 960 bytes of LDS (> 160 KiB), so the 8-bit table falls through to
    osa_tile_kernel<uint8_t>; 130 latent strings are three of its 64-lane workgroups, the last one partial."""
    assert 2200 * 4 * 8 + 255 * 256 * 2 > 160 * 1024
    sym, off, oi, li = make_case(7, 2200, 200, 255, 20, 130)
    check_table(hip, oracle, "test_osa_tile_8bit_when_the_match_masks_do_not_fit_lds", sym, off, oi, li, 0, ["osa_tile_o8"])


def test_osa_tile_16bit_and_its_capacity_refusal(hip, oracle):
    """Observed strings above 256 symbols go to osa_tile_kernel<uint16_t>.  With observed strings of 300 symbols its LDS,
    ((3 max_lb + 2) * 64 + max_la + 8) * 2 bytes, fits 160 KiB up to latent strings of 424 symbols: that table is built and
    compared; one symbol more is refused with PCLEAN_ERR_CAPACITY and its message, launches nothing, and leaves the context
    usable."""
    sym, off, oi, li = make_case(8, 300, 300, 260, 6, 70)
    got = check_table(hip, oracle, "test_osa_tile_16bit_and_its_capacity_refusal", sym, off, oi, li, 0, ["osa_tile_o16"])
    assert int(got.max()) == 300
    top = next(lb for lb in range(256, 2000) if _tile_lds(300, lb + 1) > 160 * 1024)
    assert top == 424 and _tile_lds(300, top) <= 160 * 1024
    sym, off, oi, li = make_case(9, 40, 300, top, 3, 14)
    check_table(hip, oracle, "test_osa_tile_16bit_and_its_capacity_refusal[largest]", sym, off, oi, li, 0, ["osa_tile_o16"])
    sym, off, oi, li = make_case(9, 40, 300, top + 1, 3, 14)
    hip.load_strings(sym, off)
    hip.dist_launches(reset=True)
    with pytest.raises(PCleanHipError) as err:
        hip.build_pair_table(51, oi, li, 0)
    assert "status -5" in str(err.value)
    assert f"pair table strings too long for the OSA tile kernel ({top + 1})" in str(err.value)
    assert not any(hip.dist_launches(reset=True).values())
    # the same table without the strings of top + 1 symbols: built as before
    keep = li[(off[1:] - off[:-1])[li] <= top]
    assert len(keep) >= 5 and int((off[1:] - off[:-1])[keep].max()) == top
    hip.build_pair_table(50, oi, keep, 0)
    assert np.array_equal(hip.get_pair_table(50, len(oi), len(keep)), oracle.pair_table(sym, off, oi, keep, 0))


def _dl_strings(rnd, work, lens):
    base = [[work[int(k)] for k in rnd.integers(0, len(work), size=n)] for n in lens]
    out = []
    for w in base:  # near copies: adjacent and gapped transpositions, substitutions (the dl_seg test's construction)
        c = list(w)
        for _ in range(int(rnd.integers(1, 4))):
            if len(c) > 3:
                q = int(rnd.integers(0, len(c) - 2))
                c[q], c[q + 1] = c[q + 1], c[q]
                if rnd.random() < 0.5:
                    c.insert(q + 1, work[int(rnd.integers(len(work)))])
                if rnd.random() < 0.5:
                    c[int(rnd.integers(len(c)))] = work[int(rnd.integers(len(work)))]
        out.append(c[:len(w)])
    return ["".join(s) for s in base + out]


def _dl_case(seed, n_symbols, lens, n_obs, obs_top=None):
    """latent side: strings of the given lengths and a near copy of each (no longer); observed side: every other one of
    them, n_obs in all, none longer than obs_top; the last id of each side repeats its first"""
    rnd = np.random.default_rng(seed)
    alpha = _alphabet(n_symbols)
    words = _dl_strings(rnd, _working_set(alpha), lens)
    pool = StringPool()
    pool.add("".join(alpha))
    li = pool.add_all(words)
    sym, off, _, _ = pool.arrays()
    cand = li if obs_top is None else li[pool.lens[li] <= obs_top]
    oi = cand[::2][:n_obs].copy()
    assert len(oi) == n_obs
    li[-1], oi[-1] = li[0], oi[0]
    assert int(sym.max()) + 1 == n_symbols
    return sym, off, oi, li, pool


@pytest.mark.parametrize("n_symbols", [6, 300], ids=["sym8", "sym16"])
def test_dl_seg_every_instantiation(hip, oracle, n_symbols):
    """dl_seg_kernel<NSEG, SymT>, mode 1, no switch set: one table holds every length class (<= 32, <= 64, <= 128, <= 254
    symbols: 1 / 2 / 4 / 8 lanes per pair) on both sides of its boundaries, and 40 strings above 128 symbols are more than
    the 32 pairs of an eight-lane workgroup; 33 observed strings are two chunks of 32."""
    rnd = np.random.default_rng(3)
    lens = [254, 0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 253] + [int(x) for x in rnd.integers(129, 255, size=7)] + \
        [int(x) for x in rnd.integers(0, 129, size=30)]
    sym, off, oi, li, _ = _dl_case(4, n_symbols, lens, 33)
    s = "s8" if n_symbols <= 255 else "s16"
    check_table(hip, oracle, f"test_dl_seg_every_instantiation[{s}]", sym, off, oi, li, 1, [f"dl_seg_{n}_{s}" for n in (1, 2, 4, 8)])
    # one of the two row lengths is no multiple of four (the un-permutation's byte path)
    assert len(li) % 4 == 0
    check_table(hip, oracle, f"test_dl_seg_every_instantiation[{s}]", sym, off, oi, li[:-1], 1,
                [f"dl_seg_{n}_{s}" for n in (1, 2, 4, 8)])


def test_dl_wave_in_its_production_position(hip, oracle, monkeypatch):
    """A table whose longest string is exactly 255 symbols, nothing longer, no switch set: dl_seg_kernel declines (254 is
    its limit) and dl_wave_kernel<64,4> builds the 8-bit table, two pairs per workgroup."""
    monkeypatch.delenv("PCLEAN_DL_KERNEL", raising=False)
    rnd = np.random.default_rng(5)
    lens = [255, 0, 1, 64, 65, 128, 129, 192, 193, 254] + [int(x) for x in rnd.integers(0, 41, size=25)]
    sym, off, oi, li, pool = _dl_case(6, 6, lens, 33)
    assert int(pool.lens[li].max()) == 255 == int(pool.lens[oi].max())
    check_table(hip, oracle, "test_dl_wave_in_its_production_position", sym, off, oi, li, 1, ["dl_wave_64_4"])


@pytest.mark.parametrize("top,slot", [(16, "dl_wave_16_1"), (32, "dl_wave_32_1"), (64, "dl_wave_64_1"), (128, "dl_wave_64_2"),
                                      (192, "dl_wave_64_3")])
def test_dl_wave_other_instantiations_under_the_switch(hip, oracle, monkeypatch, top, slot):
    """PCLEAN_DL_KERNEL=wave with latent strings of at most 16 / 32 / 64 / 128 / 192 symbols: 4 / 2 / 1 pairs per wavefront,
    1 / 2 / 3 column chunks per lane; the longest latent string sits on the class boundary, 300 symbols are the 16-bit case
    of the symbol compare."""
    rnd = np.random.default_rng(top)
    lens = [top, 0, 1, top - 1, top // 2, top // 2 + 1] + [int(x) for x in rnd.integers(0, min(top, 40) + 1, size=31)]
    sym, off, oi, li, pool = _dl_case(top, 300, lens, 33)
    assert int(pool.lens[li].max()) == top
    monkeypatch.setenv("PCLEAN_DL_KERNEL", "wave")
    check_table(hip, oracle, f"test_dl_wave_other_instantiations_under_the_switch[{slot}]", sym, off, oi, li, 1, [slot])


def test_dl_pair_16bit_in_its_production_position(hip, oracle, monkeypatch):
    """Strings above 255 symbols, mode 1, no switch set: the 16-bit table is built by dl_pair_kernel<uint16_t> (150 pairs:
    three workgroups of 64 lanes, the last one partial)."""
    monkeypatch.delenv("PCLEAN_DL_KERNEL", raising=False)
    rnd = np.random.default_rng(12)
    lens = [300, 0, 256, 255, 257] + [int(x) for x in rnd.integers(0, 41, size=10)]
    sym, off, oi, li, pool = _dl_case(13, 6, lens, 5, obs_top=300)
    assert len(oi) * len(li) == 150
    got = check_table(hip, oracle, "test_dl_pair_16bit_in_its_production_position", sym, off, oi, li, 1, ["dl_pair_o16"])
    assert int(got.max()) > 255


def test_dl_ladder_on_one_table(hip, oracle, monkeypatch):
    """One table, every string of at most 40 symbols (the LDS-matrix kernel's matrix fits), through dl_seg_kernel,
    dl_wave_kernel, dl_lds_kernel and dl_pair_kernel<uint8_t>: each against the oracle, all four identical.  300 latent
    strings and 70 observed ones cross the workgroup and chunk boundaries of all four."""
    rnd = np.random.default_rng(21)
    lens = [40, 0, 1, 32, 33, 39] + [int(x) for x in rnd.integers(0, 41, size=144)]
    sym, off, oi, li, pool = _dl_case(22, 6, lens, 70)
    assert len(li) == 300 and int(pool.lens[li].max()) == 40
    tabs = []
    for switch, expect in (("seg", ["dl_seg_1_s8", "dl_seg_2_s8"]), ("wave", ["dl_wave_64_1"]), ("lds", ["dl_lds"]),
                           ("pair", ["dl_pair_o8"])):
        monkeypatch.setenv("PCLEAN_DL_KERNEL", switch)
        tabs.append(check_table(hip, oracle, f"test_dl_ladder_on_one_table[{switch}]", sym, off, oi, li, 1, expect))
    for t in tabs[1:]:
        assert np.array_equal(tabs[0], t)


def test_every_table_kernel_instantiation_was_run():
    """The condition this file exists for: the tests above (run as a file) hit every slot of pclean_debug_dist_launches.
    No slot is exempt."""
    missing = [k for k in HipContext.DIST_LAUNCH_SLOTS if k not in _HIT]
    assert not missing, f"table kernels no test of this file ran: {missing}"
    assert set(_HIT) == set(HipContext.DIST_LAUNCH_SLOTS) and len(HipContext.DIST_LAUNCH_SLOTS) == 35
