"""Small programs for the memo of option-list marginals (eval.hip: eval_node_lse, memo_lookup_kernel, memo_insert_kernel),
shared by test_memo_program_cpu.py and test_gpu_leaf_memo.py.  Each program has exactly ONE open (non-cacheable) option
list under the reference slot that the tests score, so that the oracle's score_node of the slot can take the leaf's
log-marginal as `snew` (enum_variants_program.oracle_fk does the same):

  cols(k)   A.x ~ ChooseUniformly(words); Obs.a -> A; y1 .. yk ~ AddTypos(a.x): the leaf has k terms, the key k columns
            (k = 6: the third word of the stored key decides; k = 7: more values than the key holds, no memo);
  ctx2      block 0: a -> A, y0 ~ AddTypos(a.x); block 1: b -> B, w ~ AddTypos(b.z), v ~ AddTypos(j) with
            j = f(a.x, b.z): the leaf of B.z reads a ctx value, its key is 2 columns + PCLEAN_MAX_CTX ctx words = 6.
            (The lowering takes a ctx value from an EARLIER block, so the slot the tests score is block 1's.)
  tab       A.x as in cols; y1 ~ FormatName(a.x), y2, y3 ~ AddTypos(a.x): an open leaf with a tabulated term.  The frozen
            oracle does not know tabulated terms (tests/tabulated_program.py); the tests say what they compare it with.
  two       block 0: a -> A, y1, y2 ~ AddTypos(a.x); block 1: b -> B over the same words, w1, w2 ~ AddTypos(b.z), with
            the SAME strings in w1, w2 as in y1, y2: two open leaves whose tuples coincide as integers.

Data: a dozen options of 4-8 letters over "abcdefgh"; per observed column a pool of 200 strings that are not options
(_pool); one row in 97 has every cell missing, single cells are missing or hold an option; every 16th row repeats the
tuple of the row three before it (two inserts of one key in one launch); a quarter of the rows belong to families that
share some columns and differ in the others (family_of).  One table of N_ROWS rows and three row lists: FIRST (4 608
rows), AGAIN (the same) and SHIFTED (the second half of FIRST + as many new rows)."""
import numpy as np

from pclean_amd.model import AddTypos, ChooseUniformly, FormatName, LoweredModel, Model, Query
from pclean_amd.trace import Trace

LETTERS = list("abcdefgh")
POOL = 200
N_OPTIONS = 12
N_FIRST = 4608
N_ROWS = N_FIRST + N_FIRST // 2
FIRST = np.arange(N_FIRST, dtype=np.int32)
AGAIN = FIRST.copy()
SHIFTED = np.arange(N_FIRST // 2, N_ROWS, dtype=np.int32)
LISTS = {"first": FIRST, "again": AGAIN, "shifted": SHIFTED}
ALL_MISSING_EVERY, REPEAT_EVERY, REPEAT_BACK = 97, 16, 3
N_FAMILIES = 16  # per kind of family (family_of)
STRENGTH = 400.0  # Pitman-Yor strength of the scored slot's class: the new-row candidate is drawn now and then
SEED = 5
N_DRAWS = 5


def _word(rnd, lo, hi, letters=LETTERS):
    return "".join(rnd.choice(letters, size=rnd.integers(lo, hi)))


def _distinct(rnd, n, seen, lo, hi, letters=LETTERS):
    out = []
    while len(out) < n:
        w = _word(rnd, lo, hi, letters)
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def _pool(rnd, clean, taken, lo, hi, letters=LETTERS):
    """POOL strings that are none of `taken`: a quarter of them random, the others an undamaged string with two neighbouring
    letters swapped around an inserted one ("ab" -> "bca": two edits with transpositions of any letters, three when a
    swapped pair may not be edited again), so that the two distance modes give many cells another distance"""
    seen = set(taken)
    out = _distinct(rnd, POOL // 4, seen, lo, hi, letters)
    while len(out) < POOL:
        w = clean[int(rnd.integers(0, len(clean)))]
        p = int(rnd.integers(0, len(w) - 1))
        s = w[:p] + w[p + 1] + str(rnd.choice(letters)) + w[p] + w[p + 2:]
        if s not in seen:
            seen.add(s)
            out.append(s)
    return [out[j] for j in rnd.permutation(POOL)]


def is_all_missing(i):
    return i % ALL_MISSING_EVERY == 11


def is_repeat(i):
    return i % REPEAT_EVERY == 7 and not is_all_missing(i) and not is_all_missing(i - REPEAT_BACK)


def family_of(i, n_cols):
    """(family, its shared columns) of row i, or None.  The rows of a family hold the same strings in the shared columns and
    their own in the others: keys that agree in some words of the stored key and differ in the rest (an entry of the family
    that a lookup passes on its way must not answer it).  Rows 4 mod 8 share all but the last two columns (of up to three
    columns: all but the last), rows 2 mod 8 all but the first two (the first)."""
    if is_all_missing(i) or i % 8 not in (2, 4):
        return None
    cut = n_cols - 2 if n_cols >= 4 else n_cols - 1
    shared = range(cut) if i % 8 == 4 else range(n_cols - cut, n_cols)
    return (i % 8, (i // 8) % N_FAMILIES), shared


def _columns(rnd, n_cols, clean_of_row, pools, families=True):
    """n_cols observed columns of N_ROWS cells (see the module's docstring); clean_of_row[c][i]: the undamaged string"""
    cols = [[] for _ in range(n_cols)]
    shared = {}  # (family, column) -> the family's string there
    for i in range(N_ROWS):
        fam = family_of(i, n_cols) if families else None
        for c in range(n_cols):
            u, pick = rnd.random(), int(rnd.integers(0, POOL))
            if is_all_missing(i):
                cols[c].append(None)
            elif is_repeat(i):
                cols[c].append(cols[c][i - REPEAT_BACK])
            elif fam is not None and c in fam[1]:
                cols[c].append(shared.setdefault((fam[0], c), pools[c][pick]))
            elif u < 0.08:
                cols[c].append(clean_of_row[c][i])
            elif u < 0.12:
                cols[c].append(None)
            else:
                cols[c].append(pools[c][pick])
    return cols


def _finish(S, block, ctx=None):
    """adds what the tests ask of every program: the scored block, its leaf, the candidates and the leaf's key columns"""
    lw = S["lw"]
    arrs = lw.block_arrays(block)
    nodes, terms = arrs[0], arrs[1]
    leaves = [k for k in range(1, len(nodes)) if not nodes[k]["cacheable"]]
    assert len(leaves) == 1 and nodes[0]["n_children"] == 1, "exactly one open option list under the scored slot"
    leaf = leaves[0]
    tsl = slice(int(nodes[leaf]["term_begin"]), int(nodes[leaf]["term_begin"] + nodes[leaf]["n_terms"]))
    info = lw.blocks[block]["node_info"]
    S.update(block=block, leaf=leaf, leaf_terms=tsl, key_cols=sorted(set(int(c) for c in terms[tsl]["obs_col"])),
             slot_class=info[0]["cls"], leaf_attr=(info[leaf]["cls"], info[leaf]["attr"]), ctx=ctx,
             n_options=len(lw.option_values[(info[leaf]["cls"], info[leaf]["attr"])]))
    return S


def keys_of(S, rows, obs=None):
    """the memo key of every item of a list: its observed values in the leaf's columns (+ its ctx value), as tuples"""
    k = (S["obs"] if obs is None else obs)[S["key_cols"]][:, rows].T
    if S["ctx"] is not None:
        k = np.concatenate([k, S["ctx"][rows][:, None]], axis=1)
    return [tuple(int(v) for v in r) for r in k]


def cols(k, tabulated=False):
    rnd = np.random.default_rng(SEED + k + (100 if tabulated else 0))
    words = _distinct(rnd, N_OPTIONS, set(), 4, 9)
    pools = [_pool(rnd, words, words, 5, 6) for _ in range(k)]
    ent = np.arange(N_ROWS) % N_OPTIONS
    clean = [words[e] for e in ent]
    data = _columns(rnd, k, [clean] * k, pools)
    if tabulated:  # y1 ~ FormatName: the name in another case, or its initial, besides the pool strings
        for i in range(N_ROWS):
            if data[0][i] is not None and not is_repeat(i) and i % 5 == 0:
                data[0][i] = clean[i].upper() if i % 10 == 0 else clean[i][0] + "."
        for i in range(N_ROWS):
            if is_repeat(i):
                data[0][i] = data[0][i - REPEAT_BACK]
    m = Model()
    a = m.add_class("A")
    a.choice("x", ChooseUniformly(words))
    a.py_strength = STRENGTH
    o = m.add_class("Obs")
    o.fk("a", "A")
    bind = {}
    for c in range(k):
        o.choice(f"y{c + 1}", FormatName("a.x") if tabulated and c == 0 else AddTypos("a.x"))
        bind[f"Y{c + 1}"] = ("a.x", f"y{c + 1}")
    q = Query(m, "Obs", bind)
    dirty = {f"Y{c + 1}": data[c] for c in range(k)}
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    tr = Trace.from_clean_values(lw, [{"x": clean}], N_ROWS, 0)
    return _finish(dict(name=("tab" if tabulated else f"cols{k}"), lw=lw, obs=obs, trace=tr, words=words, dirty=dirty), 0)


def tab():
    return cols(3, tabulated=True)


def _two_class_model(awords, bwords):
    m = Model()
    a = m.add_class("A")
    a.choice("x", ChooseUniformly(awords))
    a.py_strength = STRENGTH
    b = m.add_class("B")
    b.choice("z", ChooseUniformly(bwords))
    b.py_strength = STRENGTH
    o = m.add_class("Obs")
    return m, o


def join(x, z):
    return f"{x}_{z}"


def ctx2():
    rnd = np.random.default_rng(SEED + 20)
    seen = set()
    awords = _distinct(rnd, N_OPTIONS, seen, 4, 9)
    bwords = _distinct(rnd, N_OPTIONS, seen, 4, 7)
    joined = [join(x, z) for x in awords for z in bwords]
    pools = [_pool(rnd, awords, awords, 5, 6), _pool(rnd, bwords, bwords, 5, 6),
             _pool(rnd, joined, joined, 9, 13, LETTERS + ["_"])]
    enta, entb = np.arange(N_ROWS) % N_OPTIONS, (np.arange(N_ROWS) // N_OPTIONS) % N_OPTIONS
    ca, cb = [awords[e] for e in enta], [bwords[e] for e in entb]
    # (no families: the leaf reads two of the three columns, and its relatives are the repeated tuples with another ctx value)
    data = _columns(rnd, 3, [ca, cb, [join(x, z) for x, z in zip(ca, cb)]], pools, families=False)
    m, o = _two_class_model(awords, bwords)
    with o.block():
        o.fk("a", "A")
        o.choice("y0", AddTypos("a.x"))
    with o.block():
        o.fk("b", "B")
        o.choice("w", AddTypos("b.z"))
        o.julia("j", join, ["a.x", "b.z"])
        o.choice("v", AddTypos("j"))
    q = Query(m, "Obs", {"Y0": ("a.x", "y0"), "W": ("b.z", "w"), "V": ("j", "v")})
    dirty = {"Y0": data[0], "W": data[1], "V": data[2]}
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    tr = Trace.from_clean_values(lw, {0: {"x": ca}, 1: {"z": cb}}, N_ROWS, 0)
    # the ctx value of an item: a value of A.x (an index of its domain).  A repeated tuple keeps the ctx value of its
    # original in every other case (one key twice) and takes another one otherwise (equal observed values, different ctx)
    n_a = len(lw.latent_dom[("A", "x")])
    ctx = rnd.integers(0, n_a, N_ROWS).astype(np.int32)
    for i in range(N_ROWS):
        if is_repeat(i):
            ctx[i] = ctx[i - REPEAT_BACK] if (i // REPEAT_EVERY) % 2 else (ctx[i - REPEAT_BACK] + 1 + i % (n_a - 1)) % n_a
    S = _finish(dict(name="ctx2", lw=lw, obs=obs, trace=tr, words=bwords, dirty=dirty), 1, ctx=ctx)
    assert len(S["key_cols"]) == 2 and len(lw.fn_tables) == 1
    return S


def two():
    """two open leaves under two slots whose tuples coincide as integers"""
    rnd = np.random.default_rng(SEED + 40)
    seen = set()
    words = _distinct(rnd, N_OPTIONS, seen, 4, 9)
    other = _distinct(rnd, N_OPTIONS, seen, 4, 9)  # B's words: other strings, so other marginals under equal keys
    pools = [_pool(rnd, words, words + other, 5, 6) for _ in range(2)]
    ent = np.arange(N_ROWS) % N_OPTIONS
    clean = [words[e] for e in ent]
    data = _columns(rnd, 2, [clean] * 2, pools)
    m, o = _two_class_model(words, other)
    with o.block():
        o.fk("a", "A")
        o.choice("y1", AddTypos("a.x"))
        o.choice("y2", AddTypos("a.x"))
    with o.block():
        o.fk("b", "B")
        o.choice("w1", AddTypos("b.z"))
        o.choice("w2", AddTypos("b.z"))
    q = Query(m, "Obs", {"Y1": ("a.x", "y1"), "Y2": ("a.x", "y2"), "W1": ("b.z", "w1"), "W2": ("b.z", "w2")})
    dirty = {"Y1": data[0], "Y2": data[1], "W1": list(data[0]), "W2": list(data[1])}
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    tr = Trace.from_clean_values(lw, {0: {"x": clean}, 1: {"z": [other[e] for e in ent]}}, N_ROWS, 0)
    S = dict(name="two", lw=lw, obs=obs, trace=tr, dirty=dirty)
    S["views"] = [_finish(dict(S, name=f"two/{b}"), b) for b in (0, 1)]  # the program as each block's tests see it
    assert [v["key_cols"] for v in S["views"]] == [[0, 1], [2, 3]] and S["views"][0]["leaf"] == S["views"][1]["leaf"]
    return S


PROGRAMS = {"cols2": lambda: cols(2), "cols3": lambda: cols(3), "cols6": lambda: cols(6), "cols7": lambda: cols(7),
            "ctx2": ctx2, "tab": tab}
ORACLE_PROGRAMS = ("cols2", "cols3", "cols6", "ctx2")  # (the oracle does not know tab's tabulated term)


# ---- the oracle's side -------------------------------------------------------------------------------------------------
def ctxv(S, rows):
    return None if S["ctx"] is None else S["ctx"][rows][:, None]


def oracle_world(oracle, helpers, S, engine=None, dist_mode=0, option_logp=None):
    if engine is not None:
        return helpers.mirror_world(oracle, S["lw"], S["obs"], S["trace"], engine)
    ol = option_logp if option_logp is not None else helpers.option_logp_cpu(oracle, S["lw"], S["trace"])
    return helpers.mirror_world(oracle, S["lw"], S["obs"], S["trace"], None, dist_mode=dist_mode, option_logp=ol)


def n_cand(S):
    return S["trace"].tables[S["slot_class"]].n + 1


def oracle_leaf(world, S, rows):
    """the leaf's log-marginal of every item"""
    return world.score_node(S["block"], S["leaf"], rows, ctxv=ctxv(S, rows))[0]


def oracle_slot(world, S, rows, snew=None):
    """(lse, scores, draws) of the scored slot; the new-row branch takes the leaf's log-marginals"""
    if snew is None:
        snew = oracle_leaf(world, S, rows)
    return world.score_node(S["block"], 0, rows, ctxv=ctxv(S, rows), snew=snew, seed=1, sweep=2, n_draws=N_DRAWS,
                            n_cand=n_cand(S), want_scores=True)


# ---- the perturbations of the reset tests (each returns what to hand to the device and to the oracle) -------------------
def other_option_logp(S):
    """other log-probabilities for the same option values (normalised, far from uniform)"""
    n = S["n_options"]
    w = 1.0 + np.arange(n, dtype=np.float64) ** 2
    return np.log(w / w.sum())


def other_max_typos(S):
    """the block's term array with max_typos = 1 on the leaf's LAST term (an AddTypos term in every program)"""
    arrs = list(S["lw"].block_arrays(S["block"]))
    terms = arrs[1].copy()
    terms["max_typos"][S["leaf_terms"].stop - 1] = 1
    arrs[1] = terms
    return arrs


def other_fn_table(S):
    """ctx2's fn table with its ctx axis reversed: the same strings under the same id, other contents"""
    (fid, fn), = S["lw"].fn_tables.items()
    return fid, np.ascontiguousarray(fn[::-1])


# ---- the device's side ---------------------------------------------------------------------------------------------------
class Rig:
    """engine + mirrored oracle world of one program (views: the program as each scored block sees it)"""

    def __init__(self, oracle, helpers, S):
        from pclean_amd.engine import Engine
        self.oracle, self.helpers, self.S = oracle, helpers, S
        self.eng = Engine(S["lw"], S["obs"], dist_mode=0)
        self.hip = self.eng.hip
        self.blocks, self.fns = {}, {}  # what the oracle's world is told after a mirror: reloaded blocks, fn tables
        self.obs, self.row_lo = S["obs"], 0
        try:
            self.eng.upload_trace(S["trace"])
            self.mirror()
        except Exception:
            self.eng.close()
            raise

    def close(self):
        self.eng.close()

    def mirror(self):
        """the oracle's world from what the device holds now"""
        S = self.S
        self.world = self.helpers.mirror_world(self.oracle, S["lw"], self.obs, S["trace"], self.eng)
        for bid, arrs in self.blocks.items():
            self.world.load_block(bid, *arrs)
        for fid, fn in self.fns.items():
            self.world.set_fn(fid, fn)

    def device(self, V, rows, snew=None):
        """(lse, scores, draws) of view V's slot for the items `rows` of the active window"""
        g = rows + self.row_lo
        return self.hip.score_node(V["block"], 0, rows, ctxv=ctxv(V, g), snew=snew, seed=1, sweep=2, n_draws=N_DRAWS,
                                   n_cand=n_cand(V), want_scores=True)

    def device_leaf(self, V, rows):
        """the leaf's log-marginals by a direct evaluation of the leaf: this call never goes through the memo"""
        return self.hip.score_node(V["block"], V["leaf"], rows, ctxv=ctxv(V, rows + self.row_lo))[0]

    def want(self, V, rows):
        """the oracle's (lse, scores, draws) for the same items"""
        return oracle_slot(self.world, V, rows + self.row_lo)

    def counted(self, V, rows):
        """device(V, rows) with the counters around it: (result, memo_stats of the call, enumeration launches of the call)"""
        self.hip.memo_stats(reset=True)
        self._launches(reset=True)
        got = self.device(V, rows)
        return got, self.hip.memo_stats(), self._launches()

    def _launches(self, reset=False):
        """launches of the generic enumeration and of the compact-table kernels (an option list may take either)"""
        return sum(self.hip.enum_launches(reset=reset).values()) + sum(self.hip.root_launches(reset=reset).values())

    def slot_alone_launches(self, V, rows):
        """what the slot launches when its new-row branch is handed in: the launches of a call besides the leaf's"""
        self._launches(reset=True)
        self.device(V, rows, snew=np.zeros(len(rows)))
        return self._launches()


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: lse differs in {int((got[0] != want[0]).sum())} of {len(want[0])} items"
    assert np.array_equal(got[1][:, -1], want[1][:, -1]), f"{what}: the new-row candidate's score differs"
    assert np.array_equal(got[1], want[1]), f"{what}: candidate scores differ"
    assert np.array_equal(got[2], want[2]), f"{what}: draws differ"


def expected_misses(V, rows, earlier):
    """items of `rows` whose key is in none of the earlier lists"""
    seen = set()
    for e in earlier:
        seen |= set(keys_of(V, e))
    return sum(k not in seen for k in keys_of(V, rows))
