"""Programs for the tests that pin every path of the compact-table root launch (pclean_launch_root_fast, root_wave.hip)
to the oracle — tests/test_root_variants_cpu.py and tests/test_gpu_root_variants.py — and the CPU model that says which
path every row's group must take.

The program: class Ent with T string attributes f0 .. f{T-1} (the first `n_long` of them strings of 34-40 letters under
StringPrior, the others of 3-5 letters under ChooseUniformly), class Obs with one reference slot and T AddTypos observations.  prefilter_terms
(eval.hip) takes the three terms with the longest latent strings, in a stable order: the long attributes, then the first
short ones — PRE below; the first attribute that is not a pre-filter term is NONPRE (none up to three terms).  Unrelated
entities are random strings: their summed pre-filter distance is far above any non-refine cut-off.  Typos in an
OBSERVED cell are digits (no latent string holds one), so k of them are exactly k edits.

Row kinds (S["kind"]), each a small family of entities and the rows that observe them:

  filler     random entities (shape "blocks": copies of 300 of them) observed exactly, by two identical rows (one group) or, every fifth, by a single row: the
             referent of a single reference is garbage-collected when the row leaves it (descriptor flag bit 0)
  peaked     the referent's values with 0, 1 and 2 typos: one survivor, the current referent (the descriptor-scored path)
  few(j)     j entities identical on the pre-filter attributes, different on NONPRE; j on both sides of SPP = 64 / NTP of
             the instantiation: by-term scoring against one candidate per lane
  cap(j)     the same with j in {255, 256, 257, 300}: the survivor cap, the overflow flag and overflow_lds_kernel; the
             members have 2 or 4 references, so the posterior is flat but not uniform
  slack      200 entities at distance 0 and 64 at summed distance want+1 .. want+3 (want: the cut-off the rows' bound
             requires, from the CPU model): the list overflows with WAVE_SLACK and fits without
  refine     rows without a referent (cur = -1) that observe an entity exactly (refine_none) or 21 edits away
             (refine_wide: nothing within the first two cut-offs), rows whose referent is another entity (refine_bad)
  new        rows that observe the values of a deleted entity (the option lists of the new-row branch hold them, no
             candidate does; its long values are likely strings under the string prior): the new-row candidate wins
  missing    one, two or all of the pre-filter cells missing (the zero row); a missing cell elsewhere
  far        NONPRE observed as a 48-letter string (more than PRE_CLAMP = 42 edits from a 3-5 letter value) while the
             pre-filter cells match, for a referent with a twin and for one with SPP twins: saturated bytes in both
             scoring schemes.  From five terms on; with four terms two of the three pre-filter terms are short strings, the
             cut-off such a row requires lets every candidate through and the rows overflow (generated, not asserted on)
  twin       100 identical rows of one referent (a group that is cut into pieces with identical descriptors), and rows of a
             second entity with the same pre-filter values (the cached list)
  block_a/b  (shape "blocks") 136 near candidates one per 64-candidate block — more than WAVE_BLK_CAP = 128 passing
             blocks, the rows are streamed whole — and 100 near candidates over 100 blocks
  dense      (shape "dense") every entity is a copy of one of 16 bases, every block holds every base: three blocks in four
             pass for every group (dense_skip)

Every family has one dead member (deleted below the high-water mark), and a few fillers are dead: the alive mask.

expected_paths() restates group_desc_kernel's bound and cut-off (c_min over the (L, d) range of the tables, inv_c,
cut_max, the refine decision), the summed saturated bytes of the pre-filter terms, the two-level scan's passing blocks and
group_settle_kernel's condition in NumPy; the candidate scores come from the oracle."""
import numpy as np

from pclean_amd.model import AddTypos, ChooseUniformly, LoweredModel, Model, Query, StringPrior
from pclean_amd.trace import Trace

# restated from root_wave.hip (the GPU test's counters and flags say whether the library still agrees)
PRE_CLAMP, CUT_ALL, FIX_CUTOFF = 42, 126, 28.5
CAP, BLK_CAP, DCUT_OK, GUESS, SLACK = 256, 128, 24, 4, 3
SETTLE_MAX_BLOCKS, SETTLE_MIN_GROUPS = 4, 4096
MIN_CAND = 1024          # try_fast_root: the table size from which a reference slot takes the compact tables

SEED = 5
N_DRAWS = 7              # (= enum_variants_program.N_DRAWS)
ALPHA = np.array(list("abcdefghijklmnopqrstuvwxyz"))
LONG, SHORT = (34, 40), (3, 5)
STRENGTH_DIV = 16        # Pitman-Yor strength n_ent / 16: the new-row candidate can be drawn


def likely_string(k, n):
    """n letters that are cheap under StringPrior's bigram model: the k-th likeliest first letter, then the likeliest next
    letter that has not been used twice in a row"""
    from pclean_amd.encode import load_lm_params
    init, trans = load_lm_params()
    out = [int(np.argsort(-init[:26])[k])]
    while len(out) < n:
        nxt = np.argsort(-trans[out[-1]][:26])
        out.append(int(next(c for c in nxt if not (len(out) >= 2 and out[-1] == c and out[-2] == c))))
    return "".join(ALPHA[c] for c in out)


def variant(n_terms):
    """term capacity of the fk_root_wave_kernel instantiation pick_kernel() takes"""
    return 2 if n_terms <= 2 else 4 if n_terms <= 4 else 8 if n_terms <= 8 else 12 if n_terms <= 12 else 16


def spp(n_terms):
    """survivors per pass of the by-term scoring: lists of up to SPP entries take it (64 / NTP)"""
    nt = variant(n_terms)
    return 64 // (2 if nt <= 2 else 4 if nt <= 4 else 8 if nt <= 8 else 16)


class _Builder:
    def __init__(self, n_terms, n_long, rng):
        self.T, self.n_long, self.rng = n_terms, n_long, rng
        n_pre = min(3, n_terms)
        self.pre = list(range(n_long)) + list(range(n_long, n_terms))[:max(0, n_pre - n_long)]
        self.pre = self.pre[:n_pre]
        self.nonpre = next((f for f in range(n_terms) if f not in self.pre), None)
        self.ents, self.rows = [], []  # ents: dict(vals, dead, pin); rows: (kind, entity handle | -1, observed tuple)

    def rand(self, f, lo=None, hi=None):
        lo_, hi_ = LONG if f < self.n_long else SHORT
        n = int(self.rng.integers(lo or lo_, (hi or hi_) + 1))
        return "".join(self.rng.choice(ALPHA, n))

    def entity(self):
        return [self.rand(f) for f in range(self.T)]

    def add(self, vals, dead=False, pin=None):
        self.ents.append(dict(vals=list(vals), dead=dead, pin=pin))
        return len(self.ents) - 1

    def row(self, kind, h, obs, times=1):
        self.rows += [(kind, h, tuple(obs))] * times

    def typos(self, s, k):
        """s with k letters replaced by digits: exactly k edits from s"""
        pos = self.rng.choice(len(s), size=k, replace=False)
        s = list(s)
        for i, p in enumerate(pos):
            s[p] = "0123456789"[i % 10]
        return "".join(s)

    def pre_typos(self, vals, k):
        """k typos spread over the long pre-filter cells"""
        out = list(vals)
        longs = [f for f in self.pre if f < self.n_long]
        for i, f in enumerate(longs):
            kf = k // len(longs) + (1 if i < k % len(longs) else 0)
            out[f] = self.typos(out[f], kf)
        return out

    def letter_subst(self, vals, k):
        """k letters of the long pre-filter cells replaced by other letters, four (or two) positions apart (a latent value)"""
        out = list(vals)
        longs = [f for f in self.pre if f < self.n_long]
        for i, f in enumerate(longs):
            kf = k // len(longs) + (1 if i < k % len(longs) else 0)
            s = list(out[f])
            step = 4 if kf <= len(s) // 4 else 2
            for p in (self.rng.permutation(len(s) // step)[:kf] * step + int(self.rng.integers(0, step))) % len(s):
                s[p] = ALPHA[(np.flatnonzero(ALPHA == s[p])[0] + 1 + int(self.rng.integers(0, 24))) % 26]
            out[f] = "".join(s)
        return out

    def family(self, j, pin=None):
        """j entities identical on the pre-filter attributes (and everywhere, up to three terms), NONPRE varied over four
        values one edit apart; one dead member in the middle.  Returns the handles of the live ones."""
        base = self.entity()
        hs = []
        for i in range(j + 1):
            v = list(base)
            if self.nonpre is not None:
                v[self.nonpre] = base[self.nonpre][:-1] + "wxyz"[i % 4]
            dead = i == j // 2
            h = self.add(v, dead=dead, pin=None if pin is None else pin[i])
            if not dead:
                hs.append(h)
        return base, hs

    def observe(self, h, **kw):
        """the values of entity h; kw: missing=[attributes], typo={attribute: k}"""
        obs = list(self.ents[h]["vals"])
        for f, k in kw.get("typo", {}).items():
            obs[f] = self.typos(obs[f], k)
        for f in kw.get("missing", ()):
            obs[f] = None
        return obs

    def flat_family(self, kind, j, pin=None):
        """family(j) with 2 or 4 references per member: exact rows (NONPRE own value, then missing), then one typo"""
        base, hs = self.family(j, pin)
        np_ = [] if self.nonpre is None else [self.nonpre]
        for i, h in enumerate(hs):
            self.row(kind, h, self.observe(h))
            self.row(kind, h, self.observe(h, missing=np_))
            if i % 3 == 0:
                self.row(kind, h, self.observe(h, typo={self.pre[0]: 1}))
                self.row(kind, h, self.observe(h, typo={self.pre[0]: 1}, missing=np_))
        return base, hs


def program(n_terms, n_long, kinds, n_ent=1100, seed=SEED, shape="std", slack_want=None, peaked=12, peaked_rows=3):
    """dict(lw, obs, trace, kind, dirty, pre, nonpre, n_terms): see the module docstring.  kinds: the row kinds to include
    besides filler and peaked; slack_want: the cut-off of the slack rows (None: the 64 near entities are left unrelated —
    the first pass of build(), which asks the CPU model for it)."""
    rng = np.random.default_rng(seed)
    B = _Builder(n_terms, n_long, rng)
    T, pre, nonpre, S_ = n_terms, B.pre, B.nonpre, spp(n_terms)
    for _ in range(peaked):
        h = B.add(B.entity())
        for r in range(peaked_rows):  # 0, 1, 2 typos: distinct tuples
            if r < 3 and peaked_rows <= 3:
                B.row("peaked", h, B.observe(h, typo={pre[0]: r} if r else {}))
            else:  # (many groups without many strings: exact, then one pre-filter cell missing)
                B.row("peaked", h, B.observe(h, missing=[pre[r - 1]] if r else []))
    if "few" in kinds:
        for j in (S_, S_ + 1):
            B.flat_family(f"few{j}", j)
    if "cap" in kinds:
        for j in (255, 256, 257, 300):
            B.flat_family(f"cap{j}", j)
    if "slack" in kinds:
        base, hs = B.family(200)
        for h in hs:
            B.row("slack", h, B.observe(h), times=2)
        for i in range(64):
            v = B.entity() if slack_want is None else B.letter_subst(base, slack_want + 1 + i % 3)
            if slack_want is not None and nonpre is not None:
                v[nonpre] = base[nonpre][:-1] + "wxyz"[i % 4]
            h = B.add(v)
            B.row("slack_near", h, B.observe(h), times=2)
    if "refine" in kinds:
        for i in range(4):
            h = B.add(B.entity())
            B.row("peaked", h, B.observe(h), times=2)
            B.row("refine_none", -1, B.observe(h))
            B.row("refine_wide", -1, B.pre_typos(B.ents[h]["vals"], 21))
            h2 = B.add(B.entity())
            B.row("peaked", h2, B.observe(h2), times=2)
            B.row("refine_bad", h2, B.observe(h))
    if "new" in kinds:
        h = B.add(B.entity())
        B.row("peaked", h, B.observe(h), times=2)
        # a deleted entity: the option lists still hold its values, no candidate does.  Its long values follow the string
        # prior's likeliest letters, so the new row (three string priors) beats every candidate (three unrelated cells)
        gone = B.add([likely_string(f, 36) if f < n_long else B.rand(f) for f in range(T)], dead=True)
        for i in range(6):
            B.row("new", -1 if i % 2 else h, B.observe(gone, typo={pre[0]: 1} if i >= 4 else {}))
    if "missing" in kinds:
        for _ in range(2):
            h = B.add(B.entity())
            B.row("peaked", h, B.observe(h), times=2)
            for p in range(len(pre)):
                B.row("missing", h, B.observe(h, missing=pre[:p + 1]))
                B.row("missing", h, B.observe(h, missing=[pre[p]], typo={pre[(p + 1) % len(pre)]: 1} if len(pre) > 1 else {}))
            if nonpre is not None:
                B.row("missing", h, B.observe(h, missing=[nonpre]))
    if "far" in kinds and nonpre is not None:
        for j in (2, S_ + 1):
            base = B.entity()
            for i in range(j):
                h = B.add(base)
                B.row("far_base", h, B.observe(h), times=2)
                if i < 2:
                    obs = B.observe(h)
                    obs[nonpre] = B.rand(nonpre, 48, 48)
                    B.row(f"far{j}", h, obs)
    if "twin" in kinds:
        v = B.entity()
        h = B.add(v)
        B.row("twin", h, B.observe(h), times=100)
        v2 = list(v)
        if nonpre is not None:
            v2[nonpre] = B.rand(nonpre)
        h2 = B.add(v2)
        B.row("twin", h2, B.observe(h2), times=2)
        B.row("twin", h2, B.observe(h2, typo={pre[0]: 1}))
        B.row("twin", h, B.observe(h2))
    if shape == "blocks":
        B.flat_family("block_a", 136, pin=[64 * b + 5 for b in range(137)])
        B.flat_family("block_b", 100, pin=[64 * (b + 20) + 9 for b in range(101)])
    if shape == "dense":
        bases = [B.entity() for _ in range(16)]
        for i in range(n_ent - len(B.ents)):
            h = B.add(bases[i % 16], dead=(i % 97 == 50))
            if not B.ents[h]["dead"]:
                B.row("dense", h, B.observe(h, typo={pre[0]: i % 3} if i % 3 else {}), times=2)
    # fillers up to n_ent entities, the padded size no multiple of 64 (a partial last block), some of them dead
    n_ent = max(n_ent, len(B.ents) + 40, MIN_CAND)
    while ((n_ent + 15) & ~15) % 64 == 0:
        n_ent += 16
    pool = [B.entity() for _ in range(300)] if shape == "blocks" else None  # (few distinct strings: small pair tables)
    for i in range(n_ent - len(B.ents)):
        dead = i % 23 == 7
        h = B.add(pool[i % 300] if pool else B.entity(), dead=dead)
        if not dead:
            B.row("filler", h, B.observe(h), times=1 if i % 5 == 0 else 2)
    # table order: the pinned entities at their places, the others shuffled over the rest
    place = np.full(n_ent, -1, dtype=np.int64)
    for h, e in enumerate(B.ents):
        if e["pin"] is not None:
            assert place[e["pin"]] < 0
            place[e["pin"]] = h
    free = np.flatnonzero(place < 0)
    loose = [h for h, e in enumerate(B.ents) if e["pin"] is None]
    place[free] = loose if shape == "dense" else rng.permutation(loose)  # (dense: every block holds every base)
    at = np.empty(n_ent, dtype=np.int64)
    at[place] = np.arange(n_ent)
    ents = [B.ents[h] for h in place]
    rows = [(k, -1 if h < 0 else int(at[h]), o) for k, h, o in B.rows]
    order = rng.permutation(len(rows))  # (the library sorts the rows into groups itself)
    rows = [rows[i] for i in order]
    return _lower(n_terms, ents, rows, dict(pre=pre, nonpre=nonpre, n_terms=n_terms, n_long=n_long), n_ent / STRENGTH_DIV, seed)


def _lower(n_terms, ents, rows, extra, strength, seed):
    fields = [f"f{f}" for f in range(n_terms)]
    dirty = {fn.upper(): [r[2][f] for r in rows] for f, fn in enumerate(fields)}
    m = Model()
    c = m.add_class("Ent")
    for f, fn in enumerate(fields):
        atoms = list(dict.fromkeys(e["vals"][f] for e in ents))
        # (the short attributes are option lists without a ProposalDummyValue: a block takes at most 8 lists that bear one, and
        # the dummy of a list of 3-5 letter strings can be drawn for every row, which makes every row's draws eager — no lazy lists)
        c.choice(fn, StringPrior(*LONG, atoms) if f < extra["n_long"] else ChooseUniformly(atoms))
    c.py_strength = float(strength)
    o = m.add_class("Obs")
    with o.block():
        o.fk("ent", "Ent")
        for fn in fields:
            o.choice(fn, AddTypos("ent." + fn))
    q = Query(m, "Obs", {fn.upper(): ("ent." + fn, fn) for fn in fields})
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    n = len(rows)
    tr = Trace(lw, n, seed)
    t = tr.tables["Ent"]
    doms = [lw.latent_dom[("Ent", fn)] for fn in fields]
    col = lw.colidx["Ent"]
    vals = np.empty((len(ents), len(fields)), dtype=np.int32)
    for f, fn in enumerate(fields):
        vals[:, col[fn]] = [doms[f].index_of(e["vals"][f]) for e in ents]
    ids = tr.insert_rows_bulk("Ent", vals)
    assert np.array_equal(ids, np.arange(len(ents)))
    cur = np.array([r[1] for r in rows], dtype=np.int64)
    tr.cur[0] = cur
    t.counts[:t.n] += np.bincount(cur[cur >= 0], minlength=t.n)
    dead = [k for k, e in enumerate(ents) if e["dead"]]
    assert not t.counts[dead].any()
    for k in dead:
        tr.delete_row("Ent", k)
    return dict(lw=lw, obs=obs, trace=tr, dirty=dirty, kind=np.array([r[0] for r in rows]), **extra)


def leaf_program(n_options=1100, n_rows=1200, seed=SEED):
    """An option list as the root launch takes it (is_leaf): `A: x ~ ChooseUniformly(words)` with n_options words of
    16-24 letters, `Obs: a ~ A; y, y2, y3 ~ AddTypos(a.x)` — three terms, so the list is not served from the per-value
    cache.  Clusters of words a few edits apart keep the posteriors flat; rows observe a word exactly, with typos in one or
    all cells, with cells missing, or a string no option is near."""
    rng = np.random.default_rng(seed)
    words, seen = [], set()
    while len(words) < n_options:
        base = "".join(rng.choice(ALPHA, int(rng.integers(16, 25))))
        for k in range(int(rng.integers(1, 9))):
            w = list(base)
            for p in rng.choice(len(w), size=min(k, 3), replace=False):
                w[p] = ALPHA[int(rng.integers(0, 26))]
            w = "".join(w)
            if w not in seen and len(words) < n_options:
                seen.add(w)
                words.append(w)
    words = [words[i] for i in rng.permutation(n_options)]
    n_lat = 64
    ent = np.arange(n_rows) % n_lat
    ys, kind = [], []

    def typo(s, k):
        s = list(s)
        for i, p in enumerate(rng.choice(len(s), size=k, replace=False)):
            s[p] = "0123456789"[i % 10]
        return "".join(s)

    for i in range(n_rows):
        w = words[int(rng.integers(0, n_options))]
        k = i % 8
        if k == 0:
            ys.append((w, w, w)), kind.append("exact")
        elif k in (1, 2):
            ys.append((typo(w, k), w, None)), kind.append("typo")
        elif k == 3:
            ys.append((typo(w, 2), typo(w, 3), typo(w, 2))), kind.append("typos")
        elif k == 4:
            ys.append((None, w, None)), kind.append("one_cell")
        elif k == 5:
            ys.append((None, None, None)), kind.append("flat")
        elif k == 6:
            ys.append(("".join(rng.choice(ALPHA, 20)),) * 3), kind.append("none_near")
        else:
            ys.append((None, None, None) if i % 16 == 7 else (None, typo(w, 6), None)), kind.append("flat")
    dirty = {"Y": [y[0] for y in ys], "Y2": [y[1] for y in ys], "Y3": [y[2] for y in ys]}
    m = Model()
    a = m.add_class("A")
    a.choice("x", ChooseUniformly(words))
    o = m.add_class("Obs")
    with o.block():
        o.fk("a", "A")
        o.choice("y", AddTypos("a.x"))
        o.choice("y2", AddTypos("a.x"))
        o.choice("y3", AddTypos("a.x"))
    q = Query(m, "Obs", {"Y": ("a.x", "y"), "Y2": ("a.x", "y2"), "Y3": ("a.x", "y3")})
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    tr = Trace.from_clean_values(lw, [{"x": [words[e] for e in ent]}], n_rows, 0)
    return dict(lw=lw, obs=obs, trace=tr, dirty=dirty, kind=np.array(kind), words=words, n_terms=3)


# ---- the shapes (shared by the CPU and the GPU tests) ----------------------------------------------------------------
ALL = ("few", "cap", "slack", "refine", "new", "missing", "far", "twin")
# name: (terms, long attributes, kinds, program arguments)
SHAPES = {
    "t1": (1, 1, ALL, {}),
    "t2": (2, 2, ALL, {}),
    "t3": (3, 3, ALL, {}),
    "t4": (4, 1, ALL, {}),
    "t5": (5, 3, ALL, {}),
    "t8": (8, 3, ALL, {}),
    "t9": (9, 3, ALL, {}),
    "t12": (12, 3, ALL, {}),
    "t13": (13, 3, ALL, {}),
    "t16": (16, 3, ALL, {}),
    "blocks": (3, 3, ("refine", "new"), dict(shape="blocks", n_ent=8800)),
    "dense": (3, 3, ("new",), dict(shape="dense", n_ent=1100)),
    "groups": (3, 3, ("few", "refine", "new"), dict(n_ent=1100, peaked=1040, peaked_rows=4)),
}
SPARE = ("t3", "blocks", "groups")  # shapes the GPU test also sweeps on a table uploaded with spare capacity (kscan < kpad)
N_PRE = {"t1": 1, "t2": 2}  # (every other shape: 3)
_cache = {}


def build(name, oracle=None, helpers=None):
    """the program of shape `name` (cached: the tests share it and leave it unchanged).  A shape with slack rows is
    generated twice: the first pass asks the CPU model for the cut-off those rows' bound requires."""
    if name in _cache:
        return _cache[name]
    T, n_long, kinds, kw = SHAPES[name]
    S = program(T, n_long, kinds, **kw)
    if "slack" in kinds:
        rows = np.flatnonzero(S["kind"] == "slack")
        want = np.unique(expected_paths(S, oracle, helpers, rows=rows)["want"])
        assert len(want) == 1, want
        S = program(T, n_long, kinds, slack_want=int(want[0]), **kw)
        S["slack_want"] = int(want[0])
    _cache[name] = S
    return S


# ---- the CPU model of the ladder ------------------------------------------------------------------------------------
def oracle_world(oracle, helpers, S, engine=None):
    if engine is not None:
        return helpers.mirror_world(oracle, S["lw"], S["obs"], S["trace"], engine)
    ol = helpers.option_logp_cpu(oracle, S["lw"], S["trace"])
    return helpers.mirror_world(oracle, S["lw"], S["obs"], S["trace"], None, dist_mode=0, option_logp=ol)


def oracle_root(world, S, rows, excl, n_draws=N_DRAWS, want_scores=False, seed=1, sweep=2):
    """(lse, scores, draws) of the reference slot for `rows`; the oracle's score_node takes the new-row branch's marginal
    (the log-marginals of Ent's option lists, summed in plan order) as an input where the device evaluates the sub-tree"""
    blk = S["lw"].blocks[0]
    node = blk["nodes"][0]
    snew = np.zeros(len(rows))
    for c in blk["children"][node[4]:node[4] + node[5]]:
        snew = snew + world.score_node(0, c, rows)[0]
    return world.score_node(0, 0, rows, excl=excl, snew=snew, seed=seed, sweep=sweep, n_draws=n_draws,
                            n_cand=S["trace"].tables[blk["root_class"]].n + 1, want_scores=want_scores)


def root_terms(S, node_id=0):
    """(observed column, candidate column, pair id) of the node's terms, in plan order"""
    blk = S["lw"].blocks[0]
    node = blk["nodes"][node_id]
    return [(t[0], t[1], t[2]) for t in blk["terms"][node[2]:node[2] + node[3]]]


def _pair_tables(S, oracle, terms):
    lw = S["lw"]
    sym, off, _, _ = lw.pool.arrays()
    by_id = {pid: (odom, ldom) for pid, odom, ldom in lw.pair_id.values()}
    out = {}
    for _, _, pid in terms:
        if pid not in out:
            odom, ldom = by_id[pid]
            d = oracle.pair_table(sym, off, odom.id_array(), ldom.id_array(), 0)
            out[pid] = (d, lw.pool.lens[ldom.id_array()], lw.pool.lens[odom.id_array()])
    return out


def c_min(tables, lmax, dmax):
    """try_fast_root's smallest density cost of one edit over the lengths and distances the node's pair tables hold"""
    mr, md, ml, nb, logl = tables
    L = np.arange(1, lmax + 1)[:, None]
    d = np.arange(1, dmax + 1)[None, :]
    l = nb[(L + 4) // 5, d]          # the three fp64 operations of add_typos.jl:61-63, in the kernels' order
    l = l - logl[L] * d
    l = l - 1.629048269010741 * d
    v = -l / d
    return float(np.min(v[~np.isnan(l)]))


def prefilter_terms(pairs, terms):
    """prefilter_terms() of eval.hip: plain terms, longest latent strings first, stable; at most three"""
    order = sorted(range(len(terms)), key=lambda i: -int(pairs[terms[i][2]][1].max()))
    return order[:min(3, len(terms))]


def _cut_of(x):
    """the cut-off group_desc_kernel / the refine step derive from x = (pmax - bound + FIX_CUTOFF) * inv_c"""
    return int(x) + 2 if 0.0 <= x < CUT_ALL - 2 else CUT_ALL


def expected_paths(S, oracle, helpers, rows=None, tables=None, world=None, node_id=0):
    """Per row of `rows` (default: all), as arrays: refine, widen (widenings of a wave that finds no list to reuse), want
    (the cut-off the descriptor holds: the required one, or the upper limit in refine mode), n_surv_slack / n_surv
    (survivors at the last scanned cut-off with WAVE_SLACK and without), overflow, certain (the overflow flag does not
    depend on which wave reused which list), scheme ("desc" the descriptor's score of the sole survivor, "by_term",
    "per_lane"), n_pass_blocks (at the last scanned cut-off with the slack), dense (three blocks in four pass at every
    cut-off scanned), settle (group_settle_kernel's condition), deleted; and n_pre, pre, kblk, kpad.
    tables: the density tables (default: computed on the CPU; the GPU test passes the device's)."""
    lw, tr, obs = S["lw"], S["trace"], S["obs"]
    blk = lw.blocks[0]
    leaf = blk["nodes"][node_id][0] == 1
    world = world or oracle_world(oracle, helpers, S)
    rows = np.arange(obs.shape[1], dtype=np.int32) if rows is None else np.asarray(rows, dtype=np.int32)
    terms = root_terms(S, node_id)
    pairs = _pair_tables(S, oracle, terms)
    pre = prefilter_terms(pairs, terms)
    lmax = max(int(pairs[p][1].max()) for _, _, p in terms)
    dmax = max(max(int(pairs[p][1].max()), int(pairs[p][2].max())) for _, _, p in terms)
    tables = tables or helpers.density_tables_cpu(oracle, int(lw.pool.lens.max()))
    inv_c = 1.0 / (c_min(tables, lmax, dmax) * (1.0 - 1e-9))
    if leaf:
        info = blk["node_info"][node_id]
        n_cand = len(lw.latent_dom[(info["cls"], info["attr"])])
        logp = helpers.option_logp_cpu(oracle, lw, tr)[(info["cls"], info["attr"])]
        alive = np.isfinite(logp)
        cols = np.stack([lw.option_values[(info["cls"], info["attr"])]])
        cur = np.full(len(rows), -1)
        counts = None
        lse, scores, _ = world.score_node(0, node_id, rows, n_cand=n_cand, want_scores=True)
        pmax_e = pmax_n = float(logp.max())
        sn = np.full(len(rows), -np.inf)
    else:
        t = tr.tables[blk["root_class"]]
        cols, counts = t.view()
        n_cand = t.n
        alive = counts > 0
        cur = tr.cur[0, rows]
        lse, scores, _ = oracle_root(world, S, rows, cur, n_draws=0, want_scores=True)
        full, m1, scal = oracle.table_priors(counts, t.strength, t.discount)
        pmax_e, pmax_n = float(full.max() - scal[1]), float(full.max() - scal[0])
        sn = scores[:, n_cand]
    kpad = (n_cand + 15) & ~15
    kblk = (kpad + 63) >> 6
    n = len(rows)
    out = dict(refine=np.zeros(n, bool), widen=np.zeros(n, np.int32), want=np.zeros(n, np.int32),
               n_surv_slack=np.zeros(n, np.int32), n_surv=np.zeros(n, np.int32), overflow=np.zeros(n, bool),
               certain=np.zeros(n, bool), scheme=np.empty(n, dtype=object), n_pass_blocks=np.zeros(n, np.int32),
               dense=np.zeros(n, bool), settle=np.zeros(n, bool), deleted=np.zeros(n, bool), lse=lse,
               n_pre=len(pre), pre=pre, kblk=kblk, kpad=kpad, n_cand=n_cand)
    S_ = spp(len(terms))
    blk_of = np.arange(n_cand) >> 6
    for i, row in enumerate(rows):
        # summed saturated bytes of the pre-filter terms (a missing observation reads the zero row)
        D = np.zeros(n_cand, dtype=np.int64)
        bmin = np.zeros(kblk, dtype=np.int64)
        for p in pre:
            oc, cc, pid = terms[p]
            o = obs[oc, row]
            if o >= 0:
                b = np.minimum(pairs[pid][0][o, cols[cc, :n_cand]], PRE_CLAMP).astype(np.int64)
                D += b
                m = np.full(kblk * 64, 255, dtype=np.int64)
                m[:n_cand] = b
                m[n_cand:kpad] = 0       # padding bytes are 0 (compact_pair_kernel), padding blocks 255
                bmin += m.reshape(kblk, 64).min(axis=1)
        Da = np.where(alive, D, 1 << 20)
        sc = scores[i, :n_cand]
        e = int(cur[i])
        deleted = e >= 0 and counts is not None and counts[e] <= 1
        have_cur = e >= 0 and not deleted and not leaf
        bound = max(sc[e] - 1.0, sn[i]) if have_cur else sn[i]
        pmax = pmax_e if e >= 0 else pmax_n
        cut_max = _cut_of((pmax - bound + FIX_CUTOFF) * inv_c) if bound > -np.inf else CUT_ALL
        refine = cut_max >= DCUT_OK
        out["refine"][i], out["want"][i], out["deleted"][i] = refine, cut_max, deleted

        def ns(c):
            return int((Da <= c).sum())

        def nb(c):
            return int((bmin <= c).sum())
        scanned = []   # the cut-offs a wave that reuses no list scans, the slack included
        state = dict(want=0)

        def scan(cut):
            """the scan at cut-off `cut`: with WAVE_SLACK, and once more without when the slack alone overflowed the list"""
            cs = min(cut + SLACK, CUT_ALL)
            scanned.append(cs)
            if ns(cs) > CAP and cs > cut:
                cs = cut
                scanned.append(cs)
            state["want"] = cut
            return cs
        over = False
        if not refine:
            cs = scan(cut_max)
            over = ns(cs) > CAP
            certain = True
        else:
            cut, widen = GUESS, 0
            while True:
                cut = cs = scan(cut)
                if ns(cs) > CAP:
                    over = True
                    break
                if ns(cs) == 0:
                    if cut >= cut_max:
                        break
                    cut = min(2 * cut + 2, cut_max)
                    widen += 1
                    continue
                best = max(bound, float(sc[Da <= cs].max()))
                need = min(_cut_of((pmax - best + FIX_CUTOFF) * inv_c), cut_max)
                if need > cut:
                    cs = scan(need)
                    over = ns(cs) > CAP
                break
            out["widen"][i] = widen
            # Is the flag the same whichever list a wave reuses?  Every list a wave can hold is S(c) for some cut-off c; a
            # non-empty one holds the candidates at the smallest distance Dmin, so the best score a wave sees lies between
            # the best at Dmin (or the bound) and the best of all, and the cut-off it then requires between need_lo and
            # need_hi.  It ends with a list that covers its requirement: overflow whenever S(need_lo) has more than CAP
            # entries; none whenever the widest cut-off a wave scans itself — below 2 Dmin + 6 in the widening series, or
            # need_hi — keeps within CAP.
            live_sc = np.where(alive, sc, -np.inf)
            dmin = int(Da.min())
            best_all = max(bound, float(live_sc.max()))
            at_min = max(bound, float(live_sc[Da == dmin].max())) if dmin <= CUT_ALL else bound
            need_lo = max(min(_cut_of((pmax - best_all + FIX_CUTOFF) * inv_c), cut_max), GUESS)
            need_hi = max(min(_cut_of((pmax - at_min + FIX_CUTOFF) * inv_c), cut_max), GUESS)
            certain = ns(need_lo) > CAP or ns(max(min(2 * dmin + 6, cut_max), need_hi)) <= CAP
        last = scanned[-1]
        out["overflow"][i], out["certain"][i] = over, certain
        out["n_surv"][i] = ns(state["want"])
        out["n_surv_slack"][i] = ns(min(state["want"] + SLACK, CUT_ALL))
        n_last = ns(last)
        sole = n_last == 1 and have_cur and Da[e] <= last
        out["scheme"][i] = "over" if over else "none" if n_last == 0 else "desc" if sole else "by_term" if n_last <= S_ else "per_lane"
        out["n_pass_blocks"][i] = nb(last)
        out["dense"][i] = kblk >= 8 and all(nb(c) * 4 >= kblk * 3 for c in scanned)
        if have_cur and not refine and len(pre) >= 1:
            hi, lo = max(sc[e], sn[i]), min(sc[e], sn[i])
            if sc[e] != sn[i] and not (lo - hi >= -28.5):
                passing = np.flatnonzero(bmin <= cut_max)
                within = np.flatnonzero(Da <= cut_max)
                out["settle"][i] = (len(passing) <= SETTLE_MAX_BLOCKS and len(within) == 1 and within[0] == e
                                    and blk_of[e] in passing)
    return out


def diversity(draws):
    """distinct values per row of draws [n][k]"""
    s = np.sort(draws, axis=1)
    return 1 + (s[:, 1:] != s[:, :-1]).sum(axis=1)


# ---- what both tests assert of a shape --------------------------------------------------------------------------------
def sample_rows(S, k=200):
    """every row — but of the peaked rows of shape "groups" and the filler rows of shape "blocks" (more than 2 000 rows
    of one kind, none of which overflows) k seeded ones: the oracle scores each distinct row once, a cap on its share of
    the test's time, not a tolerance"""
    kind = S["kind"]
    keep = np.ones(len(kind), dtype=bool)
    for big in ("peaked", "filler"):
        at = np.flatnonzero(kind == big)
        if len(at) > 2000:
            keep[at] = False
            keep[np.random.default_rng(SEED).choice(at, size=k, replace=False)] = True
    return np.flatnonzero(keep).astype(np.int32)


def check_paths(name, S, E, kind):
    """the assertions on the model's output: the CPU test runs them on the oracle's tables, the GPU test on the device's"""
    T = S["n_terms"]
    assert E["n_pre"] == N_PRE.get(name, 3) and [int(p) for p in E["pre"]] == list(S["pre"])
    assert E["n_cand"] >= MIN_CAND and E["kpad"] % 64 != 0
    assert E["certain"].all(), f"{name}: rows whose overflow flag depends on the grid: {sorted(set(kind[~E['certain']]))}"
    kinds = set(kind)

    def rows(k):
        assert k in kinds, f"{name}: no {k} rows"
        return kind == k
    pk = rows("peaked")
    assert (E["scheme"][pk] == "desc").all() and not E["refine"][pk].any() and not E["overflow"][pk].any()
    n_spp = spp(T)
    if f"few{n_spp}" in kinds:
        lo, hi = rows(f"few{n_spp}"), rows(f"few{n_spp + 1}")
        assert (E["n_surv"][lo] == n_spp).all() and (E["n_surv_slack"][lo] == n_spp).all() and (E["scheme"][lo] == "by_term").all()
        assert (E["n_surv"][hi] == n_spp + 1).all() and (E["n_surv_slack"][hi] == n_spp + 1).all() and (E["scheme"][hi] == "per_lane").all()
    if "cap256" in kinds:
        for j in (255, 256, 257, 300):
            m = rows(f"cap{j}")
            assert (E["n_surv"][m] == j).all() and (E["overflow"][m] == (j > CAP)).all(), f"{name}: cap{j}"
            assert not E["refine"][m].any()
    if "slack" in kinds:
        m = rows("slack")
        assert (E["n_surv_slack"][m] > CAP).all() and (E["n_surv"][m] == 200).all() and not E["overflow"][m].any()
    if "refine_wide" in kinds:
        for k in ("refine_none", "refine_bad", "refine_wide"):
            assert E["refine"][rows(k)].all(), f"{name}: {k}"
        assert (E["widen"][rows("refine_wide")] >= 2).all()
        assert (E["widen"][rows("refine_none")] == 0).all()
    if "missing" in kinds:
        m = rows("missing")
        assert E["overflow"][m].any() and (E["n_surv"][m] >= 1).all()  # (all pre-filter cells missing: every live candidate)
    if f"far{n_spp + 1}" in kinds and name not in ("t4",):  # (t4: two of the three pre-filter terms are short: everything passes)
        a, b = rows("far2"), rows(f"far{n_spp + 1}")
        assert E["refine"][a].all() and E["refine"][b].all() and not E["overflow"][a].any() and not E["overflow"][b].any()
        assert (E["scheme"][a] == "by_term").all() and (E["scheme"][b] == "per_lane").all()
    if "twin" in kinds:
        assert (E["n_surv"][rows("twin")] == 2).all()
    if name == "blocks":
        a, b = rows("block_a"), rows("block_b")
        assert E["kblk"] > BLK_CAP
        assert (E["n_pass_blocks"][a] > BLK_CAP).all() and (E["n_surv"][a] <= CAP).all() and not E["overflow"][a].any()
        assert (E["n_pass_blocks"][b] <= BLK_CAP).all() and (E["n_pass_blocks"][b] >= 100).all() and not E["dense"][b].any()
    if name == "dense":
        m = rows("dense")
        assert E["kblk"] >= 8 and E["dense"][m].all() and (E["n_pass_blocks"][m] * 4 >= 3 * E["kblk"]).all()
        assert (E["n_surv"][m] <= CAP).all()
    if name == "groups":
        assert len(S["kind"]) >= 4200 and E["settle"][pk].all()


def check_draws(name, S, kind, cur, draws):
    div = diversity(draws)
    for k in sorted(set(kind)):
        if k.startswith(("few", "cap", "slack", "block_")) and k != "slack_near":
            m = kind == k
            assert (div[m] >= 3).sum() * 4 >= m.sum(), f"{name}: {k}: near-deterministic draws"
    assert (draws[kind == "new"] < 0).any(), f"{name}: the oracle never draws the new-row candidate"
    assert ((draws == cur[:, None]) & (cur[:, None] >= 0)).any(), f"{name}: the oracle never keeps the current referent"
