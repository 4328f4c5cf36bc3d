"""The two-class program of test_big_option_list_kernel_parity (A.x ~ ChooseUniformly(words); Obs.a -> A;
Obs.y ~ AddTypos(a.x)) with data that keep the posteriors flat, for the tests that pin every launch variant of the
generic enumeration (test_enum_variants_cpu.py, test_gpu_enum_variants.py):

  * words are 4-8 letters over "abcdefgh": a five-letter string has many options one or two edits away;
  * a third of the observed cells (rows 0, 3, 6, ...) are the clean word;
  * a few cells are missing (every MISSING_EVERY-th row from row 5 on, and every cell of the last entity);
  * the rest are five-letter strings that are NOT options, from a pool of at most POOL such strings, so that the pair
    table stays within (POOL + n_latent) x n_options however many rows there are.

The latent state has n_latent entities, clean[i] = words[i % n_latent].  Up to n_options entities that is
Trace.from_clean_values; beyond, from_clean_values would merge the entities that hold the same word, so the rows of A
are inserted directly (entity e holds words[e % n_options]: several rows of A with the same value, a state inference
reaches whenever two rows create the same new referent).  `crowd` further rows at the end all refer to entity 0: an
evidence set of more than 64 rows without 64 rows for every entity."""
import numpy as np

from pclean_amd.model import AddTypos, ChooseUniformly, LoweredModel, Model, Query
from pclean_amd.trace import Trace

LETTERS = list("abcdefgh")
POOL = 200
MISSING_EVERY = 41


def make_words(n_options, rnd):
    words, seen = [], set()
    while len(words) < n_options:
        w = "".join(rnd.choice(LETTERS, size=rnd.integers(4, 9)))
        if w not in seen:
            seen.add(w)
            words.append(w)
    return words, seen


def program(n_options, n_rows, n_latent, seed, crowd=0, strength=None):
    """dict(lw, obs, trace, words, dirty, n_latent): n_rows observed rows over n_latent entities, plus `crowd` rows of
    entity 0.  strength: the Pitman-Yor strength of class A (default 1: among thousands of entities no draw would ever
    take the new-row candidate of the reference slot)."""
    rnd = np.random.default_rng(seed)
    words, seen = make_words(n_options, rnd)
    pool = []
    while len(pool) < POOL:
        s = "".join(rnd.choice(LETTERS, size=5))
        if s not in seen:
            seen.add(s)
            pool.append(s)
    ent = np.concatenate([np.arange(n_rows) % n_latent, np.zeros(crowd, dtype=np.int64)])
    n = len(ent)
    pick = rnd.integers(0, POOL, n)
    dirty = []
    for i in range(n):
        if ent[i] == n_latent - 1 or (i % MISSING_EVERY == 5 and i % 3):
            dirty.append(None)
        elif i % 3 == 0:
            dirty.append(words[ent[i] % n_options])
        else:
            dirty.append(pool[pick[i]])
    m = Model()
    a = m.add_class("A")
    a.choice("x", ChooseUniformly(words))
    if strength is not None:
        a.py_strength = float(strength)
    o = m.add_class("Obs")
    o.fk("a", "A")
    o.choice("y", AddTypos("a.x"))
    q = Query(m, "Obs", {"Y": ("a.x", "y")})
    dirty = {"Y": dirty}
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    if n_latent <= n_options:
        tr = Trace.from_clean_values(lw, [{"x": [words[e] for e in ent]}], n, 0)
    else:
        tr = Trace(lw, n, 0)
        dom = lw.latent_dom[("A", "x")]
        vals = np.array([dom.index_of(w) for w in words], dtype=np.int32)
        ids = tr.insert_rows_bulk("A", vals[np.arange(n_latent) % n_options][:, None])
        tr.cur[0] = ids[ent]
        t = tr.tables["A"]
        t.counts[:t.n] += np.bincount(tr.cur[0], minlength=t.n)
    return dict(lw=lw, obs=obs, trace=tr, words=words, dirty=dirty, n_latent=n_latent)


def diversity(draws):
    """distinct values per row of draws [n][k]"""
    s = np.sort(draws, axis=1)
    return 1 + (s[:, 1:] != s[:, :-1]).sum(axis=1)


# ---- the shapes (shared by the CPU and the GPU tests) ----------------------------------------------------------------
# Thresholds of pclean_launch_enum when these were chosen (lds = ((nc + 1) & ~1) * 8 + 640 bytes): workgroups of 1024
# threads up to 1 024 items, or up to 65 536 from nc >= 2 481 (lds > 20 KB); the recomputing kernel from nc >= 10 161
# (lds > 80 KB) for launches of more than 65 536 items that want neither scores nor several draws, and for every launch
# from nc >= 20 401 (lds > 160 KB); the scores-first kernel of a split launch for up to 64 items from nc >= 4 096 (with
# evidence sets: up to 1 024 items from nc >= 2 048) when no scores are asked for.
SEED = 3
N_DRAWS = 7

# leaf, score_node(0, 1, rows): {n_options: (rows of the program, [(items, call, n_draws, slots that must have run)])};
# call "gen" = force_generic(True) without scores, "scores" = want_scores=True.  Every call is repeated on the default
# path (no force_generic, no scores: the coarse-prefix leaf kernels, LEAF_CB = 256 options per block).
LEAF_SHAPES = {
    256: (1025, [(1025, "gen", N_DRAWS, {"lds_256"})]),     # n > BT of enum_node_kernel<256>: per-thread scoring ...
    257: (1025, [(1025, "gen", N_DRAWS, {"lds_256"})]),     # ... and the batched one
    1024: (65, [(64, "gen", N_DRAWS, {"lds_1024"})]),       # the same switch of enum_node_kernel<1024>
    1025: (65, [(64, "gen", N_DRAWS, {"lds_1024"})]),
    4095: (65, [(64, "gen", N_DRAWS, {"lds_1024"})]),       # one candidate short of the split launch
    4096: (65, [(64, "gen", N_DRAWS, {"lds_1024", "scores"}),
                (65, "gen", N_DRAWS, {"lds_1024"}),         # one item too many for it
                (64, "scores", N_DRAWS, {"lds_1024"})]),    # scores asked for: no split
    20400: (65, [(8, "scores", N_DRAWS, {"lds_1024"}),      # the longest list whose scores fit LDS (exactly 160 KB)
                 (8, "gen", N_DRAWS, {"lds_1024", "scores"})]),
    20401: (65, [(64, "gen", N_DRAWS, {"big_1024", "scores"}),  # the first list beyond LDS
                 (65, "gen", N_DRAWS, {"big_1024"}),
                 (8, "scores", N_DRAWS, {"big_1024"})]),
    10161: (65537, [(65537, "gen", 1, {"big_256"}),         # more items than the wide kernels take, one draw
                    (65537, "gen", 2, {"lds_256"})]),       # two draws: back to LDS, 81 936 bytes per workgroup
}

# reference slot, score_node(0, 0, rows, excl=cur): (latent rows = observed rows, items, slots).  300 options; CROWD
# further rows of entity 0 (a referent that survives the exclusion of one row) make up the second half of the items, at
# most CROWD of them; strength n_latent / FK_STRENGTH_DIV lets the new-row candidate (slot nc - 1 = n_latent) be drawn.
FK_OPTIONS = 300
CROWD = 64
FK_STRENGTH_DIV = 16
FK_SHAPES = [
    (257, 64, {"lds_1024"}),
    (1025, 64, {"lds_1024"}),
    (4094, 64, {"lds_1024"}),              # nc = 4 095
    (4095, 64, {"lds_1024", "scores"}),    # nc = n + 1 = 4 096: the split side
    (4096, 64, {"lds_1024", "scores"}),
    (1100, 1025, {"lds_256"}),
    (20400, 8, {"big_1024", "scores"}),    # nc = 20 401
]

# evidence sets, sweep_latent on A's plan with PCLEAN_NO_FAST_EV=1: (options, latent rows, slots that must have run,
# slots that must not).  Three observed rows per latent row and EV_CROWD more for entity 0.
EV_CROWD = 70
EV_SHAPES = [
    (300, 50, {"lds_1024_ev"}, {"scores_ev", "lds_256_ev", "big_1024_ev", "big_256_ev"}),
    (300, 1100, {"lds_256_ev"}, {"scores_ev", "big_1024_ev", "big_256_ev"}),
    (2047, 50, {"lds_1024_ev"}, {"scores_ev", "lds_256_ev", "big_1024_ev", "big_256_ev"}),
    (2048, 50, {"lds_1024_ev", "scores_ev"}, {"lds_256_ev", "big_1024_ev", "big_256_ev"}),
    (20401, 50, {"big_1024_ev", "scores_ev"}, {"lds_256_ev", "lds_1024_ev", "big_256_ev"}),
]
EV_CONFIGS = [(6, False), (2, True)]  # (particles, MH instead of PG)


def leaf_program(n_options):
    return program(n_options, LEAF_SHAPES[n_options][0], min(50, n_options), SEED)


def fk_program(n_latent):
    return program(FK_OPTIONS, n_latent, n_latent, SEED, crowd=CROWD, strength=n_latent / FK_STRENGTH_DIV)


def fk_items(n_latent, items):
    h = min(items // 2, CROWD)
    return np.concatenate([np.arange(items - h), n_latent + np.arange(h)]).astype(np.int32)


def ev_program(n_options, n_latent):
    return program(n_options, 3 * n_latent, n_latent, SEED, crowd=EV_CROWD)


def big_sample(n_rows, k=256):
    """the rows of the 65 537-item shape that are compared with the oracle: both ends, both sides of 1 024 and of the
    middle, and seeded others up to k rows (a cap on the oracle's share of the test's time, not a tolerance)"""
    fixed = [0, 1, 1023, 1024, 1025, n_rows // 2 - 1, n_rows // 2, n_rows // 2 + 1, n_rows - 2, n_rows - 1]
    rest = np.setdiff1d(np.arange(n_rows), fixed)
    more = np.random.default_rng(SEED).choice(rest, size=k - len(fixed), replace=False)
    return np.sort(np.concatenate([fixed, more])).astype(np.int32)


def oracle_world(oracle, helpers, S, engine=None):
    """the oracle's World of program S: with an engine its tables are read back from the device, else computed"""
    if engine is not None:
        return helpers.mirror_world(oracle, S["lw"], S["obs"], S["trace"], engine)
    ol = helpers.option_logp_cpu(oracle, S["lw"], S["trace"])
    return helpers.mirror_world(oracle, S["lw"], S["obs"], S["trace"], None, dist_mode=0, option_logp=ol)


def oracle_leaf(world, S, rows, n_draws, want_scores=False):
    return world.score_node(0, 1, rows, seed=1, sweep=2, n_draws=n_draws, n_cand=len(S["words"]), want_scores=want_scores)


def oracle_fk(world, S, rows, excl):
    """(lse, None, draws) of the reference slot; the oracle's score_node takes the new-row branch's marginal (the
    leaf's log-marginal of every row) as an input where the device evaluates the sub-tree"""
    snew = world.score_node(0, 1, rows)[0]
    return world.score_node(0, 0, rows, excl=excl, snew=snew, seed=1, sweep=2, n_draws=N_DRAWS, n_cand=S["trace"].tables["A"].n + 1)
