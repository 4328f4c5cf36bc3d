"""A Person / Obs program written with the three-name FormatName, and a pure-Python restatement of that term.

    Person:  first, middle, last          (Unmodeled, or one of them an enumerated choice: see VARIANTS)
    Obs:     p ~ Person
             full ~ FormatName(p.first, p.middle, p.last)          (format_name.jl:14-26)
             p.first / p.middle / p.last observed directly, except the variant's open name

The frozen oracle does not know this term, so the tests carry the restatement below (as tests/tabulated_program.py does
for the tabulated terms): `str.lower()` of the concatenations, written from format_name.jl:14-26.  It shares nothing
with the lowering: no symbols, no fold ids, no byte tables.  (Every character used here lowercases to one character, so
`str.lower()` is Julia's per-character `lowercase`.)"""
import math

import numpy as np

from pclean_amd.model import ChooseUniformly, FormatName, LoweredModel, Model, Query, StringPrior, Unmodeled

LOG_THREE = math.log(0.9) + math.log(0.9) + math.log(0.9)  # (added left to right, as format_name.jl:18 adds them)
LOG_TWO = math.log(0.1)
NEITHER = -1000.0


def name3_logdensity(observed, first, middle, last):
    """logdensity(::FormatName, observed, first, middle, last), format_name.jl:14-26; observed None = missing"""
    if observed is None:
        return 0.0
    if observed.lower() == f"{first} {middle} {last}".lower():
        return LOG_THREE
    if observed.lower() == f"{first} {last}".lower():
        return LOG_TWO
    return NEITHER


def is_prefix(observed, name):
    """the byte of PCLEAN_CLASS_NAME_PREFIX: lowercase(observed) starts with lowercase(name) and a space"""
    return 1 if observed.lower().startswith((name + " ").lower()) else 0


def is_suffix(observed, name):
    """the byte of PCLEAN_CLASS_NAME_SUFFIX: lowercase(observed) ends with a space and lowercase(name)"""
    return 1 if observed.lower().endswith((" " + name).lower()) else 0


def affix_table(fn, observed_strings, latent_strings):
    return np.array([[fn(o, v) for v in latent_strings] for o in observed_strings],
                    dtype=np.uint16).reshape(len(observed_strings), len(latent_strings))


# ---- the program ---------------------------------------------------------------------------------------------------
# a dozen tokens, several of them made of others, so that prefixes and suffixes collide ("al al al al" splits two ways)
FIRSTS = ["al", "al al", "bo", "Émile", "ana", "DE", "o"]
MIDDLES = ["", "al", "bo", "cy", "de la", "Ü", "Ng"]
LASTS = ["al", "al al", "bo cy", "cy", "Ng", "de la", "émile", "Ü"]
FORCED = [("al", "al", "al al"), ("al al", "al", "al"), ("al", "bo", "cy"), ("al", "", "bo cy"), ("al", "cy", "bo cy"),
          ("al", "", "al"), ("al al", "", "al"), ("Émile", "Ü", "émile"), ("o", "", "Ü")]
VARIANTS = ("observed", "middle", "last")  # which name is an enumerated choice of a new Person row ("observed": none)


def people(n=300, seed=3):
    rng = np.random.default_rng(seed)
    out = list(FORCED)
    while len(out) < n:
        p = (FIRSTS[int(rng.integers(0, len(FIRSTS)))], MIDDLES[int(rng.integers(0, len(MIDDLES)))],
             LASTS[int(rng.integers(0, len(LASTS)))])
        if p not in out:
            out.append(p)
    return out


def _recase(rng, s):
    u = rng.random()
    return s.upper() if u < 0.25 else (s.lower() if u < 0.5 else (s.title() if u < 0.6 else s))


def data(n_rows=1100, seed=5):
    """1100 rows of 300 people.  Full is "first middle last" in some case (45 %), "first last" (25 %), another person's
    full name (10 %), the full name with one wrong letter (10 %) or missing (10 %); the first rows hold the hand-picked
    collisions.  First / Middle / Last are the person's own values, never missing."""
    rng = np.random.default_rng(seed)
    ppl = people()
    dirty = {"First": [], "Middle": [], "Last": [], "Full": []}
    who = []
    for i in range(n_rows):
        j = i if i < len(FORCED) else int(rng.integers(0, len(ppl)))
        f, m, l = ppl[j]
        who.append(j)
        u = rng.random()
        if i < len(FORCED) or u < 0.45:
            full = _recase(rng, f"{f} {m} {l}")
        elif u < 0.70:
            full = _recase(rng, f"{f} {l}")
        elif u < 0.80:
            full = " ".join(ppl[int(rng.integers(0, len(ppl)))])
        elif u < 0.90:
            full = f"{f} {m} {l}"
            k = int(rng.integers(0, len(full)))
            full = full[:k] + "q" + full[k + 1:]
        else:
            full = None
        dirty["First"].append(f)
        dirty["Middle"].append(m)
        dirty["Last"].append(l)
        dirty["Full"].append(full)
    return dirty, who, ppl


def model(variant, tagged=False):
    m = Model()
    p = m.add_class("Person")
    if tagged:  # a never observed attribute with one value per person: it tells the rows of the Person table apart
        p.choice("tag", ChooseUniformly(TAGS))
    p.choice("first", Unmodeled())
    p.choice("middle", ChooseUniformly(MIDDLES) if variant == "middle" else Unmodeled())
    p.choice("last", StringPrior(1, 20, LASTS) if variant == "last" else Unmodeled())
    o = m.add_class("Obs")
    o.fk("p", "Person")
    o.choice("full", FormatName(first="p.first", middle="p.middle", last="p.last"))
    return m


def query(m, variant):
    b = {"Full": ("p.first", "full"), "First": "p.first", "Middle": "p.middle", "Last": "p.last"}
    if variant != "observed":
        del b[variant.capitalize()]
    return Query(m, "Obs", b)


TAGS = [f"t{j}" for j in range(300)]


def setup(variant, tagged=False):
    dirty, who, ppl = data()
    m = model(variant, tagged)
    q = query(m, variant)
    cols = {c: v for c, v in dirty.items() if c in q.obsmap}
    lw = LoweredModel(m, q, cols)
    obs = lw.encode_observations(cols)
    return dict(variant=variant, dirty=dirty, who=who, people=ppl, model=m, query=q, lw=lw, obs=obs)


# ---- candidate tables of a chosen size ----------------------------------------------------------------------------------
def candidates(k, seed=11):
    """(people, counts) of a Person table with k rows: the program's 300 people first, then random combinations (repeats
    allowed: a latent table may hold equal rows); every 17th row is a free slot (count 0)"""
    rng = np.random.default_rng(seed)
    ppl = people()
    while len(ppl) < k:
        ppl.append((FIRSTS[int(rng.integers(0, len(FIRSTS)))], MIDDLES[int(rng.integers(0, len(MIDDLES)))],
                    LASTS[int(rng.integers(0, len(LASTS)))]))
    counts = np.array([0 if j % 17 == 16 else 1 + j % 3 for j in range(k)], dtype=np.int64)
    return ppl[:k], counts


# candidate counts the GPU tests score (tests/test_gpu_name3.py): (candidates, rows, expected launch variant)
#   63 / 64 / 65: around a wavefront;  256 / 257: enum_node_kernel<256> goes from one candidate per thread to batches of
#   ENUM_CPT;  1030 on few rows: enum_node_kernel<1024> with batches;  20600: beyond the 160 KB of LDS (20 478 scores),
#   enum_node_big_kernel
SCORE_CASES = [(63, None, "lds_256"), (64, None, "lds_256"), (65, None, "lds_256"), (256, None, "lds_256"),
               (257, None, "lds_256"), (1030, 16, "lds_1024"), (20600, 8, "big_1024")]


def case_rows(n_rows, rows):
    """row ids of a score case: all of them (more than 1024 items: 256 threads per item), or the first `rows`"""
    return np.arange(n_rows if rows is None else rows, dtype=np.int32)


class Restated:
    """name3_logdensity with a memo over (observed, first, middle, last): the tables repeat people and strings"""

    def __init__(self):
        self.memo = {}

    def __call__(self, observed, f, m, l):
        key = (observed, f, m, l)
        v = self.memo.get(key)
        if v is None:
            v = self.memo[key] = name3_logdensity(observed, f, m, l)
        return v
