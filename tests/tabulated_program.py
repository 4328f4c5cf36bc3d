"""A small name / nickname program written with the tabulated likelihood terms, and a pure-Python restatement of them.

    Person:  name ~ StringPrior(1, 30, names)        nick ~ StringPrior(1, 12, nicks)
    Obs:     p ~ Person
             name_obs  ~ FormatName(p.name)                    (format_name.jl:33-55, the one-name method)
             long_obs  ~ ExpandOnShortVersion(p.nick, longs)    (expand_on_short_version.jl:30-41)
             name_typo ~ AddTypos(p.name)

The frozen oracle does not know these terms, so the tests carry this restatement (as tests/two_gauss_program.py does for
the Gaussian blocks).  Julia's `lowercase` maps character by character; `_low` below does the same with the
single-character rule of pclean_amd.encode.StringPool (a character whose lowercase is not one character stands for itself)."""
import numpy as np

from pclean_amd import _lib
from pclean_amd.model import AddTypos, ExpandOnShortVersion, FormatName, LoweredModel, Model, Query, StringPrior

SHORT, FORMAT = _lib.CLASS_SHORT_VERSION, _lib.CLASS_FORMAT_NAME


def _low(ch):
    low = ch.lower()
    return low if len(low) == 1 else ch


def fold(s):
    return [_low(ch) for ch in s]


def _short_folded(short, long):
    """expand_on_short_version.jl:6-19, the two-pointer loop, on sequences of lowercased characters"""
    a, b = 0, 0
    s, l = len(short), len(long)
    while a < s and b < l:
        if short[a] == long[b]:
            a += 1
        b += 1
    return a >= s


def is_short_version(short, long):
    return _short_folded(fold(short), fold(long))


def format_name_class(observed, name):
    """0: equal ignoring case, 1: observed is the name's initial + ".", 2: neither (format_name.jl:47-54)"""
    if fold(observed) == fold(name):
        return 0
    if len(name) >= 1 and fold(observed) == fold(name[0] + "."):
        return 1
    return 2


def pair_class(rule, observed, latent):
    if rule == SHORT:
        return 0 if is_short_version(latent, observed) else 1
    return format_name_class(observed, latent)


def class_table(rule, observed_strings, latent_strings):
    if rule == SHORT:  # (the strings lowercased once, not once per pair)
        fo, fl = [fold(o) for o in observed_strings], [fold(v) for v in latent_strings]
        rows = [[0 if _short_folded(v, o) else 1 for v in fl] for o in fo]
    else:
        rows = [[format_name_class(o, v) for v in latent_strings] for o in observed_strings]
    return np.array(rows, dtype=np.uint16).reshape(len(observed_strings), len(latent_strings))


def short_counts(latent_strings, options):
    return np.array([sum(is_short_version(v, x) for x in options) for v in latent_strings], dtype=np.int32)


def density_rows(rule, latent_strings, options=None):
    """T[value][class 0, 1, 2, missing observation] in float64"""
    T = np.full((len(latent_strings), 4), -1000.0)
    if rule == SHORT:
        for v, s in enumerate(latent_strings):
            n = int(sum(is_short_version(s, x) for x in options))
            if n > 0:
                T[v, 0] = -np.log(np.float64(n))
            T[v, 3] = 0.0 if s in options else -1000.0
        return T
    for v, s in enumerate(latent_strings):
        if s != "":
            T[v, 0], T[v, 1] = np.log(0.9999), np.log(0.0001)
        T[v, 3] = 0.0 if s == "" else (-1000.0 if "*" in s else -5.0)
    return T


# ---- the program ---------------------------------------------------------------------------------------------------
NAMES = ["Jim", "Émile", "J", "anna", "BORIS", "Carla", "dmitri", "Elena", "Farid", "Greta", "hiro", "Ines", "Jonas",
         "Katya", "Lars", "MIRA", "Nils", "Olga", "pablo", "Quinn", "Rosa", "Sven", "Tara", "Ugo", "Vera", "Wim", "Xena",
         "Yuri", "Zoe", "Abel", "berta", "Cyrus", "Dora", "Egon", "Fay", "Gus", "Hana", "Ivo", "Jana", "Kurt"]
NICKS = ["jim", "Bob", "al", "Liz", "tom", "Sam", "Ed", "kat", "ron", "Meg", "dan", "Joe"]
NICKS_AMONG_LONGS = ["Sam", "Ed", "Liz", "Joe"]  # a nick that is itself an option scores 0 against a missing observation
NO_NICK = ["Qqq", "Zzxw", "Xyzzy", "Www", "Vvuu", "Qzq"]


def long_forms():
    """50 long forms: the four nicks above as they are, 40 made from a nick by inserting letters (mixed case), and the six
    of NO_NICK, which hold no nick as a subsequence"""
    rng = np.random.default_rng(7)
    out = list(NICKS_AMONG_LONGS)
    k = 0
    while len(out) < 44:
        nick = NICKS[k % len(NICKS)]
        k += 1
        w = list(nick)
        for _ in range(int(rng.integers(1, 6))):
            w.insert(int(rng.integers(0, len(w) + 1)), "xyzwvq"[int(rng.integers(0, 6))])
        w = "".join(ch.upper() if rng.random() < 0.3 else ch for ch in w)
        if w not in out:
            out.append(w)
    out += NO_NICK
    assert len(out) == 50 and len(set(out)) == 50
    assert all(not any(is_short_version(n, x) for n in NICKS) for x in NO_NICK)
    return out


LONGS = long_forms()


def model():
    m = Model()
    p = m.add_class("Person")
    p.choice("name", StringPrior(1, 30, NAMES))
    p.choice("nick", StringPrior(1, 12, NICKS))
    o = m.add_class("Obs")
    o.fk("p", "Person")
    o.choice("name_obs", FormatName("p.name"))
    o.choice("long_obs", ExpandOnShortVersion("p.nick", LONGS))
    o.choice("name_typo", AddTypos("p.name"))
    return m


def query(m):
    return Query(m, "Obs", {"Name": ("p.name", "name_obs"), "Long": ("p.nick", "long_obs"), "Typo": ("p.name", "name_typo")})


def _typo(rng, s):
    if len(s) < 2 or rng.random() < 0.5:
        return s
    i = int(rng.integers(0, len(s)))
    return s[:i] + "q" + s[i + 1:]


def data(n_rows=64, seed=5):
    """64 observed rows of 20 people.  name_obs is the person's name in some case or its initial + "."; long_obs one of
    the long forms the person's nick is a short version of; name_typo the name with at most one substitution.  Each
    column is missing in 8 rows, all three in rows 0 and 1."""
    rng = np.random.default_rng(seed)
    people = [(NAMES[i], NICKS[i % len(NICKS)]) for i in range(20)]
    dirty = {"Name": [], "Long": [], "Typo": []}
    who = []
    for i in range(n_rows):
        name, nick = people[int(rng.integers(0, len(people)))]
        who.append((name, nick))
        u = rng.random()
        dirty["Name"].append(name[0] + "." if u < 0.25 else (name.upper() if u < 0.5 else (name.lower() if u < 0.75 else name)))
        fits = [x for x in LONGS if is_short_version(nick, x)]
        dirty["Long"].append(fits[int(rng.integers(0, len(fits)))])
        dirty["Typo"].append(_typo(rng, name))
    for c, col in enumerate(("Name", "Long", "Typo")):
        for i in [0, 1] + [2 + 6 * c + j for j in range(6)]:  # 8 rows per column; rows 0 and 1 miss all three
            dirty[col][i] = None
    return dirty, who


def setup():
    dirty, who = data()
    m = model()
    q = query(m)
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    return dict(dirty=dirty, who=who, model=m, query=q, lw=lw, obs=obs)


def term_tables(lw):
    """{pair id: (rule, class table [n_obs][n_lat], T [n_lat][4])} of the lowered program's tabulated terms, restated"""
    out = {}
    for pid, (rule, odom, ldom, options) in lw.class_pairs.items():
        ostr = [odom.string(u) for u in range(len(odom))]
        lstr = [ldom.string(v) for v in range(len(ldom))]
        out[pid] = (rule, class_table(rule, ostr, lstr), density_rows(rule, lstr, options))
    return out
