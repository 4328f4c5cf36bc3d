"""Programs whose LATENT class holds StringPrior choices that their atoms do not explain, and the weight a latent sweep
owes a particle that chose — or stands for — the ProposalDummyValue (TEST INFRASTRUCTURE, CPU only).

`Item: name ~ StringPrior(1, L, atoms) [; tag ~ StringPrior(1, Lt, atoms_t)]`,
`Obs: item ~ Item; name_obs ~ AddTypos(item.name) [; name_obs2 ~ AddTypos(item.name[, max_typos])] [; tag_obs ~
AddTypos(item.tag)]`: every choice of Item is a leaf root of the class's latent plan with one or two plain AddTypos
terms — what Engine.latent_dummy_served serves.

block_proposal.jl:49-60 for a latent row.  The enumerated proposal q of a choice lists the atoms a (mass prior(a) x
likelihood of the evidence under a) and the dummy (mass m_d = 1 - sum prior(atoms), likelihood of the evidence under the
PLACEHOLDER "*" x (1 + L) // 2).  A fresh particle that takes the dummy draws v ~ StringPrior and is re-scored on v; a
retained particle whose value is no atom stands for the dummy.  Against the uniform weight Z of an atom particle such a
particle weighs  exp(c(v)),
    c(v) = -log m_d + sum over terms, over the item's observed values o (with multiplicity)
           [ logdensity(o | v) - logdensity(o | placeholder) ]                      (slot_correction)
— strings from the oracle's independent C++ sampler (random_string_prior_at), densities from oracle/literal.py.

Closed forms of one latent row's update against frozen tables (they extend tests/posterior_exact.py's list; s = current
value, c0 = c(s) when s is a drawn string and 0 when s is an atom; x = the fresh particle's value, c1 = c(x) or 0):
  * MH (P = 2): W0 = e^c0 / (e^c0 + e^c1), W1 = 1 - W0, accepted with min(1, W1 / (1e-10 + W0))
        -> out(x) = proposal(x) a(x) + [x == s] (1 - sum proposal a),
           proposal(atom a) = q(a), proposal(string v) = q(dummy) prior(v)  (a drawn string equal to an atom IS that atom)
  * PG, P = 2: the fresh particle is chosen with W1 -> out(x) = proposal(x) W1(x) + [x == s] sum proposal W0
The uncorrected kernel (every weight equal: what the sweeps do without dummy_correction) is the same with c = 0
throughout.  StringPrior(1, L <= 2) makes the strings enumerable: 28 + 784 of them."""
import math

import numpy as np

import posterior_exact as pe

lit = pe.lit
KEEP = object()  # item_program: "leave this observation out of the model"


def item_program(latents, rows, atoms, max_len, tag_atoms=None, tag_len=None, second_max_typos=KEEP, extra=None):
    """latents: [{'name': str[, 'tag': str]}] current values of the Item rows; rows: [(item, name_obs, name_obs2, tag_obs)]
    (None = missing; name_obs2 / tag_obs ignored when the program has no such observation).  second_max_typos: KEEP = no
    second observation of name, else its max_typos (None = unbounded).  extra: {attr: [strings]} current values that are
    neither atoms nor the placeholder (strings drawn earlier)."""
    from pclean_amd.model import AddTypos, LoweredModel, Model, Query, StringPrior
    from pclean_amd.trace import Trace
    m = Model()
    c = m.add_class("Item")
    c.choice("name", StringPrior(1, max_len, atoms))
    if tag_atoms is not None:
        c.choice("tag", StringPrior(1, tag_len, tag_atoms))
    o = m.add_class("Obs")
    bind = {"Name": ("item.name", "name_obs")}
    with o.block():
        o.fk("item", "Item")
        o.choice("name_obs", AddTypos("item.name"))
        if second_max_typos is not KEEP:
            o.choice("name_obs2", AddTypos("item.name", second_max_typos))
            bind["Name2"] = ("item.name", "name_obs2")
        if tag_atoms is not None:
            o.choice("tag_obs", AddTypos("item.tag"))
            bind["Tag"] = ("item.tag", "tag_obs")
    q = Query(m, "Obs", bind)
    dirty = {"Name": [r[1] for r in rows]}
    if "Name2" in bind:
        dirty["Name2"] = [r[2] for r in rows]
    if "Tag" in bind:
        dirty["Tag"] = [r[3] for r in rows]
    lw = LoweredModel(m, q, dirty, None, {("Item", a): list(dict.fromkeys(v)) for a, v in (extra or {}).items()})
    obs = lw.encode_observations(dirty)
    tr = Trace(lw, len(rows), 0)
    attrs = ["name"] + (["tag"] if tag_atoms is not None else [])
    for k, lat in enumerate(latents):
        vals = np.zeros(len(lw.layout["Item"]), dtype=np.int32)
        for a in attrs:
            vals[lw.colidx["Item"][a]] = value_id(lw, a, lat[a])
        assert tr.insert_row("Item", vals) == k
    t = tr.tables["Item"]
    for i, r in enumerate(rows):
        tr.cur[0, i] = r[0]
        t.counts[r[0]] += 1
    return dict(model=m, query=q, dirty=dirty, lw=lw, obs=obs, trace=tr, attrs=attrs, rows=rows, latents=latents)


def value_id(lw, attr, s):
    dom = lw.latent_dom[("Item", attr)]
    d = lw.model.classes["Item"].attr(attr).dist
    return dom.index_of(s) if (s in d.atoms or s == d.dummy_value()) else dom.extra[s]


def terms_of(S, attr):
    """[(dirty column, max_typos)] of the AddTypos observations of Item.attr, in plan order"""
    ocls = S["model"].classes["Obs"]
    out = []
    for col, ref in S["query"].cleanmap.items():
        if ref == "item." + attr:
            out.append((col, ocls.attr(S["query"].obsmap[col]).dist.max_typos))
    return out


def evidence_counts(S, attr, item):
    """per term of Item.attr: {observed string: multiplicity} over the rows referring to `item` (missing ones left out)"""
    out = []
    for col, mt in terms_of(S, attr):
        cnt = {}
        for i, r in enumerate(S["rows"]):
            o = S["dirty"][col][i]
            if r[0] == item and o is not None:
                cnt[o] = cnt.get(o, 0) + 1
        out.append((mt, cnt))
    return out


def dummy_mass_log(S, attr):
    a = S["model"].classes["Item"].attr(attr)
    options, lps, dummy = lit.discrete_proposal(None, "Item", a)
    assert options[-1] is None and dummy == a.dist.dummy_value()
    return lps[-1]


def slot_terms(S, attr, item, v, restricted):
    """the summands of c(v) for (item, attr): [-log m_d] + [cnt l(o | v), -cnt l(o | placeholder)] per (term, observed
    value), float64 — the test's tolerance counts them"""
    ph = S["model"].classes["Item"].attr(attr).dist.dummy_value()
    terms = [-dummy_mass_log(S, attr)]
    for mt, cnt in evidence_counts(S, attr, item):
        for o in sorted(cnt):
            terms.append(cnt[o] * lit.add_typos_logpdf(o, v, mt, restricted))
            terms.append(-cnt[o] * lit.add_typos_logpdf(o, ph, mt, restricted))
    return terms


def slot_correction(S, attr, item, v, restricted):
    """(c(v), tolerance 4 k 2^-53 sum |summand|) — the float64 restatement of one slot's correction"""
    terms = slot_terms(S, attr, item, v, restricted)
    return math.fsum(terms), 4.0 * len(terms) * 2.0 ** -53 * math.fsum(abs(x) for x in terms)


def drawn_string(oracle, lw, attr, seed, block_id, node, particle, sweep_idx, key):
    """the string a fresh particle draws for a chosen dummy of Item.attr: the oracle's sampler at the stream
    pclean_dummy_seed(seed, site of the node, particle, sweep) and element `key` (the latent row)"""
    from pclean_amd import sampling
    d = lw.model.classes["Item"].attr(attr).dist
    k = sampling.dummy_seed(seed, (block_id << 16) | node, particle, sweep_idx)
    return sampling.random_string_prior_at(oracle.RandomOracle(), [k], [key], d.min_len, d.max_len)[0]


def drawn_strings(oracle, lw, attr, seed, block_id, node, particles, sweep_idx, keys):
    from pclean_amd import sampling
    d = lw.model.classes["Item"].attr(attr).dist
    ks = [sampling.dummy_seed(seed, (block_id << 16) | node, int(p), sweep_idx) for p in particles]
    if not ks:
        return []
    return sampling.random_string_prior_at(oracle.RandomOracle(), ks, [int(k) for k in keys], d.min_len, d.max_len)


# ---- enumerable variant: closed forms --------------------------------------------------------------------------------
def all_strings(max_len):
    """every string random(StringPrior(1, max_len)) can return, with the probability that the SAMPLER returns it: length
    uniform on 1..max_len, first letter from the letter probabilities, every further one from its predecessor's column of
    the transition matrix, each table normalised as the inverse-CDF draw normalises it"""
    assert 1 <= max_len <= 2
    init = np.asarray(lit._INIT, dtype=np.float64)
    trans = np.asarray(lit._TRANS, dtype=np.float64)
    init = init / init.sum()
    out = {}
    for i, a in enumerate(lit.ALPHABET):
        out[a] = float(init[i]) / max_len
        if max_len == 2:
            col = trans[:, i] / trans[:, i].sum()
            for j, b in enumerate(lit.ALPHABET):
                out[a + b] = float(init[i] * col[j]) / max_len
    return out


def proposal(atoms, max_len, ev, restricted=False):
    """the enumerated proposal of a choice StringPrior(1, max_len, atoms) whose evidence is ev = [(max_typos, {observed:
    count})]: ({atom: q}, q(dummy), c) with c(v) the log-weight of a particle holding the non-atom string v"""
    from pclean_amd.model import StringPrior
    d = StringPrior(1, max_len, atoms)
    ph = d.dummy_value()

    def lik(v):
        return math.fsum(n * lit.add_typos_logpdf(o, v, mt, restricted) for mt, cnt in ev for o, n in cnt.items())

    lps = [lit.string_prior_logpdf(a, 1, max_len) for a in atoms]
    log_md = math.log1p(-math.exp(lit.logsumexp(lps)))
    sc = {a: lp + lik(a) for a, lp in zip(atoms, lps)}
    sc[None] = log_md + lik(ph)
    q = pe.normalise(sc)
    lik_ph = lik(ph)
    return {a: q.get(a, 0.0) for a in atoms}, q.get(None, 0.0), (lambda v: -log_md + lik(v) - lik_ph)


def _fresh(atoms, max_len, ev, restricted):
    """[(value, proposal probability, log-weight)] of the fresh particle; a drawn string equal to an atom is that atom —
    its weight still the dummy's (the particle chose the dummy and drew it)"""
    qa, qd, c = proposal(atoms, max_len, ev, restricted)
    out = [(a, p, 0.0) for a, p in qa.items() if p > 0]
    if qd > 0:
        for v, pv in all_strings(max_len).items():
            if pv > 0:
                out.append((v, qd * pv, c(v)))
    return out, c


def kernel(atoms, max_len, ev, s, mh, corrected=True, restricted=False):
    """{value: probability} after one update of a row holding s (an atom or a drawn string), MH or PG with P = 2;
    corrected=False: every weight equal (the sweeps without dummy_correction)"""
    fresh, c = _fresh(atoms, max_len, ev, restricted)
    c0 = c(s) if (corrected and s not in atoms) else 0.0
    out, moved = {}, []
    for x, px, c1 in fresh:
        if not corrected:
            c1 = 0.0
        m = max(c0, c1)
        w0, w1 = math.exp(c0 - m), math.exp(c1 - m)
        W0, W1 = w0 / (w0 + w1), w1 / (w0 + w1)
        a = min(1.0, W1 / (1e-10 + W0)) if mh else W1
        out[x] = out.get(x, 0.0) + px * a
        moved.append(px * a)
    out[s] = out.get(s, 0.0) + (1.0 - math.fsum(moved))
    return {k: v for k, v in out.items() if v > 0}


def simulate(atoms, max_len, ev, s, mh, n, rng, corrected=True, restricted=False):
    """n updates by the MECHANISM (propose an option, draw the string letter by letter, weigh, accept / pick) — not by
    sampling the closed form: {value: count}"""
    qa, qd, c = proposal(atoms, max_len, ev, restricted)
    opts = list(qa) + [None]
    pr = np.array([qa[a] for a in qa] + [qd])
    pr = pr / pr.sum()
    init = np.asarray(lit._INIT, dtype=np.float64)
    trans = np.asarray(lit._TRANS, dtype=np.float64)
    c0 = c(s) if (corrected and s not in atoms) else 0.0
    memo = {}
    out = {}
    picks = rng.choice(len(opts), size=n, p=pr)
    lens = rng.integers(1, max_len + 1, size=n)
    u = rng.random(n)
    for i in range(n):
        x = opts[picks[i]]
        c1 = 0.0
        if x is None:
            prev, chars = None, []
            for _ in range(lens[i]):
                p = init if prev is None else trans[:, prev]
                prev = int(rng.choice(28, p=p / p.sum()))
                chars.append(lit.ALPHABET[prev])
            x = "".join(chars)
            if corrected:
                c1 = memo.get(x)
                if c1 is None:
                    c1 = memo[x] = c(x)
        m = max(c0, c1)
        w0, w1 = math.exp(c0 - m), math.exp(c1 - m)
        W0, W1 = w0 / (w0 + w1), w1 / (w0 + w1)
        a = min(1.0, W1 / (1e-10 + W0)) if mh else W1
        got = x if u[i] < a else s
        out[got] = out.get(got, 0) + 1
    return out


# ---- the distribution cases (CPU power test and GPU test share them) --------------------------------------------------
DIST_ATOMS = ["ab", "ba", "c"]
DIST_LEN = 2
DIST_OBS = ["ad", "ad", "a"]      # what every latent row of a case is observed as (three referring rows)
DIST_STRING = "ae"                # the drawn string of the "string state" (no atom)
DIST_ROWS = 256                   # identical latent rows
DIST_SWEEPS = 40                  # sweeps from the frozen state: DIST_ROWS x DIST_SWEEPS draws per case
DIST_CASES = [("MH-atom", True, "ab"), ("MH-string", True, DIST_STRING), ("PG-atom", False, "ab"),
              ("PG-string", False, DIST_STRING)]


def dist_evidence():
    cnt = {}
    for o in DIST_OBS:
        cnt[o] = cnt.get(o, 0) + 1
    return [(None, cnt)]


def dist_program(state):
    """DIST_ROWS identical Item rows holding `state`, each observed by len(DIST_OBS) rows"""
    latents = [{"name": state} for _ in range(DIST_ROWS)]
    rows = [(k, o, None, None) for k in range(DIST_ROWS) for o in DIST_OBS]
    extra = {"name": [state]} if state not in DIST_ATOMS else None
    return item_program(latents, rows, DIST_ATOMS, DIST_LEN, extra=extra)


# ---- the weights program (the GPU test's shapes) -----------------------------------------------------------------------
# atoms longer than the placeholder "***" and over letters no observation holds: against any observed word the placeholder
# needs no more edits than an atom and pays less per edit (log 3 < log 5), so the dummy wins wherever a name is observed
W_ATOMS = ["qqqqq", "zzzzzz"]
W_LEN = 6                         # drawn lengths 1 .. 6
W_TAG_ATOMS = ["x", "yy"]
W_TAG_LEN = 3
W_SECOND_MAX_TYPOS = 2
# item -> number of distinct observed names (the correction kernel's lanes stride over them 64 at a time)
W_DISTINCT = {2: 1, 3: 63, 4: 64, 5: 65, 6: 300}
W_STRING_ITEMS = {7: ("ca", "x"), 8: ("the", "zq")}  # rows that hold drawn strings (particle-0 slots): (name, tag)
W_EXPLAINED = range(9, 21)        # rows whose atoms explain their observations: no dummy, every weight 0


def _observed_words(rng, n):
    """n distinct strings of 1 .. 40 symbols over the sampler's alphabet; among them "y?x" for frequent letter pairs xy — a
    transposition followed by an insertion tells the two Damerau-Levenshtein flavours apart ("ca" / "abc")"""
    letters = "etaoinshr dlu"
    out = ["abc", "hat", "hte", "eht", "nia", "rae", "no", "u", "t"]
    for a in "ethansior":
        for b in "ethansior":
            if a != b:
                out.append(b + "a" + a)
    out = list(dict.fromkeys(out))
    while len(out) < n:
        k = int(rng.integers(1, 41)) if len(out) % 3 == 0 else int(rng.integers(1, 8))
        w = "".join(letters[int(j)] for j in rng.integers(0, len(letters), size=k))
        if w not in out:
            out.append(w)
    return out[:n]


def weights_program(seed=0):
    """Items of every shape the correction kernel tells apart: no referring row (item 0), missing observations only (1),
    1 / 63 / 64 / 65 / 300 distinct observed names with multiplicities above 1, observed lengths 1 .. 40, a second
    observation of the name with max_typos, a second served choice (tag), rows holding drawn strings, and rows whose atoms
    explain their observations."""
    rng = np.random.default_rng(seed)
    n_items = max(W_EXPLAINED) + 1
    latents = [{"name": W_ATOMS[0], "tag": "x"} for _ in range(n_items)]
    for k, (nm, tg) in W_STRING_ITEMS.items():
        latents[k] = {"name": nm, "tag": tg}
    rows = [(1, None, None, None), (1, None, None, "yx")]
    words = _observed_words(rng, 300)
    for item, n in W_DISTINCT.items():
        for j, w in enumerate(words[:n]):
            reps = 1 + (j % 7 == 0) + (j % 31 == 0)  # multiplicities 1 .. 3
            for r in range(reps):
                second = w if (j + r) % 3 == 0 else (None if (j + r) % 3 == 1 else words[(j + 5) % n])
                tag = None if j % 4 else ["x", "zq", "yy", "o r"][(j // 4) % 4]
                rows.append((item, w, second, tag))
    rows += [(7, "abc", "abc", "x"), (7, "abc", None, None), (7, "ca", "cab", "x"), (7, None, "c", None)]
    rows += [(8, "the", "hte", "zq"), (8, "then", None, "z"), (8, "hat", "eht", "qz"), (8, "hat", None, "zq")]
    for k in W_EXPLAINED:
        rows += [(k, W_ATOMS[0], W_ATOMS[0], "x")] * 3
    extra = {"name": [v[0] for v in W_STRING_ITEMS.values()], "tag": [v[1] for v in W_STRING_ITEMS.values() if v[1] not in W_TAG_ATOMS]}
    S = item_program(latents, rows, W_ATOMS, W_LEN, tag_atoms=W_TAG_ATOMS, tag_len=W_TAG_LEN,
                     second_max_typos=W_SECOND_MAX_TYPOS, extra=extra)
    assert max(len(r[1]) for r in rows if r[1]) >= 38 and min(len(r[1]) for r in rows if r[1]) == 1
    return S
