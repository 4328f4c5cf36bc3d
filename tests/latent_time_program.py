"""Programs whose LATENT class holds KEYED choices that their atoms do not explain — TimePrior choices under MaybeSwap
evidence (flights' shape) and keyed StringPrior choices under AddTypos evidence (rents' shape) — and the weight a latent
sweep owes a particle that chose, or stands for, the ProposalDummyValue (TEST INFRASTRUCTURE, CPU only; the unkeyed
StringPrior case is tests/latent_dummy_program.py).

    Src:  name ~ StringPrior(..)
    Trip: key ~ StringPrior(..); dep ~ TimePrior(atoms, "key") [; arr ~ TimePrior(atoms2, "key")]
          [; label ~ StringPrior(1, L, atoms)] [; name ~ StringPrior(1, Ln, atoms, keyed_by="key")]
    Obs:  trip ~ Trip [; label_obs ~ AddTypos(trip.label)] [; name_obs ~ AddTypos(trip.name)]; src ~ Src;
          error_prob = ProbLookup(error_probs, (src, key) -> src)(src.name, trip.key);
          dep_obs ~ MaybeSwap(trip.dep, atoms, trip.key, error_prob) [; arr_obs ~ MaybeSwap(trip.arr, ..)]

block_proposal.jl:49-60 for a latent row whose choice is keyed: the enumerated proposal lists the atoms OF THE ROW'S KEY and
that key's dummy (mass m_d(key), likelihood of the evidence under the PLACEHOLDER).  A fresh particle that takes the dummy
draws v (random(TimePrior) / random(StringPrior)) and is re-scored on v; a retained particle whose value is no option of its
key stands for the dummy.  Such a particle weighs exp(c(v)) against the uniform weight of an atom particle,
    c(v) = -log m_d(key) + sum over the row's evidence rows e [ l(o_e | v) - l(o_e | placeholder) ]         (slot_terms)
with l = maybe_swap.jl:13-28 (options = the key's atoms, prob = the evidence row's error probability; a MISSING observation
scores 0 when v is one of the key's atoms and -1000 otherwise) or add_typos.jl:50-66 (missing observations add nothing).
Densities come from oracle/literal.py, drawn values from the oracle's independent C++ samplers: element `elem` of
pco_random_time_prior(elem + 1, key, 0) is the time at (key, elem).

The draws depend on (seed, site of the node, particle, sweep, latent row) alone — not on the data — so weights_program
computes them first and then places atoms and observations that make every case occur:
  (i)   v equals no observed value and no atom                 -> c = -log m_d exactly;
  (ii)  v equals an observed value that is no atom of the key  -> those entries move by log1p(-p) - log p + log n;
  (iii) v equals one of the key's atoms and the row has a missing observation -> the missing entries move by +1000 each
        (reachable: an atom that does not match time_prior.jl:10's pattern — the sampler does not pad its minutes — has
        prior mass 0, so a key whose atoms are all of that kind still proposes its dummy with probability 1);
  (p0)  a retained particle holding a drawn time.

Closed forms of one row's update against frozen tables (kernel): as latent_dummy_program's, over the 1440 times."""
import math

import numpy as np

import posterior_exact as pe

lit = pe.lit
SEED = 4242
# ka: atoms the time pattern rejects (and a missing observation per row); kb: pattern atoms; kc: none — its rows are observed
# as missing alone (maybe_swap.jl:27 divides by the number of options)
KEYS = ["ka", "kb", "kc"]
SRCS = ["s0", "s1", "s2", "s3", "s4"]


def render(h, m, am):
    return f"{h}:{m} {'a.m.' if am else 'p.m.'}"


ALL_TIMES = [render(h, m, am) for h in range(1, 13) for m in range(1, 61) for am in (1, 0)]  # what the sampler can return


def trip_program(trips, rows, dep_atoms=None, arr_atoms=None, label_atoms=None, label_len=None, name_atoms=None,
                 name_len=None, extra=None, seed=0):
    """trips: [{'key': str, 'dep': str, ...}] current values of the Trip rows (row id = position); rows: [dict(trip=, src=,
    dep=, arr=, label=, name=)] observations (None / absent = missing).  extra: {attr: [strings]} current values that are
    neither atoms nor the placeholder (values drawn earlier)."""
    from pclean_amd.model import (AddTypos, IndexedProbParameter, LoweredModel, MaybeSwap, Model, ProbLookup, Query,
                                  StringPrior, TimePrior)
    from pclean_amd.trace import Trace
    timed = dep_atoms is not None
    m = Model()
    if timed:
        s = m.add_class("Src")
        s.choice("name", StringPrior(1, 8, SRCS))
    t = m.add_class("Trip")
    with t.block():
        t.choice("key", StringPrior(1, 8, KEYS))
    attrs = []
    if timed:
        t.choice("dep", TimePrior(dep_atoms, "key"))
        attrs.append("dep")
    if arr_atoms is not None:
        t.choice("arr", TimePrior(arr_atoms, "key"))
        attrs.append("arr")
    if label_atoms is not None:
        t.choice("label", StringPrior(1, label_len, label_atoms))
        attrs.append("label")
    if name_atoms is not None:
        t.choice("name", StringPrior(1, name_len, name_atoms, keyed_by="key"))
        attrs.append("name")
    o = m.add_class("Obs")
    bind = {"Key": "trip.key"}
    if timed:
        o.param("error_probs", IndexedProbParameter(10.0, 50.0))
    with o.block():
        o.fk("trip", "Trip")
        if label_atoms is not None:
            o.choice("label_obs", AddTypos("trip.label"))
            bind["Label"] = ("trip.label", "label_obs")
        if name_atoms is not None:
            o.choice("name_obs", AddTypos("trip.name"))
            bind["Name"] = ("trip.name", "name_obs")
    if timed:
        o.fk("src", "Src")
        bind["Src"] = "src.name"
        o.julia("error_prob", ProbLookup("error_probs", lambda src, key: src), ["src.name", "trip.key"])
        with o.block():
            o.choice("dep_obs", MaybeSwap("trip.dep", dep_atoms, "trip.key", "error_prob"))
            bind["Dep"] = ("trip.dep", "dep_obs")
            if arr_atoms is not None:
                o.choice("arr_obs", MaybeSwap("trip.arr", arr_atoms, "trip.key", "error_prob"))
                bind["Arr"] = ("trip.arr", "arr_obs")
    q = Query(m, "Obs", bind)
    col_of = {"dep": "Dep", "arr": "Arr", "label": "Label", "name": "Name"}
    dirty = {"Key": [trips[r["trip"]]["key"] for r in rows]}
    if timed:
        dirty["Src"] = [r["src"] for r in rows]
    for a in attrs:
        dirty[col_of[a]] = [r.get(a) for r in rows]
    lw = LoweredModel(m, q, dirty, None, {("Trip", a): list(dict.fromkeys(v)) for a, v in (extra or {}).items()})
    obs = lw.encode_observations(dirty)
    tr = Trace(lw, len(rows), seed)
    S = dict(model=m, query=q, dirty=dirty, lw=lw, obs=obs, trace=tr, attrs=attrs, rows=rows, trips=trips, col_of=col_of,
             timed=timed)
    if timed:
        for k, name in enumerate(SRCS):
            vals = np.zeros(len(lw.layout["Src"]), dtype=np.int32)
            vals[lw.colidx["Src"]["name"]] = lw.latent_dom[("Src", "name")].index_of(name)
            assert tr.insert_row("Src", vals) == k
    for k, lat in enumerate(trips):
        vals = np.zeros(len(lw.layout["Trip"]), dtype=np.int32)
        vals[lw.colidx["Trip"]["key"]] = lw.latent_dom[("Trip", "key")].index_of(lat["key"])
        for a in attrs:
            vals[lw.colidx["Trip"][a]] = value_id(S, a, lat["key"], lat[a])
        assert tr.insert_row("Trip", vals) == k
    for bi, blk in enumerate(lw.blocks):
        if blk.get("score"):
            tr.cur[bi] = 0
            continue
        cname = blk["root_class"]
        tab = tr.tables[cname]
        for i, r in enumerate(rows):
            ref = r["trip"] if cname == "Trip" else SRCS.index(r["src"])
            tr.cur[bi, i] = ref
            tab.counts[ref] += 1
    return S


def dist_of(S, attr):
    return S["model"].classes["Trip"].attr(attr).dist


def atoms_of(S, attr, key):
    d = dist_of(S, attr)
    return list(d.atoms[key]) if getattr(d, "keyed_by", None) else list(d.atoms)


def value_id(S, attr, key, s):
    """latent-domain id of string s held by a row of `key`: an option of the key (or the placeholder) by its index, anything
    else — a string listed under another key among it — as a drawn value"""
    dom = S["lw"].latent_dom[("Trip", attr)]
    if s in atoms_of(S, attr, key) or s == dist_of(S, attr).dummy_value() or s not in dom.extra:
        return dom.index_of(s)  # (the last: an atom of another key, held under its own id)
    return dom.extra[s]


def is_time(S, attr):
    from pclean_amd.model import TimePrior
    return isinstance(dist_of(S, attr), TimePrior)


def dummy_mass_log(S, attr, key):
    """log m_d of the proposal of Trip.attr for a row of `key` (oracle/literal.py)"""
    a = S["model"].classes["Trip"].attr(attr)
    if getattr(a.dist, "keyed_by", None):
        options, lps = lit.own_choice_proposal(None, "Trip", a, {"key": key})
        assert options[-1] == a.dist.dummy_value()
        return lps[-1]
    options, lps, dummy = lit.discrete_proposal(None, "Trip", a)
    assert options[-1] is None
    return lps[-1]


def evidence_of(S, attr, trip):
    """[(observed string or None, error probability or None, multiplicity)] of the rows referring to `trip`: the distinct
    (probability-table entry, observed value) pairs in ascending order of (entry, observed id) — missing first"""
    col = S["dirty"][S["col_of"][attr]]
    tr = S["trace"]
    timed = is_time(S, attr)
    pidx = tr.prob_index() if timed else None
    ptab = tr.prob_table() if timed else None
    cnt = {}
    for i, r in enumerate(S["rows"]):
        if r["trip"] != trip:
            continue
        if not timed and col[i] is None:
            continue  # (AddTypos: a missing observation adds nothing)
        k = (int(pidx[i]) if timed else -1, col[i])
        cnt[k] = cnt.get(k, 0) + 1
    return [(o, (float(ptab[p]) if timed else None), n)
            for (p, o), n in sorted(cnt.items(), key=lambda kv: (kv[0][0], "" if kv[0][1] is None else kv[0][1]))]


def density(S, attr, key, o, prob, v, restricted=False, options=None, n_options=None):
    """log density of observed o given the value v of Trip.attr of a row of `key`; options / n_options: what a MISREADING
    would use in their place (test_latent_time_cpu.py)"""
    if is_time(S, attr):
        opts = atoms_of(S, attr, key) if options is None else options
        if o is None:
            return 0.0 if v in opts else -1000.0
        if n_options is not None:  # (membership and count read from different places)
            return math.log1p(-prob) if v == o else math.log(prob) - math.log(n_options)
        return lit.maybe_swap_logpdf(o, v, opts, prob)
    return lit.add_typos_logpdf(o, v, None, restricted)


def slot_terms(S, attr, trip, v, restricted=False):
    """the summands of c(v) for (trip, attr): [-log m_d(key)] + [cnt l(o | v), -cnt l(o | placeholder)] per distinct
    (probability, observed value), float64 — the tolerance counts them"""
    key = S["trips"][trip]["key"]
    ph = dist_of(S, attr).dummy_value()
    terms = [-dummy_mass_log(S, attr, key)]
    for o, prob, n in evidence_of(S, attr, trip):
        terms.append(n * density(S, attr, key, o, prob, v, restricted))
        terms.append(-n * density(S, attr, key, o, prob, ph, restricted))
    return terms


def slot_correction(S, attr, trip, v, restricted=False):
    """(c(v), tolerance 4 k 2^-53 sum |summand|) — the float64 restatement of one slot's correction"""
    terms = slot_terms(S, attr, trip, v, restricted)
    return math.fsum(terms), 4.0 * len(terms) * 2.0 ** -53 * math.fsum(abs(x) for x in terms)


def slot_case(S, attr, trip, v):
    """which of the cases of a drawn time the slot (trip, attr, v) is: a set out of 'i', 'ii', 'iii-missing', 'iii'"""
    key = S["trips"][trip]["key"]
    atoms = atoms_of(S, attr, key)
    ev = evidence_of(S, attr, trip)
    out = set()
    if v in atoms:
        out.add("iii-missing" if any(o is None for o, _, _ in ev) else "iii")
    elif any(o == v for o, _, _ in ev):
        out.add("ii")
    else:
        out.add("i")
    return out


# ---- the drawn values -------------------------------------------------------------------------------------------------
def plan_node(lw, attr):
    """(block id of Trip's latent plan, node of attribute attr in it)"""
    pl = lw.latent_plans["Trip"]
    return pl["block_id"], pl["roots"][pl["root_attr"].index(attr)]


def time_at(oracle, key, elem):
    """random(TimePrior) at (key, elem), stream 0, by the oracle's sampler"""
    h, m, am = oracle.RandomOracle().random_time_prior(int(elem) + 1, int(key), 0)[int(elem)]
    return render(int(h), int(m), int(am))


def drawn_values(oracle, S, attr, seed, particles, sweep_idx, keys):
    """the value each (particle, latent row) draws for a chosen dummy of Trip.attr in sweep sweep_idx"""
    from pclean_amd import sampling
    block_id, node = plan_node(S["lw"], attr)
    ks = [sampling.dummy_seed(seed, (block_id << 16) | node, int(p), sweep_idx) for p in particles]
    if is_time(S, attr):
        return [time_at(oracle, k, e) for k, e in zip(ks, keys)]
    d = dist_of(S, attr)
    if not ks:
        return []
    return sampling.random_string_prior_at(oracle.RandomOracle(), ks, [int(k) for k in keys], d.min_len, d.max_len)


# ---- the weights program (the GPU test's shapes) -----------------------------------------------------------------------
PARTICLES = [(2, True), (2, False), (64, False)]  # (P, MH) of sweeps 0, 1, 2
W_ENTRIES = {2: 1, 3: 63, 4: 64, 5: 65, 6: 130}   # kb rows -> aggregated evidence entries (the lanes stride over them by 64)
W_KA_ROWS = [7, 8, 9, 10]                         # ka rows: a missing observation each, atoms the pattern rejects
W_HELD = {11: ("kb", "4:44 p.m."), 12: ("ka", "5:55 a.m."), 13: ("kb", "6:7 p.m."), 14: ("ka", "8:8 a.m.")}  # retained drawn times
W_EXPLAINED = range(15, 21)                       # kb rows observed as one of their atoms: no dummy is drawn
W_LABEL_ATOMS = ["qqqq"]
W_LABEL_LEN = 4
W_N_TRIPS = 21
W_KB_FIXED = ["10:10 a.m.", "11:45 p.m."]
W_MIN_CASE = 8


def _pool_times(exclude, n):
    """n times the pattern accepts that are none of `exclude`, in a fixed order"""
    out = []
    for s in ALL_TIMES:
        if lit._TIME_RE.match(s) and s not in exclude:
            out.append(s)
            if len(out) == n:
                return out
    raise AssertionError("not enough times")


def _skeleton():
    """the weights program without observations: what fixes the plan's block and node ids"""
    trips = [{"key": "kc", "dep": "**:** p.m.", "label": "qqqq"}]
    return trip_program(trips, [dict(trip=0, src="s0")], {k: [] for k in KEYS}, label_atoms=W_LABEL_ATOMS,
                        label_len=W_LABEL_LEN)


def weights_program(oracle):
    """Trip rows of every shape the time kernel tells apart — no referring row (0), missing observations only (1), 1 / 63 /
    64 / 65 / 130 aggregated entries with multiplicities above 1 and five error probabilities, three keys (none, 1 + the
    drawn ones, pattern-rejected atoms), rows that hold drawn times, rows whose atoms explain them — with an unkeyed
    StringPrior choice (label) served in the same call.  Returns (S, draws) with draws[(sweep, row, particle)] = the time."""
    sk = _skeleton()
    ph = dist_of(sk, "dep").dummy_value()
    draws = {}
    for sweep, (P, mh) in enumerate(PARTICLES):
        ps = [p for t in range(W_N_TRIPS) for p in range(1, P)]
        ts = [t for t in range(W_N_TRIPS) for p in range(1, P)]
        for t, p, v in zip(ts, ps, drawn_values(oracle, sk, "dep", SEED, ps, sweep, ts)):
            draws[(sweep, t, p)] = v
    big = len(PARTICLES) - 1  # the P = 64 sweep: where the cases are planted
    # (iii-missing): ka's atoms = drawn times of the ka rows that the pattern rejects (minutes below 10)
    ka_atoms = []
    for t in W_KA_ROWS + [12]:
        for p in range(1, 64):
            v = draws[(big, t, p)]
            if not lit._TIME_RE.match(v) and v not in ka_atoms and len(ka_atoms) < 24:
                ka_atoms.append(v)
    # (iii): kb's atoms = two fixed ones + drawn times of kb rows that the pattern accepts
    kb_atoms = list(W_KB_FIXED)
    for t in (3, 4):
        for p in range(1, 6):
            v = draws[(big, t, p)]
            if lit._TIME_RE.match(v) and v not in kb_atoms:
                kb_atoms.append(v)
    atoms = {"ka": ka_atoms, "kb": kb_atoms, "kc": []}
    held = [v for _, v in W_HELD.values()]
    assert not (set(held) & set(ka_atoms + kb_atoms))
    trips = []
    for t in range(W_N_TRIPS):
        key = "kc" if t < 2 else ("ka" if t in W_KA_ROWS else "kb")
        dep = ph
        if t in W_HELD:
            key, dep = W_HELD[t]
        if t in W_EXPLAINED:
            dep = W_KB_FIXED[0]
        trips.append({"key": key, "dep": dep, "label": "qqqq"})
    rows = [dict(trip=1, src="s0"), dict(trip=1, src="s0"), dict(trip=1, src="s1", label="zz")]
    # (ii): observed values that are drawn times of the row's own particles (no atoms), the rest from a pool
    for t, n in W_ENTRIES.items():
        mine = [draws[(big, t, p)] for p in range(6, 6 + min(n, 30))]
        mine += [draws[(s, t, 1)] for s in range(big)]
        mine = [v for v in dict.fromkeys(mine) if v not in kb_atoms]
        pool = _pool_times(set(kb_atoms) | set(mine) | set(held), 80)
        values = (mine + pool)
        made = set()
        j = 0
        while len(made) < n:
            src = SRCS[j % len(SRCS)]
            o = values[(j // len(SRCS)) % len(values)] if n > 1 else values[0]
            if (src, o) not in made:
                made.add((src, o))
                for _ in range(1 + (j % 7 == 0) + (j % 31 == 0)):  # multiplicities 1 .. 3
                    rows.append(dict(trip=t, src=src, dep=o, label=("hat" if j % 9 == 0 else None)))
            j += 1
    for t in W_KA_ROWS:
        rows.append(dict(trip=t, src="s0"))                                   # the missing observation
        rows.append(dict(trip=t, src="s1"))
        rows.append(dict(trip=t, src="s2", dep=draws[(big, t, 40)], label="the"))   # (ii) under ka
        rows.append(dict(trip=t, src="s3", dep="2:22 p.m."))
    for t, (key, v) in W_HELD.items():
        rows += [dict(trip=t, src="s0", dep=v), dict(trip=t, src="s0", dep=v), dict(trip=t, src="s1", dep=v),
                 dict(trip=t, src="s2", dep="1:11 a.m.")]
        if key != "kb":
            rows.append(dict(trip=t, src="s4"))
    for t in W_EXPLAINED:
        rows += [dict(trip=t, src="s0", dep=W_KB_FIXED[0], label="qqqq")] * 3
    S = trip_program(trips, rows, atoms, label_atoms=W_LABEL_ATOMS, label_len=W_LABEL_LEN, extra={"dep": held})
    assert plan_node(S["lw"], "dep") == plan_node(sk["lw"], "dep"), "the draws were computed for another node"
    for t, n in W_ENTRIES.items():
        assert len(evidence_of(S, "dep", t)) == n, (t, len(evidence_of(S, "dep", t)), n)
    return S, draws


def keyed_string_program():
    """the keyed-StringPrior twin: Trip.name ~ StringPrior(1, 5, atoms by key, keyed_by="key") observed through AddTypos;
    rows with 0, 1, 63, 64, 65 and 130 distinct observed names, three keys with different atom counts (one with none), a
    string listed under ANOTHER key held by a row (no option of its own key: the retained particle stands for the dummy)"""
    rng = np.random.default_rng(3)
    atoms = {"ka": ["qqqqq", "zzzzz"], "kb": ["xxxxx"], "kc": []}
    letters = "etaoinshr dlu"
    words = ["abc", "hat", "hte", "no", "u", "t"]
    while len(words) < 130:
        w = "".join(letters[int(j)] for j in rng.integers(0, len(letters), size=int(rng.integers(1, 9))))
        if w not in words:
            words.append(w)
    trips = [{"key": "kc", "name": "*" * 3}, {"key": "ka", "name": "*" * 3}]
    rows = []
    for n, key in ((1, "kb"), (63, "ka"), (64, "kb"), (65, "kc"), (130, "ka")):
        t = len(trips)
        trips.append({"key": key, "name": "*" * 3})
        for j, w in enumerate(words[:n]):
            rows += [dict(trip=t, name=w)] * (1 + (j % 7 == 0))
    held = {len(trips): ("ka", "ca"), len(trips) + 1: ("kb", "qqqqq"), len(trips) + 2: ("kc", "the")}
    for t, (key, v) in held.items():
        trips.append({"key": key, "name": v})
        rows += [dict(trip=t, name="abc"), dict(trip=t, name="abc"), dict(trip=t, name=v), dict(trip=t, name=None)]
    for key in ("ka", "kb"):  # rows their atoms explain
        for _ in range(3):
            t = len(trips)
            trips.append({"key": key, "name": atoms[key][0]})
            rows += [dict(trip=t, name=atoms[key][0])] * 3
    rows.append(dict(trip=1, name=None))
    S = trip_program(trips, rows, name_atoms=atoms, name_len=5, extra={"name": ["ca", "the"]})
    S["held"] = held
    return S


# ---- closed forms over the 1440 times ----------------------------------------------------------------------------------
def proposal(atoms, ev):
    """the enumerated proposal of a TimePrior choice with the key's `atoms` whose evidence is ev = [(observed or None, prob,
    count)]: ({atom: q}, q(dummy), c) with c(v) the log-weight of a particle that drew (or holds) the time v"""
    ph = "**:** p.m."

    def lik(v):
        return math.fsum(n * lit.maybe_swap_logpdf(o, v, atoms, p) for o, p, n in ev)

    lps = [(-math.log(1440.0) if lit._TIME_RE.match(a) else -math.inf) for a in atoms]
    log_md = math.log1p(-math.exp(lit.logsumexp(lps)))
    sc = {a: lp + lik(a) for a, lp in zip(atoms, lps) if lp > -math.inf}
    sc[None] = log_md + lik(ph)
    q = pe.normalise(sc)
    lik_ph = lik(ph)
    return {a: q.get(a, 0.0) for a in atoms}, q.get(None, 0.0), (lambda v: -log_md + lik(v) - lik_ph)


def kernel(atoms, ev, s, mh, corrected=True):
    """{value: probability} after one update (P = 2, MH or PG) of a row holding s — an atom or a drawn time; corrected=False:
    every weight equal (the sweeps without the flag)"""
    qa, qd, c = proposal(atoms, ev)
    fresh = [(a, p, 0.0) for a, p in qa.items() if p > 0]
    if qd > 0:
        fresh += [(v, qd / len(ALL_TIMES), c(v)) for v in ALL_TIMES]  # (a drawn time equal to an atom IS that atom)
    c0 = c(s) if (corrected and s not in atoms) else 0.0
    out, moved = {}, []
    for x, px, c1 in fresh:
        if not corrected:
            c1 = 0.0
        mx = max(c0, c1)
        w0, w1 = math.exp(c0 - mx), math.exp(c1 - mx)
        W0, W1 = w0 / (w0 + w1), w1 / (w0 + w1)
        a = min(1.0, W1 / (1e-10 + W0)) if mh else W1
        out[x] = out.get(x, 0.0) + px * a
        moved.append(px * a)
    out[s] = out.get(s, 0.0) + (1.0 - math.fsum(moved))
    return {k: v for k, v in out.items() if v > 0}


def simulate(atoms, ev, s, mh, n, rng, corrected=True):
    """n updates by the MECHANISM (propose an option, draw hour, minute and half of the day, weigh, accept / pick)"""
    qa, qd, c = proposal(atoms, ev)
    opts = list(qa) + [None]
    pr = np.array([qa[a] for a in qa] + [qd])
    pr = pr / pr.sum()
    c0 = c(s) if (corrected and s not in atoms) else 0.0
    picks = rng.choice(len(opts), size=n, p=pr)
    hs, ms, ams, u = rng.integers(1, 13, size=n), rng.integers(1, 61, size=n), rng.integers(0, 2, size=n), rng.random(n)
    memo, out = {}, {}
    for i in range(n):
        x, c1 = opts[picks[i]], 0.0
        if x is None:
            x = render(int(hs[i]), int(ms[i]), int(ams[i]))
            if corrected:
                if x not in memo:
                    memo[x] = c(x)
                c1 = memo[x]
        mx = max(c0, c1)
        w0, w1 = math.exp(c0 - mx), math.exp(c1 - mx)
        W0, W1 = w0 / (w0 + w1), w1 / (w0 + w1)
        a = min(1.0, W1 / (1e-10 + W0)) if mh else W1
        got = x if u[i] < a else s
        out[got] = out.get(got, 0) + 1
    return out


# ---- the distribution cases (CPU power test and GPU test share them) --------------------------------------------------
# c(v) differs from -log m_d only where v equals an observed value (or is an atom of a row with a missing observation), and
# it is never negative here: from an ATOM state an MH update accepts every fresh particle with or without the correction.
# What tells the corrected kernel from the uncorrected one: a key with MANY atoms (m_d = 1 - 599 / 1440, so a drawn time
# outweighs an atom by 1 / m_d) — MH from a drawn time, PG from an atom — and a retained drawn time that the row's
# observations repeat (its weight keeps it where the uncorrected sweep moves away at once).
DIST_OBS = [("s0", "7:15 a.m."), ("s0", "7:15 a.m."), ("s1", "7:15 a.m."), ("s2", "9:20 p.m.")]  # no atom explains them
DIST_ATOMS = {"few": ["10:10 a.m.", "3:30 p.m."],
              "many": [render(h, m, 1) for h in range(1, 13) for m in range(10, 60) if render(h, m, 1) != "7:15 a.m."]}
DIST_HELD = "7:15 a.m."           # the frequently observed non-atom value
DIST_DRAWN = "2:2 a.m."           # a drawn time nothing repeats
DIST_ROWS = 256                   # identical Trip rows
DIST_SWEEPS = 40
DIST_CASES = [("MH-drawn-many", True, "many", DIST_DRAWN), ("PG-atom-many", False, "many", "10:10 a.m."),
              ("MH-held-few", True, "few", DIST_HELD), ("PG-held-few", False, "few", DIST_HELD)]


def dist_program(atoms_id, state):
    """DIST_ROWS identical Trip rows of key kb holding `state`, each observed by len(DIST_OBS) rows"""
    atoms = DIST_ATOMS[atoms_id]
    trips = [{"key": "kb", "dep": state} for _ in range(DIST_ROWS)]
    rows = [dict(trip=k, src=s, dep=o) for k in range(DIST_ROWS) for s, o in DIST_OBS]
    extra = {"dep": [state]} if state not in atoms else None
    return trip_program(trips, rows, {"ka": [], "kb": list(atoms), "kc": []}, extra=extra)


def dist_evidence(S):
    return evidence_of(S, "dep", 0)
