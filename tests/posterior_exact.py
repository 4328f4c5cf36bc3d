"""Exact output distributions of the batched sweep, from the LITERAL interpreter (TEST INFRASTRUCTURE, CPU only).

In a batched sweep the latent tables are frozen, so one row's update is a Markov kernel whose output distribution has
a closed form in the row's exact conditional posterior pi.  pi comes from oracle/literal.py (model description +
strings, nothing of the product's lowering, fixed-point arithmetic or Philox streams); the probabilities are formed in
high precision (mpmath when it imports, else math.fsum of shifted exponentials).  The closed forms:

  * no current referent (cur = -1): no retained particle, every particle draws from pi          -> pi
  * PG, current referent s, ONE enumerated block: all weights equal, the chosen particle is
    uniform on 0..P-1                                                                            -> (1/P) d_s + (1 - 1/P) pi
  * MH (P = 2), one block: w0 == w1, accepted with 0.5 / (1e-10 + 0.5)                           -> pi (up to 2e-10)
  * MH (P = 2), two blocks, block 1 depends on block 0's value: proposal q(t) = pi0(t0) pi1(t1 | t0),
    accepted with a(t) = min(1, exp(Z1(t0) - Z1(s0)))                                             -> q a + [t == s] (1 - sum q a)
  * PG, P particles, the same two blocks: nothing is resampled after block 0 (equal weights), particle p ends with the
    weight z(x_p) = exp(Z1(x_p)) of its block-0 value, the final pick is proportional to the weights: pg_two_blocks,
    one one-dimensional integral per distinct block-0 value (E[1 / (c + S_k)] = int exp(-c u) E[exp(-u z)]^k du)

A candidate is a referent key of the block's root table, or ('NEW', value) — a fresh row together with its sampled
own choice (the nested conditional of the new-row branch: the option's prior mass times its likelihood).  Not covered:
resampling that fires inside a sweep (three or more blocks, or prior proposals) together with apply_ancestors_kernel,
which stay pinned to the oracle (tests/particle_exact.py pins the primitive they call); rows that can draw a
ProposalDummyValue (the weight correction changes the kernel): root classes here hold a single ChooseUniformly choice,
which has none; and the hospital workload itself.

draw_program holds AddTypos observations; tab_draw_program the tabulated kind (FormatName, ExpandOnShortVersion) next
to one AddTypos term, whose pi comes from the literal interpreter's densities on the strings.

gof() is the one goodness-of-fit routine: a G-test pooled over rows (rows with identical expected distributions are
summed first), cells with an expected count below 5 merged, p-value from scipy.stats.chi2, and the worst cells named.
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "oracle") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
import literal as lit  # noqa: E402

try:
    import mpmath
    mpmath.mp.dps = 40
except ImportError:  # optional: math.fsum below is exact enough for probabilities of 1e5 draws
    mpmath = None

MH_ACCEPT = 0.5 / (1e-10 + 0.5)  # run_smc!'s min(1, w1 / (1e-10 + w0)) at w0 == w1 = 1/2


def normalise(scores):
    """{candidate: log score} -> {candidate: probability} (zero-probability candidates dropped)."""
    finite = {k: v for k, v in scores.items() if v > -math.inf}
    if not finite:
        raise ValueError("no candidate has positive probability")
    top = max(finite.values())  # (a candidate 745 nats below the best has a probability below the smallest double: dropped
    finite = {k: v for k, v in finite.items() if v > top - 745.0}  # here, as its float(x / z) == 0 was below)
    if mpmath is not None:
        w = {k: mpmath.exp(mpmath.mpf(v)) for k, v in finite.items()}
        z = mpmath.fsum(w.values())
        return {k: float(x / z) for k, x in w.items() if x > 0}
    m = max(finite.values())
    w = {k: math.exp(v - m) for k, v in finite.items()}
    z = math.fsum(w.values())
    return {k: x / z for k, x in w.items() if x > 0}


def log_marginal(scores):
    """log sum exp of the candidates' scores, in high precision."""
    vals = [v for v in scores.values() if v > -math.inf]
    if mpmath is not None:
        return float(mpmath.log(mpmath.fsum(mpmath.exp(mpmath.mpf(v)) for v in vals)))
    m = max(vals)
    return m + math.log(math.fsum(math.exp(v - m) for v in vals))


# ---- exact conditionals -------------------------------------------------------------------------------------------
class RowConditionals:
    """Exact block conditionals of observed rows of a program whose blocks each hold ONE reference slot to a class
    with a single own choice (a ChooseUniformly attribute): scores of every existing row and of every (new row, own
    value) from the literal interpreter, the row's own references removed first (run_smc!, row_inference.jl:115-126).

    S: {lw, trace, query, dirty}; the literal trace is built once (keys = the product's row ids)."""

    def __init__(self, S):
        self.lw, self.tr, self.q, self.dirty = S["lw"], S["trace"], S["query"], S["dirty"]
        self.m = self.lw.model
        self.lt = lit.lit_trace_from(self.lw, self.tr)
        self.ocls = self.m.classes[self.q.cls]
        self.blocks = [list(b) for b in self.ocls.blocks]
        self.fks = [[a for a in b if self.ocls.attr(a).kind == "fk"][0] for b in self.blocks]
        self.own = []
        for fk in self.fks:
            cls = self.m.classes[self.ocls.attr(fk).target]
            (a,) = [a for a in cls.attrs if a.kind != "param"]
            assert a.kind == "choice", "root classes with a single own choice only"
            self.own.append((cls.name, a))
        self._memo = {}

    def observed(self, i):
        return {self.q.obsmap[c]: self.dirty[c][i] for c in self.q.obsmap}

    def _unincorporated(self, i):
        """snapshot for restoring the literal trace after the row's references were dropped"""
        lt = self.lt
        saved = {c: (dict(lt.tables[c]), dict(lt.counts[c])) for c in lt.tables}
        for bi, fk in enumerate(self.fks):
            if self.tr.cur[bi, i] >= 0:
                lt.unrefer(self.ocls.attr(fk).target, int(self.tr.cur[bi, i]))
        return saved

    def _restore(self, saved):
        for c, (t, n) in saved.items():
            self.lt.tables[c], self.lt.counts[c] = t, n

    def _block_scores(self, i, bi, ctx):
        """{key | ('NEW', own value string): log score} of block bi of row i given the earlier blocks' values ctx"""
        bp = lit.BlockProposal(self.lt, self.q, self.blocks[bi], self.observed(i), ctx, restricted=False)
        sc = bp.scores()
        new = sc.pop("NEW")
        cname, a = self.own[bi]
        path = a.name
        terms = [t for t in bp.terms if path in t["paths"]]
        options, lps, dummy = lit.discrete_proposal(self.lt, cname, a)
        assert dummy is None, "rows that can draw a ProposalDummyValue are out of scope"
        own = {o: lp + sum(bp._lik(t, {path: o}) for t in terms) for o, lp in zip(options, lps)}
        z_own = lit.logsumexp(list(own.values()))
        for o, v in own.items():  # the new row's mass split over its own value: nested conditional
            sc[("NEW", o)] = new - z_own + v
        return sc, lit.logsumexp([v for k, v in sc.items() if not isinstance(k, tuple)] + [new])

    def value(self, bi, cand):
        """own value string of a candidate of block bi"""
        if isinstance(cand, tuple):
            return cand[1]
        cname, a = self.own[bi]
        return self.lt.tables[cname][cand][a.name] if cand in self.lt.tables[cname] else None

    def _key(self, i, what):
        """rows with the same observations and the same current referents have the same conditionals"""
        return what, tuple(sorted((k, v) for k, v in self.observed(i).items())), tuple(int(c) for c in self.tr.cur[:, i])

    def block0(self, i):
        """(pi over candidates, log-marginal Z) of the first block of row i"""
        key = self._key(i, 0)
        if key not in self._memo:
            self._memo[key] = self._block0(i)
        return self._memo[key]

    def _block0(self, i, bi=0):
        saved = self._unincorporated(i)
        try:
            sc, z = self._block_scores(i, bi, {})
        finally:
            self._restore(saved)
        return normalise(sc), z

    def block_alone(self, i, bi):
        """(pi, Z) of block bi of row i when the block reads no other block's value (independent blocks)"""
        key = self._key(i, ("alone", bi))
        if key not in self._memo:
            self._memo[key] = self._block0(i, bi)
        return self._memo[key]

    def two_blocks(self, i):
        """pi0, Z0 and, per distinct block-0 value x reachable under pi0 or held by the current referent:
        (pi1(. | x), Z1(x)) — the context of block 1 is the value of block 0 its JuliaNode reads."""
        key = self._key(i, 2)
        if key not in self._memo:
            self._memo[key] = self._two_blocks(i)
        return self._memo[key]

    def _two_blocks(self, i):
        saved = self._unincorporated(i)
        try:
            sc0, z0 = self._block_scores(i, 0, {})
            pi0 = normalise(sc0)
            ctx_path = self._ctx_path()
            xs = {self.value(0, t) for t, p in pi0.items() if p >= 1e-13}  # (two_block_expected's floor)
            cur0 = int(self.tr.cur[0, i])
            if cur0 >= 0:
                xs.add(self._cur_value(0, cur0))
            b1 = {}
            for x in xs:
                sc1, z1 = self._block_scores(i, 1, {ctx_path: x})
                b1[x] = (normalise(sc1), z1)
        finally:
            self._restore(saved)
        return pi0, z0, b1

    def _cur_value(self, bi, key):
        cname, a = self.own[bi]
        return self.lw.latent_dom[(cname, a.name)].string(int(self.tr.tables[cname].cols[self.lw.colidx[cname][a.name], key]))

    def _ctx_path(self):
        (j,) = [a for a in self.ocls.attrs if a.kind == "julia"]
        (p,) = [x for x in j.args if x.split(".", 1)[0] == self.fks[0]]
        return p


# ---- closed-form kernels ------------------------------------------------------------------------------------------
def pg_one_block(pi, s, P):
    """output of one enumerated block under PG with P particles; s = current referent (None: no referent)"""
    if s is None:
        return dict(pi)
    out = {k: (1.0 - 1.0 / P) * v for k, v in pi.items()}
    out[s] = out.get(s, 0.0) + 1.0 / P
    return {k: v for k, v in out.items() if v > 0}


def mh_one_block(pi, s):
    out = {k: MH_ACCEPT * v for k, v in pi.items()}
    out[s] = out.get(s, 0.0) + (1.0 - MH_ACCEPT)
    return out


def mh_two_blocks(pi0, b1, s, value0, invert=False):
    """output over (t0, t1) of MH with two blocks, block 1 given block 0's value: b1[x] = (pi1(. | x), Z1(x)),
    value0(t0) = block-0 value of candidate t0, s = (s0, s1) the current referents.  invert: the acceptance of the
    reversed ratio (a mutation for the power self-test)."""
    z_s = b1[value0(s[0])][1]
    out, acc = {}, []
    for t0, p0 in pi0.items():
        pi1, z1 = b1[value0(t0)]
        d = (z_s - z1) if invert else (z1 - z_s)
        a = 1.0 if d >= 0 else math.exp(d)
        for t1, p1 in pi1.items():
            qa = p0 * p1 * a
            out[(t0, t1)] = qa
            acc.append(qa)
    stay = 1.0 - math.fsum(acc)
    out[s] = out.get(s, 0.0) + stay
    return {k: v for k, v in out.items() if v > 0}


def inv_moment(c, k, mu, z, enumerate_it=False):
    """E[1 / (c + S_k)], S_k the sum of k iid z(X), X ~ mu ({x: mass}, z: {x: weight}): by 1 / a = int_0^inf exp(-a u) du
    the one-dimensional integral int exp(-c u) (sum_x mu(x) exp(-u z(x)))^k du.  enumerate_it: the sum over all k-tuples
    instead (the check of the integral, small k only)."""
    xs = list(mu)
    if enumerate_it:
        import itertools
        tot = mpmath.mpf(0)
        for tup in itertools.product(xs, repeat=k):
            pr = mpmath.mpf(1)
            for x in tup:
                pr *= mu[x]
            tot += pr / (c + mpmath.fsum(z[x] for x in tup))
        return tot
    if k == 0 or len({z[x] for x in xs}) == 1:  # (S_k is the constant k z: nothing to integrate)
        return mpmath.fsum(mu.values()) ** k / (mpmath.mpf(c) + k * mpmath.mpf(z[xs[0]]))
    with mpmath.workdps(25):
        m = [(mpmath.mpf(mu[x]), mpmath.mpf(z[x])) for x in xs]
        c = mpmath.mpf(c)
        return +mpmath.quad(lambda u: mpmath.exp(-c * u) * mpmath.fsum(a * mpmath.exp(-u * b) for a, b in m) ** k,
                            [0, 1, 10, 100, mpmath.inf])


PG_MUTATIONS = ("uniform pick", "retained as a fresh draw", "weights squared", "Z1 at the retained value")


def pg_two_blocks(pi0, b1, s, value0, P, mutation=None, enumerate_it=False):
    """output over (t0, t1) of PG with P particles over two blocks, block 1 given block 0's value (data-driven proposals).
    Every particle carries block 0's log marginal after block 0 and nothing is resampled there; after block 1 particle p
    weighs z(x_p) = exp(Z1(x_p)), x_p its block-0 value.  With q(t) = pi0(t0) pi1(t1 | t0), mu(x) the pi0 mass of the
    candidates holding x, S_k the sum of k iid z(X), X ~ mu, and the retained particle s of weight z_s:

      P(out = t) = (P-1) q(t) z(t0) E[1 / (z_s + z(t0) + S_{P-2})]  +  [t == s] z_s E[1 / (z_s + S_{P-1})]
      s = None (no current referent):  P q(t) z(t0) E[1 / (z(t0) + S_{P-1})]

    z is scaled to a maximum of 1.  mutation: one of PG_MUTATIONS (the power self-test); enumerate_it: see inv_moment."""
    assert mpmath is not None, "the closed form of PG over two blocks needs mpmath"
    assert mutation is None or mutation in PG_MUTATIONS
    mu = {}
    for t0, p0 in pi0.items():
        mu[value0(t0)] = mu.get(value0(t0), 0.0) + p0
    xs = set(mu) | ({value0(s[0])} if s is not None else set())
    top = max(b1[x][1] for x in xs)
    z = {x: mpmath.exp(mpmath.mpf(b1[x][1]) - top) for x in xs}
    if mutation == "weights squared":
        z = {x: v * v for x, v in z.items()}
    if mutation == "retained as a fresh draw":
        s_w = None
    else:
        s_w = s
    if s_w is not None:
        z_s = z[value0(s[0])]
        if mutation == "Z1 at the retained value":
            z = {x: z_s for x in z}
    memo = {}

    def E(c, k):
        if (c, k) not in memo:
            memo[(c, k)] = inv_moment(c, k, mu, z, enumerate_it)
        return memo[(c, k)]

    out = {}
    for t0, p0 in pi0.items():
        x = value0(t0)
        if mutation == "uniform pick":
            f = (P - 1.0) / P if s is not None else 1.0
        elif s_w is not None:
            f = float((P - 1) * z[x] * E(z_s + z[x], P - 2)) if P > 1 else 0.0
        else:
            f = float(P * z[x] * E(z[x], P - 1))
        for t1, p1 in b1[x][0].items():
            out[(t0, t1)] = p0 * p1 * f
    if mutation == "uniform pick":
        if s is not None:
            out[s] = out.get(s, 0.0) + 1.0 / P
    elif s_w is not None:
        out[s] = out.get(s, 0.0) + float(z_s * E(z_s, P - 1))
    return {k: v for k, v in out.items() if v > 0}


# ---- goodness of fit ----------------------------------------------------------------------------------------------
def _merge(exp, obs, min_exp=5.0):
    """cells sorted by expectation; the small ones pooled until the pool reaches min_exp"""
    order = sorted(range(len(exp)), key=lambda j: exp[j])
    cells, pool_e, pool_o, pool_n = [], 0.0, 0, []
    for j in order:
        if exp[j] < min_exp or pool_e and pool_e < min_exp:
            pool_e += exp[j]
            pool_o += obs[j]
            pool_n.append(j)
        else:
            cells.append((exp[j], obs[j], [j]))
    if pool_n:
        if pool_e < min_exp and cells:  # fold the remainder into the smallest full cell
            e, o, js = cells.pop(0)
            pool_e, pool_o, pool_n = pool_e + e, pool_o + o, pool_n + js
        cells.append((pool_e, pool_o, pool_n))
    return cells


def gof(items, n_worst=5):
    """G-test of observed draws against expected distributions, pooled over rows.

    items: [(label, expected {cand: prob}, observed {cand: count})].  Rows with the same expected distribution are
    summed first; each group's G is divided by Williams' correction factor.  A draw of a candidate of probability 0 fails outright (p = 0).  Returns dict(p, G, df, n, worst)
    with worst = [(label, cand, observed, expected)] by standardized residual."""
    from scipy.stats import chi2
    groups = {}
    for label, exp, obs in items:
        sig = tuple(sorted((repr(k), round(v, 13)) for k, v in exp.items()))
        g = groups.get(sig)
        if g is None:
            groups[sig] = g = [label, exp, {}]
        for k, c in obs.items():
            g[2][k] = g[2].get(k, 0) + c
    G, df, n, worst = 0.0, 0, 0, []
    impossible = []
    for label, exp, obs in groups.values():
        tot = sum(obs.values())
        n += tot
        for k, c in obs.items():
            if k not in exp:
                impossible.append((label, k, c, 0.0))
        keys = list(exp)
        e = [tot * exp[k] for k in keys]
        o = [obs.get(k, 0) for k in keys]
        cells = _merge(e, o)
        g = 0.0
        for ce, co, js in cells:
            if co > 0:
                g += 2.0 * co * math.log(co / ce)
            g -= 2.0 * (co - ce)  # (sum o = sum e up to rounding: keeps G exact when some mass was dropped)
            cand = keys[js[0]] if len(js) == 1 else f"{len(js)} merged"
            worst.append(((co - ce) / math.sqrt(ce), label, cand, co, ce))
        k = len(cells)
        if k > 1:  # Williams' correction: G overshoots chi2(k - 1) by about a factor q when cells hold few draws
            q = 1.0 + (sum(tot / ce for ce, _, _ in cells) - 1.0) / (6.0 * tot * (k - 1))
            G += g / q
        df += max(k - 1, 0)
    worst.sort(key=lambda w: -abs(w[0]))
    if impossible:
        return dict(p=0.0, G=math.inf, df=df, n=n, worst=impossible[:n_worst])
    p = float(chi2.sf(G, df)) if df > 0 else 1.0
    return dict(p=p, G=G, df=df, n=n, worst=[w[1:] for w in worst[:n_worst]])


def pooled_mass(expected, n):
    """largest share of a group's expected mass that gof() would put into its pooled cell (expectations below 5) when
    every row of `expected` ([{cand: prob}]) is drawn n times; rows with one expected distribution form one group"""
    groups = {}
    for exp in expected:
        sig = tuple(sorted((repr(k), round(v, 13)) for k, v in exp.items()))
        g = groups.setdefault(sig, [exp, 0])
        g[1] += n
    worst = 0.0
    for exp, tot in groups.values():
        worst = max(worst, sum(v for v in exp.values() if tot * v < 5.0))  # (the cells _merge pools for being small)
    return worst


def describe(res):
    w = "; ".join(f"row {lab} cand {c!r}: {o} drawn, {e:.1f} expected" for lab, c, o, e in res["worst"])
    return f"p = {res['p']:.3g} (G = {res['G']:.1f}, df = {res['df']}, {res['n']} draws); worst cells: {w}"


def tabulate(draws):
    """[per-sweep list of candidates] for one row -> {cand: count}"""
    out = {}
    for d in draws:
        out[d] = out.get(d, 0) + 1
    return out


def logml_bound(n_terms, z):
    """the quantisation bound of include/pclean_detmath.h on a log-sum-exp of n_terms: n 2^-40 + 1e-12 |Z|"""
    return n_terms * 2.0 ** -40 + 1e-12 * abs(z)


# ---- the programs of the draw tests -------------------------------------------------------------------------------
def _words(rng, n, lo=18, hi=25, alphabet="abcdefghijklmnop", taken=()):
    out, seen = [], set(taken)
    while len(out) < n:
        w = "".join(rng.choice(list(alphabet), size=int(rng.integers(lo, hi))))
        if w not in seen:
            seen.add(w)
            out.append(w)
    return out


def _typo(rng, w, alphabet="abcdefghijklmnop"):
    j = int(rng.integers(len(w)))
    c = w[j]
    while c == w[j]:
        c = str(rng.choice(list(alphabet)))
    return w[:j] + c + w[j + 1:]


def draw_program(n_table, seed=0, n_dead=0, two_blocks=False):
    """`A: x ~ ChooseUniformly(words)`, `Obs: a ~ A; y, y2, y3 ~ AddTypos(a.x)` with a latent table of n_table rows (n_dead of
    them dead, below the high-water mark) and observed rows of every posterior shape the sweep's kernels tell apart;
    row kind in S['kind']:
      peaked — the observation equals its entity's far-away word (the "decided" groups of the fast path);
      spread — clusters of five entities one or two edits apart: 3-10 candidates within a few nats;
      tied   — pairs of entities with identical values;
      flat   — a missing observation: the CRP prior over every live row (more than 256 survivors);
      new    — the row is its entity's only reference and observes a word no entity holds: the new-row branch wins;
      filler — single-reference entities observed exactly; the filler words repeat, so the row's own value is held
               by other single-reference entities as well (ties against the new row with that word).
    y2 and y3 repeat y on the peaked, new and filler rows and are missing elsewhere.
    Words are 18-24 letters long, so that the fast path's pre-filter (about ten edits) tells candidates apart.
    two_blocks: a second block `b ~ B; w ~ AddTypos(b.z); v ~ AddTypos(j)` with the JuliaNode j = x + "_" + z reading
    block 0's value (block 1 depends on block 0: the MH closed form of two blocks)."""
    from pclean_amd.model import AddTypos, ChooseUniformly, LoweredModel, Model, Query
    from pclean_amd.trace import Trace
    rng = np.random.default_rng(seed)
    ents, rows = [], []  # ents: word per latent row (None = dead); rows: (kind, entity, observed word | None)

    def ent(w):
        ents.append(w)
        return len(ents) - 1

    far = _words(rng, 30)
    for w in far:
        e = ent(w)
        rows += [("peaked", e, w)] * 3
    used = set(far)
    for _ in range(12):
        (base,) = _words(rng, 1, taken=used)
        cl = [base]
        while len(cl) < 5:
            v = _typo(rng, base)
            if v not in cl and v not in used:
                cl.append(v)
        used.update(cl)
        es = [ent(w) for w in cl]
        for e in es:
            rows += [("spread", e, _typo(rng, base)), ("spread", e, base)]
    for w in _words(rng, 12, taken=used):
        used.add(w)
        e1, e2 = ent(w), ent(w)
        rows += [("tied", e1, _typo(rng, w)), ("tied", e2, w), ("tied", e1, w), ("tied", e2, _typo(rng, w))]
    hub = ent(_words(rng, 1, taken=used)[0])
    used.add(ents[hub])
    rows += [("flat", hub, None)] * 60
    fresh = _words(rng, 24, taken=used)
    used.update(fresh)
    n_dead_at = set(range(len(ents) + 10, len(ents) + 10 + 7 * n_dead, 7)) if n_dead else set()
    pool = _words(rng, 60, taken=used)  # filler entities share their words: few distinct strings, many candidates
    used.update(pool)
    for w in fresh:
        while len(ents) in n_dead_at:
            ents.append(None)
        rows.append(("new", ent(pool[len(ents) % len(pool)]), w))
    n_fill = n_table - len(ents)
    assert n_fill > 0
    for w in (pool[k % len(pool)] for k in range(n_fill)):
        while len(ents) in n_dead_at:
            ents.append(None)
        if len(ents) >= n_table:
            break
        rows.append(("filler", ent(w), w))
    extra = _words(rng, 20, taken=used)
    words = sorted({w for w in ents if w is not None} | set(fresh) | set(extra))
    m = Model()
    a = m.add_class("A")
    a.choice("x", ChooseUniformly(words))
    bwords = None
    if two_blocks:
        bwords = _words(rng, 12, lo=3, hi=5, alphabet="qrstuvwxyz")
        b = m.add_class("B")
        b.choice("z", ChooseUniformly(bwords))
    o = m.add_class("Obs")
    with o.block():
        o.fk("a", "A")
        o.choice("y", AddTypos("a.x"))
        o.choice("y2", AddTypos("a.x"))
        o.choice("y3", AddTypos("a.x"))
    bind = {"Y": ("a.x", "y"), "Y2": ("a.x", "y2"), "Y3": ("a.x", "y3")}
    if two_blocks:
        with o.block():
            o.fk("b", "B")
            o.choice("w", AddTypos("b.z"))
            o.julia("j", lambda x, z: f"{x}_{z}", ["a.x", "b.z"])
            o.choice("v", AddTypos("j"))
        bind.update({"W": ("b.z", "w"), "V": ("j", "v")})
    q = Query(m, "Obs", bind)
    n = len(rows)
    dirty = {"Y": [r[2] for r in rows]}
    # rows whose referent is decided observe it three times (y2, y3): the fast path's pre-filter sums three terms; the
    # other shapes leave y2 and y3 missing
    decided = [r[0] in ("peaked", "new", "filler") for r in rows]
    dirty["Y2"] = [r[2] if d else None for r, d in zip(rows, decided)]
    dirty["Y3"] = list(dirty["Y2"])
    bcur = None
    if two_blocks:  # block 1: B rows with one of 12 short words, three references each; w and v noisy copies
        n_b = 40
        bvals = [bwords[k % len(bwords)] for k in range(n_b)]
        bcur = rng.integers(0, n_b, size=n)
        dirty["W"] = [bvals[k] if i % 3 else _typo(rng, bvals[k], "qrstuvwxyz") for i, k in enumerate(bcur)]
        dirty["V"] = [None if r[2] is None else f"{ents[r[1]]}_{bvals[k]}" for r, k in zip(rows, bcur)]
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    tr = Trace(lw, n, seed)
    dom = lw.latent_dom[("A", "x")]
    t = tr.tables["A"]
    ids = [tr.insert_row("A", np.array([dom.index_of(w if w is not None else words[0])], np.int32)) for w in ents]
    for k, w in enumerate(ents):
        assert ids[k] == k
    for i, r in enumerate(rows):
        tr.cur[0, i] = r[1]
        t.counts[r[1]] += 1
    for k, w in enumerate(ents):
        if w is None:
            tr.delete_row("A", k)
    assert t.n == n_table and int((~t.live[:t.n]).sum()) == len([w for w in ents if w is None])
    if two_blocks:
        bdom, tb = lw.latent_dom[("B", "z")], tr.tables["B"]
        for k in range(n_b):
            assert tr.insert_row("B", np.array([bdom.index_of(bvals[k])], np.int32)) == k
        for i, k in enumerate(bcur):
            tr.cur[1, i] = k
            tb.counts[k] += 1
    return dict(lw=lw, trace=tr, obs=obs, query=q, dirty=dirty, model=m, kind=np.array([r[0] for r in rows]))


# ---- the draw program of the tabulated terms (FormatName, ExpandOnShortVersion) -------------------------------------
TAB_CROWD = ["Jack", "jane", "JILL", "Joan", "john", "Jude", "JENS", "Judy", "Jo", "jUNE"]  # one initial, mixed case
TAB_CROWD_IN_LONGS = ["jane", "Joan", "Jude", "Jo"]  # crowd names that are themselves options (exact strings)
TAB_STAR = "J*"  # the name holding "*": -1000 against a missing name_obs, the initial class against "J."
# every crowd name and TAB_STAR is a short version of this option
TAB_CROWD_LONG = "Jack*JaneJillJoanJohnJudeJensJudyJune"
TAB_CROWD_MORE = ["Jackson", "Joanne", "Johanna", "Judith", "Jensen", "Jolene", "Juliane", "Jeanette"]  # so that n differs


def _insert(rng, w, k, letters="xyzwvq"):
    w = list(w)
    for _ in range(k):
        w.insert(int(rng.integers(0, len(w) + 1)), letters[int(rng.integers(0, len(letters)))])
    return "".join(ch.upper() if rng.random() < 0.3 else ch for ch in w)


def _mixed_names(rng, n, taken):
    """n names of 4-7 letters over a-p in mixed case, no two equal ignoring case, none starting with j or q"""
    out, seen = [], {t.lower() for t in taken}
    while len(out) < n:
        w = "".join(rng.choice(list("abcdefghiklmnop"), size=int(rng.integers(4, 8))))
        if w in seen:
            continue
        seen.add(w)
        out.append(w.capitalize() if len(out) % 3 == 0 else (w.upper() if len(out) % 3 == 1 else w))
    return out


def _swapped(w):
    return w.swapcase()


def _tab_free(kinds):
    """the rows the cases without a current referent free: the flat rows and every third initial row"""
    ini = [i for i, k in enumerate(kinds) if k == "initial"]
    return np.array(sorted(ini[::3] + [i for i, k in enumerate(kinds) if k == "flat"]), dtype=np.int64)


def tab_free_rows(S):
    return _tab_free(list(S["kind"]))


def free_rows(S, rows, blocks=(0,)):
    """cur = -1 on `rows` (initialize_trace's state): the referents lose the reference, none loses its last one"""
    tr = S["trace"]
    for bi in blocks:
        t = tr.tables[S["lw"].blocks[bi]["root_class"]]
        for i in rows:
            t.counts[tr.cur[bi, i]] -= 1
            assert t.counts[tr.cur[bi, i]] >= 1
            tr.cur[bi, i] = -1


def tab_spread_rows(S):
    """the initial rows: about ten candidates of the initial class within a few nats of each other"""
    return np.flatnonzero(S["kind"] == "initial").astype(np.int64)


def tab_draw_program(n_table, seed=0, n_dead=0, as_typos=False, second_block=0):
    """`A: x ~ ChooseUniformly(names)`,
    `Obs: a ~ A; name_obs ~ FormatName(a.x); long_obs ~ ExpandOnShortVersion(a.x, longs); typo ~ AddTypos(a.x)`
    with a latent table of n_table rows (n_dead of them dead, below the high-water mark).  Row kind in S['kind']:
      equal   — name_obs is the entity's name in another case, the other two missing (the name is one of longs: the
                short rule's missing column is 0 for it and -1000 for every name outside longs);
      initial — name_obs is "J." / "j.", long_obs the option every crowd name is a short version of: ten names and
                TAB_STAR in the initial class, weighted by their CRP counts and their own -log(n); typo missing on
                every other row (the spread case);
      long    — long_obs alone: FormatName's missing column separates ordinary names (-5) from TAB_STAR (-1000);
      nolong  — name_obs an initial, long_obs missing: 0 for the crowd names among longs, -1000 for the others;
      flat    — all three missing, 60 rows on one hub entity: the CRP prior over the entities named by an option;
      tied    — pairs of entities with identical names;
      new     — the row is its entity's only reference and observes a name of the domain that no entity holds
                (a single name, two names equal ignoring case, or the initial of five unheld names with different n);
      filler  — single-reference entities observed exactly; the filler names repeat.
    The names domain holds mixed-case names, the ten crowd names, names that are options themselves, TAB_STAR and names
    that are a short version of 1, 2 and 5 or more options.  The EMPTY NAME IS LEFT OUT: the lowering takes it, but the
    AddTypos term on the same reference has no density for an empty clean value (add_typos.jl: NegativeBinomial(0, 0.9)
    and log(0)), so no exact posterior exists for a row that observes typo.  FormatName's empty-name row of T is held
    by the known answers and the restatement agreement of tests/test_tabulated_terms.py instead.
    as_typos: the two tabulated terms declared as AddTypos on the same references (the routing contrast).
    second_block: a second, independent block `b ~ B; w ~ AddTypos(b.z)` with a table of that many rows."""
    from pclean_amd.model import AddTypos, ChooseUniformly, ExpandOnShortVersion, FormatName, LoweredModel, Model, Query
    from pclean_amd.trace import Trace
    rng = np.random.default_rng(seed)
    ents, rows = [], []  # ents: name per latent row (None = dead); rows: (kind, entity, name_obs, long_obs, typo)

    def ent(w):
        ents.append(w)
        return len(ents) - 1

    longs = [TAB_CROWD_LONG] + list(TAB_CROWD_MORE) + list(TAB_CROWD_IN_LONGS)
    taken = set(TAB_CROWD) | {TAB_STAR}
    # ordinary names with 1, 2 or 5 long forms of their own; `own` = names that are options themselves
    plain = _mixed_names(rng, 36, taken)
    taken.update(plain)
    forms = {}
    for k, w in enumerate(plain):
        forms[w] = []
        while len(forms[w]) < (1, 2, 5)[k % 3]:
            f = _insert(rng, w, int(rng.integers(1, 5)))
            if f not in longs:
                forms[w].append(f)
                longs.append(f)
    own = _mixed_names(rng, 10, taken)
    taken.update(own)
    longs += own
    for w in own:
        forms[w] = [w]
    # crowd: every name on 1-3 entities with unequal reference counts, TAB_STAR on one
    crowd_e = {}
    for k, w in enumerate(TAB_CROWD + [TAB_STAR]):
        crowd_e[w] = [ent(w) for _ in range(1 + k % 3)]
    k = 0
    # two initial rows per crowd entity (freeing one leaves the entity alive), a third on some; typo on every other entity's:
    # the rows of an entity share one expected distribution, which gof pools
    for w, es in crowd_e.items():
        for e in es:
            for j in range(2 + (k % 4 == 0)):
                rows.append(("initial", e, "J." if (k + j) % 4 else "j.", TAB_CROWD_LONG, w if k % 2 else None))
            k += 1
    for k in range(20):
        w = TAB_CROWD_IN_LONGS[k % 4]
        e = crowd_e[w][k % len(crowd_e[w])]
        rows.append(("nolong", e, "j." if k % 3 == 0 else "J.", None, w if k % 2 else None))
    for k in range(10):  # long rows of the crowd: every crowd name, -5 - log(n) each, TAB_STAR at -1000
        w = TAB_CROWD[k]
        rows.append(("long", crowd_e[w][0], None, TAB_CROWD_LONG, None))
    eq_e = {w: [ent(w), ent(w)] for w in own[:5]}
    for k in range(20):
        w = (own[:5] + TAB_CROWD_IN_LONGS)[k % 9]
        es = eq_e.get(w) or crowd_e[w]
        rows.append(("equal", es[k % len(es)], _swapped(w), None, None))
    for k, w in enumerate(plain[:12]):  # long rows of ordinary names
        e = ent(w)
        rows += [("long", e, None, forms[w][j % len(forms[w])], None) for j in range(2)]
    for k, w in enumerate(plain[12:18]):
        e1, e2 = ent(w), ent(w)
        f = forms[w]
        rows += [("tied", e1, None, f[0], _typo(rng, w)), ("tied", e2, w.upper(), f[-1], w),
                 ("tied", e1, w[0] + ".", f[0], None), ("tied", e2, w.lower(), f[-1], _typo(rng, w))]
    hub = ent(own[5])
    rows += [("flat", hub, None, None, None)] * 60
    rows += [("equal", hub, _swapped(own[5]), None, None)] * 2  # (the hub outlives its flat rows being freed)
    # names no entity holds: ten single ones, two pairs equal ignoring case, five with one initial
    fresh = _mixed_names(rng, 10, taken)
    taken.update(fresh)
    for k, w in enumerate(fresh):
        forms[w] = [_insert(rng, w, 2) for _ in range(1 + k % 2)]
        longs += forms[w]
    pairs = [("Quinn", "QUINN"), ("quade", "Quade")]
    for a_, b_ in pairs:
        forms[a_] = forms[b_] = [a_ + "xy"]
        longs.append(a_ + "xy")
    q_names = ["Quill", "quint", "QUIRE", "Quoin", "Quota"]
    q_long = "QuillQuintQuireQuoinQuota"
    longs += [q_long, "Quillon", "Quintet", "Quintal", "Quotas"]
    pool = plain[18:] + _mixed_names(rng, 110, taken)  # filler names: about eight entities each at 1090 rows
    taken.update(pool)
    for w in pool:
        if w not in forms:
            forms[w] = [_insert(rng, w, 2)]
            longs += forms[w]
    assert len(set(longs)) == len(longs)
    n_dead_at = set(range(len(ents) + 10, len(ents) + 10 + 7 * n_dead, 7)) if n_dead else set()
    new_obs = ([(_swapped(w), forms[w][0], w if k % 2 else None) for k, w in enumerate(fresh)]
               + [(a_.lower(), forms[a_][0], None) for a_, b_ in pairs] + [(b_, forms[a_][0], None) for a_, b_ in pairs]
               + [("Q." if k % 2 else "q.", q_long, q_names[k % 5] if k >= 5 else None) for k in range(10)])
    assert len(new_obs) == 24
    for name_obs, long_obs, typo in new_obs:
        while len(ents) in n_dead_at:
            ents.append(None)
        w = pool[len(ents) % len(pool)]
        rows.append(("new", ent(w), name_obs, long_obs, typo))
    assert n_table - len(ents) > 0
    k = 0
    while len(ents) < n_table:
        if len(ents) in n_dead_at:
            ents.append(None)
            continue
        w = pool[k % len(pool)]
        k += 1
        rows.append(("filler", ent(w), w, forms[w][0], w))
    names = sorted({w for w in ents if w is not None} | set(plain) | set(own) | set(fresh) | set(q_names)
                   | {x for p_ in pairs for x in p_})
    m = Model()
    a = m.add_class("A")
    a.choice("x", ChooseUniformly(names))
    bwords = None
    if second_block:
        bwords = _words(rng, 40, lo=18, hi=25, alphabet="qrstuvwxyz")
        b = m.add_class("B")
        b.choice("z", ChooseUniformly(bwords))
    o = m.add_class("Obs")
    with o.block():
        o.fk("a", "A")
        o.choice("name_obs", AddTypos("a.x") if as_typos else FormatName("a.x"))
        o.choice("long_obs", AddTypos("a.x") if as_typos else ExpandOnShortVersion("a.x", longs))
        o.choice("typo", AddTypos("a.x"))
    bind = {"Name": ("a.x", "name_obs"), "Long": ("a.x", "long_obs"), "Typo": ("a.x", "typo")}
    if second_block:
        with o.block():
            o.fk("b", "B")
            o.choice("w", AddTypos("b.z"))
        bind["W"] = ("b.z", "w")
    q = Query(m, "Obs", bind)
    n = len(rows)
    dirty = {"Name": [r[2] for r in rows], "Long": [r[3] for r in rows], "Typo": [r[4] for r in rows]}
    bcur = None
    if second_block:  # B rows holding one of 40 long words; w the word or the word with one typo
        bvals = [bwords[k % len(bwords)] for k in range(second_block)]
        assert n >= second_block + 70
        bcur = np.arange(n) % second_block  # every B row is referred to; the rows of tab_free_rows share theirs with a
        free = _tab_free([r[0] for r in rows])  # row past the table's size, so that freeing them deletes no B row
        bcur[second_block:second_block + len(free)] = bcur[free]
        dirty["W"] = [bvals[k] if i % 3 else _typo(rng, bvals[k], "qrstuvwxyz") for i, k in enumerate(bcur)]
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    tr = Trace(lw, n, seed)
    dom = lw.latent_dom[("A", "x")]
    t = tr.tables["A"]
    for k, w in enumerate(ents):
        assert tr.insert_row("A", np.array([dom.index_of(w if w is not None else names[0])], np.int32)) == k
    for i, r in enumerate(rows):
        tr.cur[0, i] = r[1]
        t.counts[r[1]] += 1
    for k, w in enumerate(ents):
        if w is None:
            tr.delete_row("A", k)
    assert t.n == n_table and int((~t.live[:t.n]).sum()) == len([w for w in ents if w is None])
    if second_block:
        bdom, tb = lw.latent_dom[("B", "z")], tr.tables["B"]
        for k in range(second_block):
            assert tr.insert_row("B", np.array([bdom.index_of(bvals[k])], np.int32)) == k
        for i, k in enumerate(bcur):
            tr.cur[1, i] = k
        for k in range(second_block):
            tb.counts[k] = int((bcur == k).sum())
        assert (tb.counts[:second_block] > 0).all() and (tb.counts[bcur[free]] >= 2).all()
    return dict(lw=lw, trace=tr, obs=obs, query=q, dirty=dirty, model=m, kind=np.array([r[0] for r in rows]),
                names=names, longs=longs)


# ---- draws of the product's sweeps as candidates ------------------------------------------------------------------
class Encoder:
    """candidate <-> int code of one block: an existing key k is k, a new row with option j of its own choice is
    n_table + j (what the sweep outputs: the referent, PCLEAN_CHOICE_NEW = -1 with the option index in new_rows)."""

    def __init__(self, lw, tr, bi):
        blk = lw.blocks[bi]
        self.cname = blk["root_class"]
        self.n_table = tr.tables[self.cname].n
        (self.attr,) = [c.name for c in lw.layout[self.cname] if c.kind == "val"]
        dom = lw.latent_dom[(self.cname, self.attr)]
        self.opt = {dom.string(int(v)): j for j, v in enumerate(lw.option_values[(self.cname, self.attr)])}
        (self.leaf,) = [k for k in range(1, len(blk["nodes"]))]

    def code(self, cand):
        return self.n_table + self.opt[cand[1]] if isinstance(cand, tuple) else int(cand)

    def codes(self, choice_row, new_rows, n):
        """int codes of one block's outputs over rows 0..n-1 of a sweep"""
        out = np.asarray(choice_row[:n], dtype=np.int64).copy()
        if new_rows is not None:
            rows, vals = new_rows
            sel = rows < n
            out[rows[sel]] = self.n_table + vals[sel, self.leaf]
        assert (out >= 0).all(), "a new referent without its new-row record"
        return out


ALPHA = 1e-4  # a case fails below this pooled p-value (its seeds are fixed: the outcome is deterministic)

# the particle counts of the cases: the edges of the DISPATCH_PMAX buckets of the sweep kernels; (P, MH)
PARTICLES = [(1, False), (2, False), (2, True), (3, False), (8, False), (9, False), (32, False), (33, False), (64, False)]


def check_rows(S, every_filler=4):
    """rows whose draws are tabulated: every row of a shape of interest, every k-th filler row"""
    kind = S["kind"]
    rows = [i for i in range(len(kind)) if kind[i] != "filler" or i % every_filler == 0]
    return np.array(rows, dtype=np.int64)


def one_block_case(eng, S, rc, rows, P, mh, n_sweeps, seed):
    """S sweeps (sweep_idx 0..n_sweeps-1, nothing committed in between) of a one-block program; draws of `rows`
    against the closed form, logml against the exact log-marginal.  Returns (gof result, max |logml - Z| / bound,
    number of new-row records)."""
    from pclean_amd.engine import InferenceConfig
    tr = S["trace"]
    enc = Encoder(S["lw"], tr, 0)
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
    n = tr.cur.shape[1]
    D = np.empty((n_sweeps, len(rows)), dtype=np.int64)
    dev, n_new = 0.0, 0
    exact = [rc.block0(int(i)) for i in rows]
    for s in range(n_sweeps):
        choice, chosen, logml, new_rows = eng.sweep(tr, cfg, seed, s)
        n_new += len(new_rows[0][0]) if 0 in new_rows else 0
        D[s] = enc.codes(choice[0], new_rows.get(0), n)[rows]
        if s == 0:
            for j, i in enumerate(rows):
                z = exact[j][1]
                dev = max(dev, abs(float(logml[i]) - z) / logml_bound(enc.n_table + len(enc.opt) + 1, z))
    items = []
    for j, i in enumerate(rows):
        pi = {enc.code(k): v for k, v in exact[j][0].items()}
        s0 = int(tr.cur[0, i])
        s0 = None if s0 < 0 else s0
        e = mh_one_block(pi, s0) if (mh and s0 is not None) else pg_one_block(pi, s0, P)
        items.append((int(i), e, tabulate(D[:, j].tolist())))
    return gof(items), dev, n_new


def two_block_expected(S, rc, rows, invert=False, floor=1e-13, P=2, mh=True, mutation=None, enumerate_it=False):
    """closed form of MH (mh_two_blocks) or of PG with P particles (pg_two_blocks) over the two blocks of
    draw_program(two_blocks=True) per row, in the encoders' codes (t0 code, t1 code); block-0 candidates below `floor` are
    left out (their mass, < 1e-10 in all, stays put).  A row without current referents (cur = -1) has no retained
    particle.  Rows with the same conditionals and referents share one computation."""
    tr = S["trace"]
    e0, e1 = Encoder(S["lw"], tr, 0), Encoder(S["lw"], tr, 1)
    out, memo = [], {}
    for i in rows:
        key = rc._key(int(i), 2)
        if key not in memo:
            pi0, z0, b1 = rc.two_blocks(int(i))
            pi0 = {k: v for k, v in pi0.items() if v >= floor}
            val = {k: rc.value(0, k) for k in pi0}
            cur = (int(tr.cur[0, i]), int(tr.cur[1, i]))
            assert (cur[0] < 0) == (cur[1] < 0)
            if cur[0] < 0:
                cur = None
            else:
                val[cur[0]] = rc._cur_value(0, cur[0])
            if mh:
                assert cur is not None and P == 2 and mutation is None
                ex = mh_two_blocks(pi0, b1, cur, lambda t: val[t], invert=invert)
            else:
                ex = pg_two_blocks(pi0, b1, cur, lambda t: val[t], P, mutation=mutation, enumerate_it=enumerate_it)
            memo[key] = {(e0.code(t[0]), e1.code(t[1])): v for t, v in ex.items()}
        out.append(memo[key])
    return out


def two_block_case(eng, S, rc, rows, n_sweeps, seed, P=2, mh=True):
    from pclean_amd.engine import InferenceConfig
    tr = S["trace"]
    e0, e1 = Encoder(S["lw"], tr, 0), Encoder(S["lw"], tr, 1)
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
    n = tr.cur.shape[1]
    D0 = np.empty((n_sweeps, len(rows)), dtype=np.int64)
    D1 = np.empty_like(D0)
    for s in range(n_sweeps):
        choice, chosen, logml, new_rows = eng.sweep(tr, cfg, seed, s)
        D0[s] = e0.codes(choice[0], new_rows.get(0), n)[rows]
        D1[s] = e1.codes(choice[1], new_rows.get(1), n)[rows]
    exp = two_block_expected(S, rc, rows, P=P, mh=mh)
    items = [(int(i), exp[j], tabulate(list(zip(D0[:, j].tolist(), D1[:, j].tolist())))) for j, i in enumerate(rows)]
    return gof(items)


# ---- the cases both legs share --------------------------------------------------------------------------------------
S_GPU = 200            # sweeps per case of the device leg (the power self-test samples at this S)
SPREAD_SWEEPS = 2000   # sweeps of the spread-row case: a 0.1-nat shift moves p by ~0.1 p (1 - p), visible only there
SPREAD_P = 2
PROGRAMS = {"generic": dict(n_table=300, seed=0, n_dead=0), "fast": dict(n_table=1090, seed=0, n_dead=5)}
TWO_BLOCK = dict(n_table=1090, seed=1, two_blocks=True)
PROGRAMS_TAB = {"generic": dict(n_table=300, seed=0, n_dead=0), "large": dict(n_table=1090, seed=0, n_dead=5)}
TAB_PARTICLES = [(1, False), (2, False), (2, True), (9, False), (33, False), (64, False)]
TAB_LATENT = [(2, False), (2, True), (9, False)]
TAB_MIXED = dict(PROGRAMS_TAB["large"], second_block=1100)  # block 1's table: 1100 rows, the fast root path


def two_block_rows(S):
    return np.array([i for i, k in enumerate(S["kind"]) if k in ("peaked", "spread", "tied", "new")][::2])


TWO_BLOCK_PG = [3, 9, 33]  # particle counts of the two-block PG cases: one DISPATCH_PMAX bucket each


def two_block_free_rows(S):
    """the rows the case without current referents frees in both blocks: the peaked and spread rows of two_block_rows
    (free_rows checks that their referents keep another reference)"""
    return np.array([i for i in two_block_rows(S) if S["kind"][i] in ("peaked", "spread")], dtype=np.int64)


def near_candidate(pi, s):
    """the most probable existing row other than s among those holding 10%..90% (None when there is none)"""
    near = [k for k, v in pi.items() if k != s and not isinstance(k, tuple) and 0.1 < v < 0.9]
    return max(near, key=lambda c: pi[c]) if near else None


def shift_near(pi, s, nats=0.1):
    """pi with its near candidate's score shifted by `nats` (a mutation for the power self-test)"""
    k = near_candidate(pi, s)
    if k is None:
        return pi
    out = dict(pi)
    out[k] *= math.exp(nats)
    z = sum(out.values())
    return {c: v / z for c, v in out.items()}


def spread_rows(S, rc):
    """rows whose posterior holds a near candidate: the row set of the spread case (SPREAD_SWEEPS draws each)"""
    tr = S["trace"]
    return np.array([i for i in range(tr.cur.shape[1]) if near_candidate(rc.block0(i)[0], int(tr.cur[0, i])) is not None],
                    dtype=np.int64)


# ---- latent rows: the own choice x of class A against its evidence set ----------------------------------------------
def latent_setup(S):
    """(live, ev_off, ev_rows, ev_ctx, excl) of class A for sweep_latent"""
    from pclean_amd.engine import InferenceConfig
    from pclean_amd.inference import build_evidence, latent_current_choices
    live, ev_off, ev_rows, ev_ctx = build_evidence(S["lw"], S["trace"], "A")
    excl = latent_current_choices(S["lw"], S["trace"], "A", live, InferenceConfig(1, 2))
    return live, ev_off, ev_rows, ev_ctx, excl


def latent_exact(S, rc, live, ev_off, ev_rows, items):
    """pi over option indices of x for the latent rows live[items] (LatentProposal: every AddTypos observation of every
    referring row) and the option index of each row's current value"""
    lw, tr = S["lw"], S["trace"]
    enc = Encoder(lw, tr, 0)
    col = lw.colidx["A"]["x"]
    dom = lw.latent_dom[("A", "x")]
    memo, out = {}, []
    for t in items:
        ev = [rc.observed(int(r)) for r in ev_rows[ev_off[t]:ev_off[t + 1]]]
        key = tuple(tuple(sorted(o.items())) for o in ev)
        if key not in memo:
            lp = lit.LatentProposal(rc.lt, rc.q, rc.blocks[0], "", [(o, {}) for o in ev])
            memo[key] = {enc.opt[o]: v for o, v in normalise(lp.leaf_scores("A", "x")).items()}
        cur = enc.opt[dom.string(int(tr.tables["A"].cols[col, live[t]]))]
        out.append((memo[key], cur))
    return out


def latent_case(eng, S, rc, P, mh, n_sweeps, seed, every=3, exact=None):
    """sweep_latent over every live row of A, n_sweeps times (sweep_idx 0..n_sweeps-1): the chosen particle 0 keeps
    the current value, any other draws from pi -> (1/P) d_cur + (1 - 1/P) pi under PG, MH_ACCEPT pi + ... under MH"""
    from pclean_amd.engine import InferenceConfig
    live, ev_off, ev_rows, ev_ctx, excl = latent_setup(S)
    items = np.arange(0, len(live), every)
    if exact is None:  # (a caller with several cases over one frozen trace passes latent_exact's result for `items`)
        exact = latent_exact(S, rc, live, ev_off, ev_rows, items)
    assert len(exact) == len(items)
    root = S["lw"].latent_plans["A"]["roots"][0]
    cfg = InferenceConfig(1, P, use_mh_instead_of_pg=mh)
    D = np.empty((n_sweeps, len(items)), dtype=np.int64)
    for s in range(n_sweeps):
        chosen, vals = eng.sweep_latent(S["trace"], "A", cfg, seed, s, live, ev_off, ev_rows, ev_ctx, excl)
        keep = np.array([c for _, c in exact])
        got = np.where(chosen[items] == 0, keep, vals[items, root])
        assert (got >= 0).all(), "a latent row chose a particle without its draw"
        D[s] = got
    res = []
    for j, t in enumerate(items):
        pi, cur = exact[j]
        e = mh_one_block(pi, cur) if mh else pg_one_block(pi, cur, P)
        res.append((int(t), e, tabulate(D[:, j].tolist())))
    return gof(res)


def mixed_case(eng, S, rc, rows, P, n_sweeps, seed):
    """n_sweeps sweeps of a program with two INDEPENDENT blocks over rows without a current referent in either; one
    G-test per block against the block's own pi.  Returns ([gof of block 0, gof of block 1], max logml deviation)."""
    from pclean_amd.engine import InferenceConfig
    tr = S["trace"]
    encs = [Encoder(S["lw"], tr, bi) for bi in (0, 1)]
    cfg = InferenceConfig(1, P)
    n = tr.cur.shape[1]
    D = np.empty((2, n_sweeps, len(rows)), dtype=np.int64)
    exact = [[rc.block_alone(int(i), bi) for i in rows] for bi in (0, 1)]
    dev = 0.0
    for s in range(n_sweeps):
        choice, chosen, logml, new_rows = eng.sweep(tr, cfg, seed, s)
        for bi in (0, 1):
            D[bi, s] = encs[bi].codes(choice[bi], new_rows.get(bi), n)[rows]
        if s == 0:
            for j, i in enumerate(rows):
                z = exact[0][j][1] + exact[1][j][1]
                n_terms = sum(e.n_table + len(e.opt) + 1 for e in encs)
                dev = max(dev, abs(float(logml[i]) - z) / logml_bound(n_terms, z))
    out = []
    for bi in (0, 1):
        items = [(int(i), {encs[bi].code(k): v for k, v in exact[bi][j][0].items() if v > 0}, tabulate(D[bi, :, j].tolist()))
                 for j, i in enumerate(rows)]
        out.append(gof(items))
    return out, dev
