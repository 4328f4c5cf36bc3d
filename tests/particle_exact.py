"""The particle primitives against an arbitrary-precision restatement (TEST INFRASTRUCTURE, CPU only).

Every sweep ends in fix_weights / fix_pick (csrc/sweep_internal.h), maybe_resample_kernel and final_choice_kernel
(csrc/sweep.hip).  This module restates what they must compute from row_inference.jl:76-105,158-165 and the header
comment of include/pclean_detmath.h, in Python integers and mpmath (40 digits), and imports nothing of the product or of
the C++ oracle: a mistake the two share cannot hide here.  For a weight row w[0..P-1]:

  m = max w, d_p = w_p - m (float64), e_p = exp(d_p) 2^40 exactly, u_p = floor(e_p) (0 for d_p < -28.5 and -inf), U = sum u_p
  wn_p = e_p / sum e, ESS = 1 / sum wn_p^2, lse = m + log(sum e 2^-40)                       (all exact, nothing floored)
  pick(u, R): x = (R U) >> 64 in Python integers, the first p whose cumulative u exceeds x; P - 1 when U == 0
  resampling (ESS < P / 2, strict): ancestor p = pick(u, R_p), R_p at site 0x40000000 | block, particle p; ancestor 0 is
      0 for a retained particle; logml_inc = lse - log P (0.0 and the identity when nothing is resampled)
  final choice: pick(u, R) at site 0x50000000, particle 0; MH with a current referent: particle 1 when
      u01(R) < min(1, (u_1 / U) / (1e-10 + u_0 / U)), R at site 0x50000001, u01(r) = (r >> 11) 2^-53

The random bits R are the implementation's own (pclean_debug_rand64 / pco_rand64; Philox itself is pinned by
tests/test_gpu_tables.py and tests/test_contract.py); everything downstream of them is recomputed here, integer for integer.

Bounds (derived, not measured):
  * pclean_exp is within 1 ulp and an ulp at 2^40 is 2^-12: fixw(d) == floor(e) when e is further than 2^-10 (four
    ulps) from an integer, and within 1 of it otherwise.  d == 0 gives 2^40 and d < -28.5 gives 0 exactly.
  * every u_p is off by less than 1 of a total of at least 2^40, so U and sum u^2 are each off by at most 2 P 2^-40
    relative; ESS_BOUND = 8 P 2^-40 relative covers the quotient.
  * `acc > x` against `acc >= x` in the scan, and `ess < P/2` against `<=`, differ on an event of probability below
    64 * 2^-40 per draw: no sample can tell them apart.  They are told apart by CONSTRUCTED rows: exact ESS ties (k
    particles at the maximum, P - k at -inf, k = P / 2), and boundary_rows(), which reads the implementation's R for a
    row and solves for the weight u_0 at which x == u_0 exactly.

A backend (the device, the oracle, or the mutable sampler of the power self-test) has
  maybe_resample(W, retain_first, seed, sweep, block) -> (anc, inc, ess);  final_choice(W, mh, csmc, seed, sweep) -> (c, tot)
  fixw(d) -> uint64;  rand64(seed, rows, site, particle, sweep) -> uint64;  offset(k): context manager, row offset k
"""
import math

import mpmath
import numpy as np

mpmath.mp.dps = 40
mpf = mpmath.mpf

FIX_BITS = 40
ONE = 1 << FIX_BITS
FLOOR = -28.5                 # pclean_fixw: exp(-28.5) 2^40 < 1
NEAR = mpf(2) ** -10          # four ulps of a double at 2^40
# include/pclean_hip.h: PCLEAN_SITE_RESAMPLE(block), PCLEAN_SITE_FINAL, PCLEAN_SITE_MH
SITE_FINAL, SITE_MH = 0x50000000, 0x50000001


def site_resample(block):
    return 0x40000000 | block


P_EDGES = [1, 2, 3, 8, 9, 32, 33, 64]  # both edges of every DISPATCH_PMAX bucket (2 / 8 / 32 / 64)
N_BIG = 4099                            # rows of the large calls: more than one block of 256 threads, no multiple of it
NEG = -math.inf


def ess_bound(P):
    return 8.0 * P * 2.0 ** -FIX_BITS


# ---- the exact quantities of one weight row ---------------------------------------------------------------------------
class Exact:
    """m, d (float64), e (mpf), u (int), U, wn (mpf), ess (mpf), lse (mpf | -inf), near (e within 2^-10 of an integer)"""

    def __init__(self, w):
        w = [float(x) for x in w]
        self.P = P = len(w)
        self.m = m = max(w)
        if m == NEG:
            self.d, self.e, self.u, self.U = [NEG] * P, [mpf(0)] * P, [0] * P, 0
            self.wn, self.ess, self.lse, self.near = [mpf(0)] * P, mpf(0), NEG, [False] * P
            return
        self.d = [x - m for x in w]  # float64 subtraction, as the kernels form it
        self.e = [mpf(0) if x == NEG else mpmath.exp(mpf(x)) * ONE for x in self.d]
        self.u = [0 if x < FLOOR else int(mpmath.floor(v)) for x, v in zip(self.d, self.e)]
        self.U = sum(self.u)
        z = mpmath.fsum(self.e)
        self.wn = [v / z for v in self.e]
        self.ess = 1 / mpmath.fsum(v * v for v in self.wn)
        self.lse = mpf(m) + mpmath.log(z / ONE)
        # d == 0 and d < -28.5 are exact by construction of pclean_fixw: not members of the "near an integer" class
        self.near = [x != 0.0 and x >= FLOOR and abs(v - mpmath.nint(v)) <= NEAR for x, v in zip(self.d, self.e)]

    def tie(self):
        """an ESS tie that is exact in fixed point: P / 2 particles at the maximum (u = 2^40 exactly), the others with
        e < 0.99 (u = 0 whatever the last bit of pclean_exp) -> U^2 / sum u^2 == P / 2 in integers, and `<` is strict"""
        return (self.U > 0 and 2 * sum(1 for d in self.d if d == 0.0) == self.P
                and all(d == 0.0 or v < 0.99 for d, v in zip(self.d, self.e)))

    def resamples(self):
        return self.ess < mpf(self.P) / 2

    def decided(self):
        """the exact ESS is further from P / 2 than the bound on the fixed-point ESS"""
        return abs(self.ess - mpf(self.P) / 2) > ess_bound(self.P) * self.ess or self.U == 0


_memo = {}


def exact(w):
    w = np.ascontiguousarray(w, dtype=np.float64)
    key = w.tobytes()
    if key not in _memo:
        _memo[key] = Exact(w)
    return _memo[key]


def pick(u, R):
    """fix_pick: x = floor(R U / 2^64), the first p with u_0 + .. + u_p > x"""
    U = sum(u)
    if U == 0:
        return len(u) - 1
    x = (int(R) * U) >> 64
    acc = 0
    for p, v in enumerate(u):
        acc += v
        if acc > x:
            return p
    raise AssertionError("x < U: some cumulative weight exceeds it")


def u01(r):
    return (int(r) >> 11) * 2.0 ** -53


def mh_pick(u, R):
    """row_inference.jl:162 on the fixed-point weights, in float64 as written there; total weight 0 keeps particle 0
    (0 / 0 compares false)"""
    U = sum(u)
    if U == 0:
        return 0
    w0, w1 = u[0] / U, u[1] / U
    return 1 if u01(R) < min(1.0, w1 / (1e-10 + w0)) else 0


def pick_all(u, R):
    """pick() over a matrix: u int64 [n, P], R uint64 [n, K] -> int32 [n, K]; the 128-bit product in Python integers"""
    u = np.asarray(u, dtype=np.int64)
    n, P = u.shape
    cum = np.cumsum(u, axis=1)
    U = cum[:, -1]
    X = ((np.asarray(R).astype(object) * U.astype(object)[:, None]) >> 64).astype(np.int64)
    out = (cum[:, None, :] > X[:, :, None]).argmax(axis=2).astype(np.int32)
    out[U == 0] = P - 1
    return out


# ---- the weight rows ----------------------------------------------------------------------------------------------------
def heavy_row(P, j, share=0.9):
    """particle j holds `share` of the mass, the others share the rest equally"""
    if P == 1:
        return np.array([-50.0])
    w = np.full(P, -50.0 + math.log((1.0 - share) / (P - 1)))
    w[j] = -50.0 + math.log(share)
    return w


def geometric_row(P):
    return -50.0 - 0.7 * np.arange(P)


def weight_rows(P):
    """[(name, float64 [P])]: the fixed list of rows of one particle count.  The 'tie' rows are the constructed ESS ties
    (Exact.tie: no resampling, `<` is strict; with two particles 'single' and the 'floor' rows are ties as well),
    'all-inf' is the row of total weight 0."""
    rows = [("equal", np.full(P, -50.0)), ("geometric", geometric_row(P))]
    for name, j in (("heavy-first", 0), ("heavy-last", P - 1), ("heavy-middle", P // 2)):
        rows.append((name, heavy_row(P, j)))
    w = -50.0 - 0.3 * np.arange(P)
    w[0] = w[P - 1] = -49.0
    rows.append(("two-maxima", w))
    w = geometric_row(P)
    w[P // 2] = NEG
    rows.append(("inf-middle" if P > 1 else "all-inf", w))
    w = np.full(P, NEG)
    w[P // 3] = -50.0
    rows.append(("single", w))
    rows.append(("all-inf", np.full(P, NEG)))
    if P >= 3:  # the two sides of pclean_fixw's floor in one row
        w = -50.0 - 0.1 * np.arange(P)
        w[P // 2], w[P - 1] = -50.0 - 28.4, -50.0 - 28.6
        rows.append(("floor", w))
    elif P == 2:
        rows += [("floor-above", np.array([-50.0, -78.4])), ("floor-below", np.array([-50.0, -78.6]))]
    # multiples of 2^-3 in (-3, 0]: the shifts by 700 are exact, so the three rows have the same d and the same u
    g = -((np.arange(P) * 37) % 23) / 8.0
    rows += [("grid", g), ("grid-700", g - 700.0), ("grid+700", g + 700.0)]
    if P % 2 == 0:  # exact ESS ties: k = P / 2 particles at the maximum, the others at -inf -> ESS == P / 2 exactly
        k = P // 2
        a = np.where(np.arange(P) < k, -3.25, NEG)
        rows += [("tie-front", a), ("tie-back", a[::-1].copy())]
        if P > 2:
            rows.append(("tie-interleaved", np.where(np.arange(P) % 2 == 0, NEG, 11.5)))
    rng = np.random.default_rng(1)
    R = rng.normal(-50.0, 1.0, (30, P))
    R[::3] += rng.normal(0.0, 8.0, (10, P))
    rows += [(f"random{k}", R[k]) for k in range(30)]
    return rows


def degenerate_random_row(P):
    """the first of the random rows with 8-nat noise (the distribution checks' fourth row)"""
    return dict(weight_rows(P))["random0"]


def boundary_rows(be, P, seed, sweep, site, particle, n=64):
    """Rows [d_0, 0, -inf, ...] whose u_0 is solved from the implementation's own R so that x == u_0 exactly: the scan must
    step over particle 0 (`acc > x` is strict).  x = floor(R (u_0 + 2^40) / 2^64) == u_0 has the solution
    u_0 = floor(R 2^40 / (2^64 - R)) whenever that is in [2^12, 2^40 a], a < 1 chosen so that the row resamples for
    P >= 3; d_0 = log((u_0 + 1/2) 2^-40) puts e_0 in the middle between two integers (far from the 2^-10 class).
    Returns (W [n, P], is_boundary [n]); the other rows hold the geometric row."""
    assert P >= 2
    R = be.rand64(seed, np.arange(n, dtype=np.uint32), site, particle, sweep)
    W = np.tile(geometric_row(P), (n, 1))
    hit = np.zeros(n, dtype=bool)
    a_max = 0.25 if P < 5 else 0.9  # ESS of (a, 1) is (1 + a)^2 / (1 + a^2): below 1.5 for a < 0.267
    for i, r in enumerate(int(x) for x in R):
        u0 = (r << FIX_BITS) // ((1 << 64) - r)
        if not (1 << 12) <= u0 <= int(a_max * ONE):
            continue
        assert (r * (u0 + ONE)) >> 64 == u0
        W[i] = NEG
        W[i, 0], W[i, 1] = float(mpmath.log((mpf(u0) + mpf(1) / 2) / ONE)), 0.0
        hit[i] = True
    return W, hit


# ---- running a backend and checking what it returns ------------------------------------------------------------------------
def run(be, W, seed, sweep, block, retain_first):
    W = np.ascontiguousarray(W, dtype=np.float64)
    anc, inc, ess = be.maybe_resample(W, retain_first, seed, sweep, block)
    pg, tot = be.final_choice(W, 0, 1, seed, sweep)
    mh, tot2 = be.final_choice(W, 1, 1, seed, sweep)
    mh0, tot3 = be.final_choice(W, 1, 0, seed, sweep)
    assert np.array_equal(tot, tot2) and np.array_equal(tot, tot3), "log_total depends on the kind of choice"
    return dict(anc=anc, inc=inc, ess=ess, pg=pg, mh=mh, mh0=mh0, tot=tot)


def same(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(np.array_equal(a[k][rows_a], b[k][rows_b]) for k in a)


def device_u(be, W):
    """the implementation's own fixed-point weights of every row (0 where the maximum is -inf)"""
    W = np.asarray(W, dtype=np.float64)
    m = W.max(axis=1, keepdims=True)
    with np.errstate(invalid="ignore"):
        D = W - m
    D[np.isnan(D)] = NEG
    vals, inv = np.unique(D, return_inverse=True)
    return np.asarray(be.fixw(vals), dtype=np.uint64)[inv].reshape(D.shape).astype(np.int64), D


def verify(be, W, res, seed, sweep, block, retain_first, first_row=0, names=None, logml_bound=None):
    """Checks 1-6 on what run() returned for the rows W, whose Philox rows are first_row, first_row + 1, ...
    Returns dict(weights, near, resampled, undecided, mh_accepts)."""
    W = np.ascontiguousarray(W, dtype=np.float64)
    n, P = W.shape
    ex = [exact(W[i]) for i in range(n)]
    u, D = device_u(be, W)
    stats = dict(weights=0, near=0, resampled=0, undecided=0, mh_accepts=0)
    # 1. fixed-point weights
    for i, e in enumerate(ex):
        for p in range(P):
            got, want = int(u[i, p]), e.u[p]
            assert abs(got - want) <= 1, f"row {i} particle {p}: fixw({D[i, p]!r}) = {got}, floor(e) = {want}"
            if e.d[p] == 0.0 or e.d[p] < FLOOR:
                assert got == want
                continue
            stats["weights"] += 1
            stats["near"] += bool(e.near[p])
            assert e.near[p] or got == want, f"row {i} particle {p}: fixw({D[i, p]!r}) = {got}, floor(e) = {want}, e = {e.e[p]}"
    rows = np.arange(first_row, first_row + n, dtype=np.uint32)
    R = np.stack([be.rand64(seed, rows, site_resample(block), p, sweep) for p in range(P)], axis=1)
    picks = pick_all(u, R)
    final = pick_all(u, be.rand64(seed, rows, SITE_FINAL, 0, sweep)[:, None])[:, 0]
    Rmh = be.rand64(seed, rows, SITE_MH, 0, sweep)
    ident = np.arange(P, dtype=np.int32)
    log_p = mpmath.log(P)
    for i, e in enumerate(ex):
        tag = f"row {i} ({names[i] if names else ''}) P={P}"
        # 2. ESS
        ess = float(res["ess"][i])
        if e.U == 0:
            assert ess == 0.0, tag
        else:
            assert abs(mpf(ess) - e.ess) <= ess_bound(P) * e.ess, f"{tag}: ESS {ess!r}, exact {e.ess}"
        # 3. the decision
        if e.tie():
            expect = False
        elif e.decided():
            expect = bool(e.resamples())
        else:
            stats["undecided"] += 1
            expect = ess < P / 2.0
        if P <= 2 and e.U != 0:
            assert not expect, tag
        a = res["anc"][i]
        inc = float(res["inc"][i])
        if not expect:
            assert np.array_equal(a, ident) and inc == 0.0, f"{tag}: resampled at ESS {e.ess} (ancestors {a.tolist()}, inc {inc!r})"
        else:
            # 4. ancestors, integer for integer from the implementation's own u and R
            stats["resampled"] += 1
            want = picks[i].copy()
            if retain_first:
                want[0] = 0
            assert np.array_equal(a, want), f"{tag}: ancestors {a.tolist()}, expected {want.tolist()} (u = {u[i].tolist()})"
            if e.U == 0:  # total weight 0: every free particle takes P - 1, the increment is -inf, no error
                assert all(int(x) == P - 1 for x in a[(1 if retain_first else 0):]) and inc == NEG, tag
            # 5. increments
            elif logml_bound is not None:
                assert abs(mpf(inc) - (e.lse - log_p)) <= logml_bound(P, float(e.lse)), f"{tag}: inc {inc!r}, exact {e.lse - log_p}"
        tot = float(res["tot"][i])
        if e.U == 0:
            assert tot == NEG, tag
        elif logml_bound is not None:
            assert abs(mpf(tot) - e.lse) <= logml_bound(P, float(e.lse)), f"{tag}: log_total {tot!r}, exact {e.lse}"
        # 6. the final choice
        ui = [int(x) for x in u[i]]
        assert int(res["pg"][i]) == int(final[i]), f"{tag}: final pick {res['pg'][i]}, expected {final[i]} (u = {ui})"
        assert int(res["mh0"][i]) == int(final[i]), f"{tag}: MH without a current referent is the Categorical pick"
        want = mh_pick(ui, Rmh[i]) if P >= 2 else int(final[i])
        stats["mh_accepts"] += want
        assert int(res["mh"][i]) == want, f"{tag}: MH choice {res['mh'][i]}, expected {want} (u = {ui[:2]}, U = {sum(ui)})"
        if P == 2 and ui[0] == 0 and ui[1] > 0:
            assert int(res["mh"][i]) == 1, f"{tag}: a retained particle of weight 0 must be left"
    return stats


def check(be, W, seed, sweep, block, retain_first, first_row=0, names=None, logml_bound=None):
    res = run(be, W, seed, sweep, block, retain_first)
    return res, verify(be, W, res, seed, sweep, block, retain_first, first_row, names, logml_bound)


def big_call(P, small):
    """the rows `small` followed by geometric rows up to N_BIG rows"""
    return np.concatenate([small, np.tile(geometric_row(P), (N_BIG - len(small), 1))])


def deterministic_checks(be, P, logml_bound, seed=11, sweep=2, block=1):
    """checks 1-7 on the fixed rows of one particle count; returns the statistics of the fixed rows"""
    named = weight_rows(P)
    names = [k for k, _ in named]
    W = np.stack([w for _, w in named])
    n = len(W)
    total = None
    base = {}
    for retain in (1, 0):
        base[retain], stats = check(be, W, seed, sweep, block, retain, names=names, logml_bound=logml_bound)
        total = stats if total is None else total
    res = base[1]
    g = {k: i for i, k in enumerate(names)}
    u, _ = device_u(be, W)
    assert np.array_equal(u[g["grid"]], u[g["grid-700"]]) and np.array_equal(u[g["grid"]], u[g["grid+700"]])
    # 7a. row independence: the same rows inside a call of N_BIG rows
    big = big_call(P, W)
    rb, _ = check(be, big, seed, sweep, block, 1, names=names + ["filler"] * (N_BIG - n), logml_bound=logml_bound)
    assert same(res, rb, rows_b=slice(0, n)), "a row's results depend on the other rows of the call"
    # 7b. row offset: row i at offset k is row i + k at offset 0
    k = 7
    with be.offset(k):
        rs, _ = check(be, W[k:], seed, sweep, block, 1, first_row=k, names=names[k:], logml_bound=logml_bound)
    assert same(res, rs, rows_a=slice(k, n)), "row i at offset k differs from row i + k at offset 0"
    r0, _ = check(be, W, seed, sweep, block, 1, names=names, logml_bound=logml_bound)
    assert same(res, r0), "the row offset was not restored"
    # 7c. seed, sweep and block enter the counters (the draws of N_BIG rows cannot coincide by chance)
    for what, (s2, w2, b2) in (("seed", (seed + 1, sweep, block)), ("sweep", (seed, sweep + 1, block)), ("block", (seed, sweep, block + 1))):
        rv, _ = check(be, big, s2, w2, b2, 1, names=names + ["filler"] * (N_BIG - n), logml_bound=logml_bound)
        if P >= 6:  # (the geometric filler rows resample from six particles on)
            assert not np.array_equal(rv["anc"], rb["anc"]), f"the resampling draws ignore the {what}"
        if what != "block" and P >= 2:
            assert not np.array_equal(rv["pg"], rb["pg"]) and not np.array_equal(rv["mh"], rb["mh"]), f"the final draws ignore the {what}"
    return total


def boundary_checks(be, P, logml_bound, seed=23, sweep=4, block=1):
    """the constructed rows on which `acc > x` and `acc >= x` differ: the final pick (particle 0's R) and, from three
    particles on, the ancestor of particle 1.  Returns the number of boundary rows of each kind."""
    out = []
    for site, particle in [(SITE_FINAL, 0)] + ([(site_resample(block), 1)] if P >= 3 else []):
        W, hit = boundary_rows(be, P, seed, sweep, site, particle)
        assert hit.sum() >= 4, "too few boundary rows"
        res, stats = check(be, W, seed, sweep, block, 1, logml_bound=logml_bound)
        u, _ = device_u(be, W)
        R = be.rand64(seed, np.arange(len(W), dtype=np.uint32), site, particle, sweep)
        x = np.array([(int(r) * int(U)) >> 64 for r, U in zip(R, u.sum(axis=1))], dtype=np.int64)
        on = hit & (x == u[:, 0])  # (the implementation's u_0 is the one solved for: e_0 sits mid-way between integers)
        assert on.sum() == hit.sum()
        got = res["pg"] if site == SITE_FINAL else res["anc"][:, 1]
        assert (got[on] == 1).all(), "x == u_0 must step over particle 0"
        out.append(int(on.sum()))
    return out


# ---- distribution checks ------------------------------------------------------------------------------------------------
def distribution_rows(P):
    return [("geometric", geometric_row(P)), ("heavy-middle", heavy_row(P, P // 2)),
            ("inf-middle", dict(weight_rows(P)).get("inf-middle", geometric_row(P))), ("random-degenerate", degenerate_random_row(P))]


def tabulate(a):
    v, c = np.unique(np.asarray(a).ravel(), return_counts=True)
    return {int(k): int(n) for k, n in zip(v, c)}


def draw_items(P, name, w, res, retain_first=1):
    """gof items of N_BIG replicas of one row: the ancestors of every free particle (when the row resamples) and the
    final picks, against the exact normalised weights; a particle with u_p == 0 is left out of the expectation, so that
    a single draw of it fails"""
    e = exact(w)
    expected = {p: float(e.wn[p]) for p in range(P) if e.u[p] > 0}
    items = [(f"{name} final", expected, tabulate(res["pg"]))]
    resamples = e.decided() and bool(e.resamples()) and e.U > 0
    if resamples:
        free = res["anc"][:, (1 if retain_first else 0):]
        if free.size:
            items.append((f"{name} ancestors", expected, tabulate(free)))
    return items, resamples


def independence(a, b, wn, n_min=5.0):
    """chi-square test of independence of two ancestor columns over the replicas; particles whose expected joint count
    with themselves is below n_min are pooled into one category.  Returns (p, chi2, df); (1, 0, 0) when fewer than two
    categories remain."""
    from scipy.stats import chi2_contingency
    n = len(a)
    big = [p for p, v in enumerate(wn) if n * float(v) * float(v) >= n_min]
    cat = np.full(len(wn), -1)
    for k, p in enumerate(big):
        cat[p] = k
    K = len(big)
    rest = sum(float(v) for p, v in enumerate(wn) if p not in big)
    if n * rest * rest >= n_min:
        cat[cat < 0] = K
        K += 1
    elif K:  # a small remainder joins the last category
        cat[cat < 0] = K - 1
    if K < 2:
        return 1.0, 0.0, 0
    T = np.zeros((K, K))
    np.add.at(T, (cat[np.asarray(a)], cat[np.asarray(b)]), 1)
    T = T[T.sum(axis=1) > 0][:, T.sum(axis=0) > 0]
    if min(T.shape) < 2:
        return 0.0, math.inf, 0  # (one column is constant although it has several categories to draw from)
    c2, p, df, _ = chi2_contingency(T, correction=False)
    return float(p), float(c2), int(df)


def distribution_checks(be, P, gof, logml_bound, seed=31, sweep=5, block=1):
    """N_BIG replicas of four rows: goodness of fit of ancestors and final picks, independence of two ancestor columns.
    Returns (gof result, [(row, p, chi2, df)] of the independence checks)."""
    items, indep = [], []
    for k, (name, w) in enumerate(distribution_rows(P)):
        W = np.tile(w, (N_BIG, 1))
        res, _ = check(be, W, seed + k, sweep, block, 1, logml_bound=logml_bound)
        it, resamples = draw_items(P, name, w, res)
        items += it
        if resamples and P >= 3:
            indep.append((name,) + independence(res["anc"][:, 1], res["anc"][:, 2], exact(w).wn))
    return gof(items), indep
