"""The particle primitives against the arbitrary-precision restatement (tests/particle_exact.py), on the CPU oracle,
and the power of those checks.

The oracle leg runs the harness of tests/test_gpu_particle_primitives.py with pco_maybe_resample, pco_final_choice,
pco_fixw and pco_rand64 in the device's place: it proves the restatement and its bounds without a GPU.

The power self-test runs a NumPy sampler of the same primitives (Sim) under six mutations through the same checks.
Four of them change a distribution and are rejected by the distribution checks alone at p < 1e-6 (index off by one,
weights squared: goodness of fit; retained particle not kept: its ancestor column follows the weights instead of being
0; particle index missing from the counter: independence of two ancestor columns).  Two change an event of probability
below 64 * 2^-40 per draw (`>=` in the cumulative scan, `<=` at the ESS threshold), which no sample can see: they are
rejected, with certainty, by the constructed rows (boundary_rows, the exact ESS ties).  Every mutation also fails the
exact integer comparison of particle_exact.verify."""
import contextlib
import ctypes as C
import math

import mpmath
import numpy as np
import pytest

import particle_exact as px
import posterior_exact as pe


class OracleBackend:
    def __init__(self, oracle):
        self.o, self.L, self.k = oracle, oracle.lib(), 0

    @contextlib.contextmanager
    def offset(self, k):
        self.k = k
        try:
            yield
        finally:
            self.k = 0

    def maybe_resample(self, W, retain_first, seed, sweep, block):
        n, P = W.shape
        anc, inc, ess = np.empty((n, P), dtype=np.int32), np.empty(n), np.empty(n)
        self.L.pco_maybe_resample(n, P, self.o._p(W, C.c_double), int(retain_first), C.c_uint64(seed), C.c_uint32(sweep),
                                  C.c_uint32(block), C.c_int64(self.k), self.o._p(anc, C.c_int32), self.o._p(inc, C.c_double),
                                  self.o._p(ess, C.c_double))
        return anc, inc, ess

    def final_choice(self, W, mh, csmc, seed, sweep):
        n, P = W.shape
        ch, tot = np.empty(n, dtype=np.int32), np.empty(n)
        self.L.pco_final_choice(n, P, self.o._p(W, C.c_double), mh, csmc, C.c_uint64(seed), C.c_uint32(sweep),
                                C.c_int64(self.k), self.o._p(ch, C.c_int32), self.o._p(tot, C.c_double))
        return ch, tot

    def fixw(self, d):
        return np.array([self.L.pco_fixw(float(x)) for x in d], dtype=np.uint64)

    def rand64(self, seed, rows, site, particle, sweep):
        f = self.L.pco_rand64
        return np.array([f(seed, int(r), site, particle, sweep) for r in rows], dtype=np.uint64)


@pytest.fixture(scope="module")
def be(oracle):
    return OracleBackend(oracle)


def test_restatement_is_self_consistent():
    """pick_all is pick; the site constants are the header's; the fixed inputs hold few weights near an integer"""
    import os
    import re
    hdr = open(os.path.join(pe.ROOT, "include", "pclean_hip.h")).read()
    assert re.search(r"PCLEAN_SITE_RESAMPLE\(block\) \(0x40000000u \| ", hdr)
    assert re.search(r"PCLEAN_SITE_FINAL 0x50000000u", hdr) and re.search(r"PCLEAN_SITE_MH 0x50000001u", hdr)
    rng = np.random.default_rng(0)
    for P in px.P_EDGES:
        rows = px.weight_rows(P)
        u = np.array([px.exact(w).u for _, w in rows], dtype=np.int64)
        R = rng.integers(0, 2 ** 64, size=(len(rows), 3), dtype=np.uint64)
        R[0] = [0, 2 ** 64 - 1, 2 ** 63]
        got = px.pick_all(u, R)
        for i in range(len(rows)):
            assert [px.pick(u[i].tolist(), r) for r in R[i]] == got[i].tolist()
        near = sum(sum(px.exact(w).near) for _, w in rows)
        tot = sum(sum(1 for d in px.exact(w).d if d != 0.0 and d >= px.FLOOR) for _, w in rows)
        assert near <= 0.01 * tot, (P, near, tot)
        names = [k for k, _ in rows]
        assert "all-inf" in names and "single" in names and ("floor" in names or P < 3)
        for k, w in rows:
            e = px.exact(w)
            if k.startswith("tie"):
                assert e.U == (P // 2) * px.ONE and abs(e.ess - mpmath.mpf(P) / 2) < 1e-30
            elif k.startswith("floor") and P >= 2:
                # 28.4 below the maximum goes through pclean_exp (0 < e < 1, floor 0), 28.6 below takes the early exit
                assert any(d >= px.FLOOR and 0 < v < 1 for v, d in zip(e.e, e.d)) or k == "floor-below"
                assert any(-math.inf < d < px.FLOOR for d in e.d) or k == "floor-above"
    assert px.pick([0, 0, 0], 5) == 2 and px.pick([0, 4, 0], 2 ** 64 - 1) == 1 and px.mh_pick([0, 7], 2 ** 64 - 1) == 1
    assert px.mh_pick([0, 0], 0) == 0


@pytest.mark.parametrize("P", px.P_EDGES)
def test_oracle_primitives_match_exact_restatement(be, P):
    stats = px.deterministic_checks(be, P, pe.logml_bound)
    print(f"P={P}: {stats}")
    assert stats["undecided"] == 0, "a fixed row sits within the ESS bound of P / 2 without being a constructed tie"
    assert stats["near"] <= 0.01 * stats["weights"]
    assert stats["resampled"] > 0 and (P <= 2 or stats["resampled"] > 5)
    if P >= 2:
        print(f"P={P}: boundary rows {px.boundary_checks(be, P, pe.logml_bound)}")


@pytest.mark.parametrize("P", px.P_EDGES)
def test_oracle_primitive_draws_follow_exact_weights(be, P):
    res, indep = px.distribution_checks(be, P, pe.gof, pe.logml_bound)
    print(f"P={P}: {pe.describe(res)}; independence {indep}")
    assert res["p"] > pe.ALPHA, pe.describe(res)
    assert P < 6 or indep, "no row resampled"
    for name, p, c2, df in indep:
        assert p > pe.ALPHA, (name, p, c2, df)


# ---- power self-test ------------------------------------------------------------------------------------------------------
MUTATIONS = ["off-by-one", "scan-ge", "retained-dropped", "squared", "ess-le", "counter-without-particle"]
STATISTICAL = {"off-by-one", "retained-dropped", "squared", "counter-without-particle"}


def _mix(x):
    """splitmix64's finaliser on uint64 arrays"""
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


class Sim:
    """the primitives in NumPy and Python integers, with one optional mutation; its random bits are a hash of the counter"""

    def __init__(self, mutation=None):
        self.mut, self.k = mutation, 0

    @contextlib.contextmanager
    def offset(self, k):
        self.k = k
        try:
            yield
        finally:
            self.k = 0

    def fixw(self, d):
        return np.array([px.exact(np.array([0.0, x])).u[1] if x > -math.inf else 0 for x in d], dtype=np.uint64)

    def rand64(self, seed, rows, site, particle, sweep):
        with np.errstate(over="ignore"):
            x = _mix(np.asarray(rows, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B97F4A7C15))
            x = _mix(x ^ np.uint64((site << 32) | sweep))
            return _mix(x + np.uint64(particle) * np.uint64(0xD1B54A32D192ED03))

    def _u(self, W):
        u, _ = px.device_u(self, W)
        if self.mut == "squared":
            u = ((u.astype(object) * u.astype(object)) >> 40).astype(np.int64)
        return u

    def _pick(self, u, R):
        if self.mut == "scan-ge":
            cum = np.cumsum(u, axis=1)
            U = cum[:, -1]
            X = ((np.asarray(R).astype(object) * U.astype(object)[:, None]) >> 64).astype(np.int64)
            out = (cum[:, None, :] >= X[:, :, None]).argmax(axis=2).astype(np.int32)
            out[U == 0] = u.shape[1] - 1
            return out
        out = px.pick_all(u, R)
        if self.mut == "off-by-one":
            out = np.minimum(out + 1, u.shape[1] - 1).astype(np.int32)
        return out

    def maybe_resample(self, W, retain_first, seed, sweep, block):
        n, P = W.shape
        u = self._u(W)
        rows = np.arange(n, dtype=np.uint32) + np.uint32(self.k)
        part = (lambda p: 0) if self.mut == "counter-without-particle" else (lambda p: p)
        R = np.stack([self.rand64(seed, rows, px.site_resample(block), part(p), sweep) for p in range(P)], axis=1)
        picks = self._pick(u, R)
        Ud = u.sum(axis=1).astype(np.float64)
        s2 = (u.astype(np.float64) ** 2).sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            ess = np.where(Ud > 0, Ud * Ud / s2, 0.0)
            lse = W.max(axis=1) + np.log(Ud * 2.0 ** -40)
        did = (ess <= P / 2.0) if self.mut == "ess-le" else (ess < P / 2.0)
        if retain_first and self.mut != "retained-dropped":
            picks[:, 0] = 0
        anc = np.where(did[:, None], picks, np.arange(P, dtype=np.int32)[None, :]).astype(np.int32)
        return anc, np.where(did, lse - math.log(P), 0.0), ess

    def final_choice(self, W, mh, csmc, seed, sweep):
        n, P = W.shape
        u = self._u(W)
        rows = np.arange(n, dtype=np.uint32) + np.uint32(self.k)
        Ud = u.sum(axis=1).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            tot = W.max(axis=1) + np.log(Ud * 2.0 ** -40)
        if mh and csmc and P >= 2:
            R = self.rand64(seed, rows, px.SITE_MH, 0, sweep)
            return np.array([px.mh_pick(u[i, :2].tolist() + [int(u[i, 2:].sum())], R[i]) for i in range(n)], dtype=np.int32), tot
        return self._pick(u, self.rand64(seed, rows, px.SITE_FINAL, 0, sweep)[:, None])[:, 0], tot


P_POWER = 8  # one bucket; an even count (exact ESS ties exist), every distribution row resamples


def _statistics(be, P=P_POWER, seed=31, sweep=5, block=1):
    """the distribution checks WITHOUT the exact comparison: smallest p-value over goodness of fit, independence and the
    retained column (which must be 0 in every replica of a resampled row)"""
    items, ps = [], []
    for k, (name, w) in enumerate(px.distribution_rows(P)):
        res = px.run(be, np.tile(w, (px.N_BIG, 1)), seed + k, sweep, block, 1)
        it, resamples = px.draw_items(P, name, w, res)
        assert resamples
        items += it
        ps.append(px.independence(res["anc"][:, 1], res["anc"][:, 2], px.exact(w).wn)[0])
        items.append((f"{name} retained", {0: 1.0}, px.tabulate(res["anc"][:, 0])))
    ps.append(pe.gof(items)["p"])
    return min(ps)


def test_power_unmutated_sampler_passes():
    be = Sim()
    px.deterministic_checks(be, P_POWER, pe.logml_bound)
    px.boundary_checks(be, P_POWER, pe.logml_bound)
    assert _statistics(be) > pe.ALPHA


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_power_mutation_is_rejected(mutation):
    be = Sim(mutation)
    with pytest.raises(AssertionError):  # the exact comparison sees every one of them
        px.deterministic_checks(be, P_POWER, pe.logml_bound)
        px.boundary_checks(be, P_POWER, pe.logml_bound)
    if mutation in STATISTICAL:
        p = _statistics(be)
        print(f"{mutation}: p = {p:.3g}")
        assert p < 1e-6
    elif mutation == "scan-ge":  # a 2^-40 event: the constructed boundary rows alone, every other check passes
        px.deterministic_checks(be, P_POWER, pe.logml_bound)
        assert _statistics(be) > pe.ALPHA
        with pytest.raises(AssertionError, match="final pick|ancestors"):
            px.boundary_checks(be, P_POWER, pe.logml_bound)
    else:  # ess-le: the constructed ties alone
        assert _statistics(be) > pe.ALPHA
        px.boundary_checks(be, P_POWER, pe.logml_bound)
        with pytest.raises(AssertionError, match=r"\(tie-.*resampled at ESS"):
            px.deterministic_checks(be, P_POWER, pe.logml_bound)
