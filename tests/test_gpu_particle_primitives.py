"""The device's particle primitives (fix_weights / fix_pick of csrc/sweep_internal.h, maybe_resample_kernel and
final_choice_kernel of csrc/sweep.hip, through pclean_maybe_resample and pclean_final_choice) against the
arbitrary-precision restatement of tests/particle_exact.py — not against the C++ oracle, which compiles the same
pclean_detmath.h and was written from the same reading of row_inference.jl:76-105,158-165.

Per particle count at both edges of every DISPATCH_PMAX bucket: the fixed weight rows (equal, geometric, one heavy
particle, tied maxima, -inf entries, total weight 0, both sides of pclean_fixw's floor, exact shifts by 700, exact ESS
ties, random and degenerate rows) through the deterministic checks (fixed-point weights, ESS, the strict resampling
decision, ancestors and final picks integer for integer from the device's own u and random bits, the log-ML
increments, the MH rule, row independence inside a call of 4 099 rows, the row offset, seed / sweep / block in the
counters); rows constructed from the device's random bits so that x == u_0 exactly (`acc > x` is strict); and 4 099
replicas of four rows whose ancestors and final picks are tested for goodness of fit against the exact normalised
weights and for independence between particles.  tests/test_particle_exact_cpu.py runs the same harness on the oracle
and measures its power under six mutations."""
import contextlib

import numpy as np
import pytest

import particle_exact as px
import posterior_exact as pe

pytestmark = pytest.mark.gpu


class DeviceBackend:
    def __init__(self, hip):
        self.hip = hip

    @contextlib.contextmanager
    def offset(self, k):
        self.hip.set_row_offset(k)
        try:
            yield
        finally:
            self.hip.set_row_offset(0)

    def maybe_resample(self, W, retain_first, seed, sweep, block):
        return self.hip.maybe_resample(W, bool(retain_first), seed, sweep, block)

    def final_choice(self, W, mh, csmc, seed, sweep):
        return self.hip.final_choice(W, mh, csmc, seed, sweep)

    def fixw(self, d):
        return self.hip.debug_detmath(np.ascontiguousarray(d, dtype=np.float64))[2]

    def rand64(self, seed, rows, site, particle, sweep):
        return self.hip.debug_rand64(seed, rows, site, particle, sweep)


@pytest.fixture(scope="module")
def be(hip):
    hip.set_row_offset(0)
    return DeviceBackend(hip)


@pytest.mark.parametrize("P", px.P_EDGES)
def test_device_primitives_match_exact_restatement(be, P):
    stats = px.deterministic_checks(be, P, pe.logml_bound)
    print(f"\n[P={P}] {stats}")
    assert stats["undecided"] == 0
    assert stats["near"] <= 0.01 * stats["weights"]
    assert stats["resampled"] > 0 and (P <= 2 or stats["resampled"] > 5)


@pytest.mark.parametrize("P", px.P_EDGES[1:])
def test_device_scan_is_strict_at_a_boundary(be, P):
    """rows solved from the device's own random bits so that x == u_0: the pick must step over particle 0"""
    print(f"\n[P={P}] boundary rows {px.boundary_checks(be, P, pe.logml_bound)}")


@pytest.mark.parametrize("P", px.P_EDGES)
def test_device_primitive_draws_follow_exact_weights(be, P):
    res, indep = px.distribution_checks(be, P, pe.gof, pe.logml_bound)
    print(f"\n[P={P}] {pe.describe(res)}; independence of ancestors 1 and 2: {indep}")
    assert res["p"] > pe.ALPHA, pe.describe(res)
    assert P < 6 or indep, "no row resampled"
    for name, p, c2, df in indep:
        assert p > pe.ALPHA, (name, p, c2, df)
