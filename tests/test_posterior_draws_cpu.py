"""Sweep draws against EXACT posteriors, on the CPU oracle (tests/oracle_engine.py), and the power of the check.

tests/posterior_exact.py turns the literal interpreter's per-candidate scores (oracle/literal.py) into the closed-form
output distribution of one batched sweep per row; S sweeps with sweep_idx = 0..S-1 over one frozen trace give S
independent draws per row, pooled into one G-test.  The oracle's draws equal the device's bit for bit (the parity
tests), so this leg checks the closed forms and the thresholds without a GPU and catches a contract-level mistake
that both sides share (a mis-weighted retained particle, an inverted MH ratio, a Philox counter without the sweep
index, a draw off by one).  tests/test_gpu_posterior_draws.py runs the same cases on the device at full size.

The power self-test samples with NumPy from perturbed distributions with exactly the S, rows and pooling of the GPU
leg's cases (posterior_exact.PROGRAMS / TWO_BLOCK, S_GPU, SPREAD_SWEEPS): every mutation must be rejected with
p < 1e-6 and exact samples must pass.  The pooled all-row cases catch the gross mutations (the dropped 1/P mass, an
inverted MH acceptance, paired sweep indices); a 0.1-nat shift of a near candidate moves a probability p by about
0.1 p (1 - p) and is caught by the spread-row case (SPREAD_SWEEPS draws of the rows that hold a near candidate),
not by the all-row cases at S_GPU."""
import numpy as np
import pytest

import posterior_exact as pe

S_SWEEPS = 60  # CPU: the device leg uses posterior_exact.S_GPU


@pytest.fixture(scope="module")
def prog():
    S = pe.draw_program(300, seed=0, n_dead=3)
    return S, pe.RowConditionals(S), pe.check_rows(S)


@pytest.fixture(scope="module")
def prog2():
    S = pe.draw_program(300, seed=1, two_blocks=True)
    rows = np.array([i for i, k in enumerate(S["kind"]) if k in ("peaked", "spread", "tied", "new")][::2])
    return S, pe.RowConditionals(S), rows


def _engine(oracle, S):
    from oracle_engine import OracleEngine
    return OracleEngine(oracle, S["lw"], S["obs"], cached=True)


@pytest.mark.parametrize("P,mh", [(1, False), (2, False), (2, True), (3, False), (9, False)],
                         ids=["P1", "P2-PG", "P2-MH", "P3", "P9"])
def test_oracle_draws_follow_exact_posterior(oracle, prog, P, mh):
    S, rc, rows = prog
    res, dev, _ = pe.one_block_case(_engine(oracle, S), S, rc, rows, P, mh, S_SWEEPS, seed=101 + P)
    print(f"oracle P={P}{' MH' if mh else ''}: {pe.describe(res)}; logml deviation {dev:.3f} of its bound")
    assert res["p"] > pe.ALPHA, pe.describe(res)
    assert dev <= 1.0
    if P == 1:  # nothing moves: every draw is the current referent
        assert res["df"] == 0 and not np.isinf(res["G"])


def test_oracle_draws_without_current_referent(oracle):
    """cur = -1 (initialize_trace): no retained particle, the output is pi for every P"""
    S = pe.draw_program(300, seed=2)
    tr, kind = S["trace"], S["kind"]
    t = tr.tables["A"]
    free = [i for i in range(len(kind)) if (kind[i] == "flat" and i % 2 == 0) or (kind[i] == "peaked" and i % 3 == 0)]
    for i in free:
        t.counts[tr.cur[0, i]] -= 1
        tr.cur[0, i] = -1
    rc = pe.RowConditionals(S)
    res, dev, _ = pe.one_block_case(_engine(oracle, S), S, rc, np.array(free), 3, False, S_SWEEPS, seed=7)
    print(f"oracle cur=-1 P=3: {pe.describe(res)}; logml deviation {dev:.3f} of its bound")
    assert res["p"] > pe.ALPHA, pe.describe(res)
    assert dev <= 1.0


def test_oracle_two_block_mh_follows_closed_form(oracle, prog2):
    S, rc, rows = prog2
    res = pe.two_block_case(_engine(oracle, S), S, rc, rows, S_SWEEPS, seed=31)
    print(f"oracle two blocks MH: {pe.describe(res)}")
    assert res["p"] > pe.ALPHA, pe.describe(res)


def test_oracle_latent_draws_follow_exact_posterior(oracle, prog):
    """sweep_latent of A's own choice against LatentProposal's pi: (1/P) d_cur + (1 - 1/P) pi (PG), ~pi (MH)"""
    S, rc, rows = prog
    for P, mh in [(2, False), (2, True), (9, False)]:
        res = pe.latent_case(_engine(oracle, S), S, rc, P, mh, S_SWEEPS, seed=404 + P)
        print(f"oracle latent P={P}{' MH' if mh else ''}: {pe.describe(res)}")
        assert res["p"] > pe.ALPHA, pe.describe(res)


# ---- power self-test: the device leg's cases, sampled with NumPy ------------------------------------------------
def _sample(rng, dist, n):
    keys = list(dist)
    p = np.array([dist[k] for k in keys])
    idx = rng.choice(len(keys), size=n, p=p / p.sum())
    return [keys[j] for j in idx]


def _items(rng, exact, draw_from, n, pairs=False):
    items = []
    for r, (e, d) in enumerate(zip(exact, draw_from)):
        if pairs:  # sweep indices 2j and 2j + 1 give the same draw
            half = _sample(rng, d, n // 2)
            draws = [x for x in half for _ in range(2)]
        else:
            draws = _sample(rng, d, n)
        items.append((r, e, pe.tabulate(draws)))
    return items


@pytest.fixture(scope="module", params=list(pe.PROGRAMS))
def gpu_case(request):
    """the device leg's program, its checked rows and spread rows, with their exact (pi, s)"""
    S = pe.draw_program(**pe.PROGRAMS[request.param])
    rc = pe.RowConditionals(S)
    tr = S["trace"]
    rows, spread = pe.check_rows(S), pe.spread_rows(S, rc)
    return ([(rc.block0(int(i))[0], int(tr.cur[0, i])) for i in rows],
            [(rc.block0(int(i))[0], int(tr.cur[0, i])) for i in spread])


@pytest.fixture(scope="module")
def gpu_two_block():
    S = pe.draw_program(**pe.TWO_BLOCK)
    return S, pe.RowConditionals(S), pe.two_block_rows(S)


def test_power_exact_samples_pass(gpu_case, gpu_two_block):
    rows, spread = gpu_case
    rng = np.random.default_rng(1)
    for P in (2, 9):
        exact = [pe.pg_one_block(pi, s, P) for pi, s in rows]
        res = pe.gof(_items(rng, exact, exact, pe.S_GPU))
        assert res["p"] > pe.ALPHA, pe.describe(res)
    exact = [pe.pg_one_block(pi, s, pe.SPREAD_P) for pi, s in spread]
    res = pe.gof(_items(rng, exact, exact, pe.SPREAD_SWEEPS))
    assert res["p"] > pe.ALPHA, pe.describe(res)
    S, rc, trows = gpu_two_block
    exact = pe.two_block_expected(S, rc, trows)
    res = pe.gof(_items(rng, exact, exact, pe.S_GPU))
    assert res["p"] > pe.ALPHA, pe.describe(res)


def test_power_near_candidate_shifted(gpu_case):
    """the spread-row case of the device leg: its rows, SPREAD_P, SPREAD_SWEEPS draws per row, one pooled G-test"""
    _, spread = gpu_case
    assert len(spread) >= 20
    rng = np.random.default_rng(2)
    exact = [pe.pg_one_block(pi, s, pe.SPREAD_P) for pi, s in spread]
    bad = [pe.pg_one_block(pe.shift_near(pi, s), s, pe.SPREAD_P) for pi, s in spread]
    res = pe.gof(_items(rng, exact, bad, pe.SPREAD_SWEEPS))
    print(f"shifted by 0.1 nats ({len(spread)} rows):", pe.describe(res))
    assert res["p"] < 1e-6


def test_power_retained_mass_dropped(gpu_case):
    rows, _ = gpu_case
    rng = np.random.default_rng(3)
    exact = [pe.pg_one_block(pi, s, 2) for pi, s in rows]
    bad = [dict(pi) for pi, s in rows]
    res = pe.gof(_items(rng, exact, bad, pe.S_GPU))
    print("1/P on the retained value dropped:", pe.describe(res))
    assert res["p"] < 1e-6


def test_power_mh_acceptance_inverted(gpu_two_block):
    S, rc, rows = gpu_two_block
    rng = np.random.default_rng(4)
    exact = pe.two_block_expected(S, rc, rows)
    bad = pe.two_block_expected(S, rc, rows, invert=True)
    res = pe.gof(_items(rng, exact, bad, pe.S_GPU))
    print("MH acceptance inverted:", pe.describe(res))
    assert res["p"] < 1e-6


def test_power_sweep_indices_identical(gpu_case):
    rows, _ = gpu_case
    rng = np.random.default_rng(5)
    exact = [pe.pg_one_block(pi, s, 9) for pi, s in rows]
    res = pe.gof(_items(rng, exact, exact, pe.S_GPU, pairs=True))
    print("two sweep indices with one draw:", pe.describe(res))
    assert res["p"] < 1e-6
