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
not by the all-row cases at S_GPU.

PG with P > 2 over two dependent blocks ends with unequal particle weights; its closed form
(posterior_exact.pg_two_blocks, one integral per distinct block-0 value) is checked here against the direct
enumeration of the particles' values for P <= 4, against the oracle's draws at P = 3 and 9, and for its power against
four mistakes of the final pick.  Not covered by an exact posterior: rows that can draw a ProposalDummyValue, the
hospital workload, and resampling that fires inside a sweep (three or more blocks, or prior proposals) together with
apply_ancestors_kernel — those stay pinned to the oracle, and tests/test_particle_exact_cpu.py pins the primitive
they call.

The tabulated kind (FormatName, ExpandOnShortVersion) has no CPU oracle leg: neither oracle layer below the literal
interpreter knows the two distributions.  Its part here states the conditions the device leg's inputs must meet
(posterior_exact.tab_draw_program) and measures the power of tests/test_gpu_tabulated_draws.py's cases against four
mistakes of a sweep: a skipped missing observation, two exchanged classes, a dropped -log(n), a class byte read one
column off."""
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


@pytest.mark.parametrize("P", [3, 9])
def test_oracle_two_block_pg_follows_closed_form(oracle, prog2, P):
    """PG with P > 2 over two dependent blocks: unequal final weights exp(Z1(x_p)), posterior_exact.pg_two_blocks"""
    S, rc, rows = prog2
    res = pe.two_block_case(_engine(oracle, S), S, rc, rows, S_SWEEPS, seed=31 + P, P=P, mh=False)
    print(f"oracle two blocks PG P={P}: {pe.describe(res)}")
    assert res["p"] > pe.ALPHA, pe.describe(res)


def test_oracle_two_block_pg_without_current_referent(oracle):
    S = pe.draw_program(300, seed=1, two_blocks=True)
    rows = pe.two_block_free_rows(S)
    assert len(rows) >= 40
    pe.free_rows(S, rows, blocks=(0, 1))
    res = pe.two_block_case(_engine(oracle, S), S, pe.RowConditionals(S), rows, S_SWEEPS, seed=41, P=3, mh=False)
    print(f"oracle two blocks PG cur=-1 P=3: {pe.describe(res)}")
    assert res["p"] > pe.ALPHA, pe.describe(res)


@pytest.mark.parametrize("P", [2, 3, 4])
def test_pg_two_block_integral_agrees_with_enumeration(prog2, P):
    """E[1 / (c + S_k)] as the one-dimensional integral against the sum over all k-tuples of block-0 values, on every
    sixth row with and without the retained particle, and with each mutation of the power test"""
    S, rc, rows = prog2
    worst, several = 0.0, 0
    for i in rows[::6]:
        pi0, z0, b1 = rc.two_blocks(int(i))
        pi0 = {k: v for k, v in pi0.items() if v >= 1e-13}
        val = {k: rc.value(0, k) for k in pi0}
        cur = (int(S["trace"].cur[0, i]), int(S["trace"].cur[1, i]))
        val[cur[0]] = rc._cur_value(0, cur[0])
        several += len({val[k] for k in pi0}) > 1
        for s in (cur, None):
            for mut in (None,) + pe.PG_MUTATIONS:
                a = pe.pg_two_blocks(pi0, b1, s, lambda t: val[t], P, mutation=mut)
                b = pe.pg_two_blocks(pi0, b1, s, lambda t: val[t], P, mutation=mut, enumerate_it=True)
                assert set(a) == set(b)
                worst = max(worst, max(abs(a[k] - b[k]) for k in a))
                assert abs(sum(a.values()) - 1.0) < 1e-9, (i, s, mut, sum(a.values()))
    print(f"P={P}: integral against enumeration, largest difference {worst:.3g}; {several} rows with several block-0 values")
    assert several >= 5 and worst <= 1e-12
    if P == 2:  # two particles, no referent: P q z / (z + z') summed over the second particle's value by hand
        mu, z = {"a": 0.25, "b": 0.75}, {"a": 1.0, "b": 0.5}
        for c, k, want in [(1.0, 1, 0.25 / 2.0 + 0.75 / 1.5), (0.5, 2, 0.0625 / 2.5 + 0.375 / 2.0 + 0.5625 / 1.5)]:
            assert abs(float(pe.inv_moment(c, k, mu, z)) - want) < 1e-15


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


@pytest.fixture(scope="module", params=pe.TWO_BLOCK_PG[:2])
def gpu_two_block_pg(request, gpu_two_block):
    """the exact closed form of the device leg's two-block PG case at P particles, and P"""
    S, rc, rows = gpu_two_block
    return request.param, pe.two_block_expected(S, rc, rows, P=request.param, mh=False)


def test_power_two_block_pg_exact_samples_pass(gpu_two_block_pg):
    P, exact = gpu_two_block_pg
    res = pe.gof(_items(np.random.default_rng(20 + P), exact, exact, pe.S_GPU))
    print(f"two blocks PG P={P}, exact samples:", pe.describe(res))
    assert res["p"] > pe.ALPHA, pe.describe(res)


@pytest.mark.parametrize("mutation", pe.PG_MUTATIONS)
def test_power_two_block_pg_mutation_is_rejected(gpu_two_block, gpu_two_block_pg, mutation):
    """the device leg's rows and S_GPU draws per row: a uniform final pick, a retained particle weighted like a fresh
    draw, a pick proportional to w^2 and Z1 taken at the retained value for every particle each fail at p < 1e-6 — at
    nine particles every one of them, at three all but w^2: with two free particles, most of them on one block-0 value,
    squaring the weights moves too little mass for S_GPU draws (p = 0.77 measured); the nine- and 33-particle cases of
    the device leg carry that mutation."""
    S, rc, rows = gpu_two_block
    P, exact = gpu_two_block_pg
    bad = pe.two_block_expected(S, rc, rows, P=P, mh=False, mutation=mutation)
    res = pe.gof(_items(np.random.default_rng(30 + P), exact, bad, pe.S_GPU))
    print(f"two blocks PG P={P}, {mutation}:", pe.describe(res))
    if (P, mutation) != (3, "weights squared"):
        assert res["p"] < 1e-6


def test_power_sweep_indices_identical(gpu_case):
    rows, _ = gpu_case
    rng = np.random.default_rng(5)
    exact = [pe.pg_one_block(pi, s, 9) for pi, s in rows]
    res = pe.gof(_items(rng, exact, exact, pe.S_GPU, pairs=True))
    print("two sweep indices with one draw:", pe.describe(res))
    assert res["p"] < 1e-6


# ---- the tabulated kind (FormatName, ExpandOnShortVersion): conditions on the inputs and the power of the device leg ----
import contextlib  # noqa: E402
import math  # noqa: E402

import tabulated_program as tp  # noqa: E402

lit = pe.lit


def _mutations(S):
    """the four mistakes the device leg (tests/test_gpu_tabulated_draws.py) must be able to see, as replacements of the
    literal interpreter's two densities: {name: (format_name_logpdf, expand_on_short_version_logpdf)}"""
    f0, g0 = lit.format_name_logpdf, lit.expand_on_short_version_logpdf
    EQUAL, INITIAL = math.log(0.9999), math.log(0.0001)
    dom = S["lw"].latent_dom[("A", "x")]
    strings = [dom.string(v) for v in range(len(dom))]
    nxt = {w: strings[(v + 1) % len(strings)] for v, w in enumerate(strings)}  # the value one column further

    def f_skip(o, name):
        return 0.0 if o is None else f0(o, name)

    def g_skip(o, short, options):
        return 0.0 if o is None else g0(o, short, options)

    def f_swap(o, name):
        v = f0(o, name)
        return v if o is None or name == "" or v == EQUAL else (-1000.0 if v == INITIAL else INITIAL)

    def g_one(o, short, options):
        v = g0(o, short, options)
        return v if o is None or v == -1000.0 else -0.0

    def f_next(o, name):  # class byte of (o, next value), density row of the value itself
        if o is None or name == "":
            return f0(o, name)
        return f0(o, nxt[name]) if nxt[name] != "" else -1000.0

    def g_next(o, short, options):
        if o is None:
            return g0(o, short, options)
        if not lit._is_short_version(nxt[short], o):
            return -1000.0
        n = sum(1 for x in options if lit._is_short_version(short, x))
        return -math.log(n) if n > 0 else -1000.0

    return {"exact": (f0, g0), "a: missing observation skipped": (f_skip, g_skip), "b: classes 1 and 2 exchanged": (f_swap, g0),
            "c: -log(n) dropped": (f0, g_one), "d: class byte one column off": (f_next, g_next)}


@contextlib.contextmanager
def _densities(f, g):
    f0, g0 = lit.format_name_logpdf, lit.expand_on_short_version_logpdf
    lit.format_name_logpdf, lit.expand_on_short_version_logpdf = f, g
    try:
        yield
    finally:
        lit.format_name_logpdf, lit.expand_on_short_version_logpdf = f0, g0


def _tab_variant(name, f, g):
    """(pi, current) per row of every case of the device leg, under the densities f, g"""
    with _densities(f, g):
        S = pe.tab_draw_program(**pe.PROGRAMS_TAB[name])
        rc = pe.RowConditionals(S)
        tr = S["trace"]
        out = {"S": S, "rows": pe.check_rows(S)}
        out["obs"] = [(rc.block0(int(i)), int(tr.cur[0, i])) for i in out["rows"]]
        out["spread"] = [(rc.block0(int(i)), int(tr.cur[0, i])) for i in pe.tab_spread_rows(S)]
        live, ev_off, ev_rows, ev_ctx, excl = pe.latent_setup(S)
        out["latent"] = pe.latent_exact(S, rc, live, ev_off, ev_rows, np.arange(len(live)))
        out["hub_evidence"] = int((ev_off[1:] - ev_off[:-1]).max())
        F = pe.tab_draw_program(**pe.PROGRAMS_TAB[name])
        free = pe.tab_free_rows(F)
        pe.free_rows(F, free)
        rcf = pe.RowConditionals(F)
        out["free"] = [(rcf.block0(int(i)), None) for i in free]
    return out


@pytest.fixture(scope="module", params=list(pe.PROGRAMS_TAB))
def tab_cases(request):
    S = pe.tab_draw_program(**pe.PROGRAMS_TAB[request.param])
    return request.param, {m: _tab_variant(request.param, f, g) for m, (f, g) in _mutations(S).items()}


def _tab_closed_forms(v):
    """{case name: ([closed-form output distribution per row], draws per row)} — the cases of the device leg"""
    out = {}
    for P, mh in pe.TAB_PARTICLES:
        out[f"observed P{P}{'-MH' if mh else ''}"] = ([pe.mh_one_block(pi, s) if mh else pe.pg_one_block(pi, s, P)
                                                       for (pi, z), s in v["obs"]], pe.S_GPU)
    out["no referent P3"] = ([dict(pi) for (pi, z), s in v["free"]], pe.S_GPU)
    out["spread rows"] = ([pe.pg_one_block(pi, s, pe.SPREAD_P) for (pi, z), s in v["spread"]], pe.SPREAD_SWEEPS)
    for P, mh in pe.TAB_LATENT:
        out[f"latent P{P}{'-MH' if mh else ''}"] = ([pe.mh_one_block(pi, c) if mh else pe.pg_one_block(pi, c, P)
                                                     for pi, c in v["latent"]], pe.S_GPU)
    return out


def test_tab_program_conditions(tab_cases):
    """conditions on the inputs of the device leg (not measurements): every checked row is carried by ordinary terms,
    every class byte and both missing columns are scored with and without the AddTypos term, and little of a row's
    expected mass sits in gof's pooled cell"""
    name, variants = tab_cases
    v = variants["exact"]
    S = v["S"]
    t = S["trace"].tables["A"]
    kinds = S["kind"]
    for k in ("equal", "initial", "long", "nolong", "tied", "new", "filler"):
        assert (kinds == k).sum() >= 20, k
    assert (kinds == "flat").sum() == 60 and v["hub_evidence"] > 60  # (more than a wavefront of missing observations)
    if name == "large":
        assert t.n >= 1024 and ((t.n + 15) & ~15) % 64 != 0 and not t.live[:t.n].all()
    for (pi, z), s in v["obs"] + v["free"]:
        assert z > -100.0
    names, longs, d = S["names"], S["longs"], S["dirty"]
    assert "" not in names and sum(w.startswith(("J", "j")) for w in names) >= 8 and any("*" in w for w in names)
    assert set(names) & set(longs) and any(w != w.lower() and w != w.upper() for w in names)
    n_of = {w: sum(tp.is_short_version(w, x) for x in longs) for w in names}
    assert {1, 2} <= set(n_of.values()) and max(n_of.values()) >= 5
    seen = set()
    for i in v["rows"]:
        typo = d["Typo"][i] is not None
        for w in names:  # (every name is a candidate: through the entities that hold it or through the new row)
            seen.add(("format", 3 if d["Name"][i] is None else tp.format_name_class(d["Name"][i], w), typo))
            seen.add(("short", 3 if d["Long"][i] is None else tp.pair_class(tp.SHORT, d["Long"][i], w), typo))
    assert seen == {("format", c, t_) for c in (0, 1, 2, 3) for t_ in (False, True)} | {("short", c, t_) for c in (0, 1, 3) for t_ in (False, True)}
    for case, (exp, n) in _tab_closed_forms(v).items():
        if case.startswith(("observed", "no referent")):
            share = pe.pooled_mass(exp, n)
            print(f"[{name}] {case}: at most {share:.3f} of a row's mass in the pooled cell")
            assert share <= 0.25, case


def test_tab_power_exact_samples_pass(tab_cases):
    name, variants = tab_cases
    rng = np.random.default_rng(11)
    for case, (exp, n) in _tab_closed_forms(variants["exact"]).items():
        res = pe.gof(_items(rng, exp, exp, n))
        print(f"[{name}] {case}: {pe.describe(res)}")
        assert res["p"] > pe.ALPHA, (case, pe.describe(res))


@pytest.mark.parametrize("mutation", ["a", "b", "c", "d"])
def test_tab_power_mutation_is_caught(tab_cases, mutation):
    """each mutated sampler fails pe.ALPHA on at least one case of the device leg, at the device leg's number of sweeps"""
    name, variants = tab_cases
    (key,) = [k for k in variants if k.startswith(mutation + ":")]
    exact, bad = _tab_closed_forms(variants["exact"]), _tab_closed_forms(variants[key])
    rng = np.random.default_rng(12)
    caught = []
    for case in exact:
        res = pe.gof(_items(rng, exact[case][0], bad[case][0], exact[case][1]))
        if res["p"] < pe.ALPHA:
            caught.append(case)
            print(f"[{name}] {key} fails {case}: {pe.describe(res)}")
    assert caught, f"{key} passes every case of the {name} program"
