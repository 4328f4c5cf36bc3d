"""Latent sweeps that weigh chosen ProposalDummyValues: the float64 restatement and the closed forms of
tests/latent_dummy_program.py have to earn their place before the device is compared with them
(tests/test_gpu_latent_dummy.py), and the host side of the flag is checked where no GPU is needed.

  * the enumerable variant StringPrior(1, L <= 2): the enumerated strings carry all of the sampler's mass, and the
    oracle's C++ sampler never returns anything else;
  * the closed forms (MH and PG with P = 2, from an atom and from a drawn string) are distributions, and updates
    simulated by the MECHANISM — propose an option, draw the string letter by letter, weigh, accept — follow them;
  * power at the device test's draw count: the uncorrected kernel (every weight equal, what the sweeps do without the
    flag) is rejected with p < 1e-6, the bar of test_posterior_draws_cpu.py's mutations;
  * the pooled cell of every case stays below test_posterior_draws_cpu.py's cap of a quarter of the mass;
  * host logic: which choices are served, the `excl` convention, the recorded origin and the refusal of several ranks."""
import math
import types

import numpy as np
import pytest

import latent_dummy_program as ld
import posterior_exact as pe

N_DRAWS = ld.DIST_ROWS * ld.DIST_SWEEPS
POOL_CAP = 0.25  # tests/test_posterior_draws_cpu.py


def test_enumerated_strings_carry_all_of_the_prior_mass(oracle):
    for L in (1, 2):
        strings = ld.all_strings(L)
        assert len(strings) == (28 if L == 1 else 28 + 784)
        assert abs(math.fsum(strings.values()) - 1.0) <= 1e-12
    # ... and they are what the independent sampler returns: its alphabet is the enumeration's
    from pclean_amd import sampling
    got = sampling.random_string_prior_at(oracle.RandomOracle(), [sampling.dummy_seed(5, 3, p, 0) for p in range(1, 401)],
                                          list(range(400)), 1, 2)
    strings = ld.all_strings(2)
    assert all(s in strings for s in got) and {len(s) for s in got} == {1, 2}
    # the sampler's frequencies follow the enumerated probabilities (one coarse check: the first letter)
    first = {}
    for s in got:
        first[s[0]] = first.get(s[0], 0) + 1
    exp = {}
    for s, p in strings.items():
        exp[s[0]] = exp.get(s[0], 0.0) + p
    assert pe.gof([(0, exp, first)])["p"] > pe.ALPHA


def test_correction_of_the_placeholder_is_the_dummy_mass_alone():
    """c(placeholder) = -log m_d: the likelihood terms cancel exactly; c of a string that explains the evidence is larger"""
    S = ld.item_program([{"name": "ab"}], [(0, "ad", None, None), (0, "ad", None, None), (0, None, None, None)], ["ab", "c"], 2)
    ph = S["model"].classes["Item"].attr("name").dist.dummy_value()
    c_ph, tol = ld.slot_correction(S, "name", 0, ph, False)
    assert abs(c_ph + ld.dummy_mass_log(S, "name")) <= tol
    assert ld.evidence_counts(S, "name", 0) == [(None, {"ad": 2})]  # multiplicity 2, the missing observation left out
    c_ad, _ = ld.slot_correction(S, "name", 0, "ad", False)
    want = -ld.dummy_mass_log(S, "name") + 2 * (ld.lit.add_typos_logpdf("ad", "ad") - ld.lit.add_typos_logpdf("ad", ph))
    assert abs(c_ad - want) <= 1e-12 and c_ad > c_ph
    # the two distance flavours differ where a transposition is followed by an insertion ("ca" -> "abc")
    assert ld.lit.damerau_levenshtein("ca", "abc", False) == 2 and ld.lit.damerau_levenshtein("ca", "abc", True) == 3


@pytest.mark.parametrize("name,mh,state", ld.DIST_CASES, ids=[c[0] for c in ld.DIST_CASES])
def test_closed_forms_power_and_pooling(name, mh, state):
    ev = ld.dist_evidence()
    exact = ld.kernel(ld.DIST_ATOMS, ld.DIST_LEN, ev, state, mh)
    assert abs(math.fsum(exact.values()) - 1.0) <= 1e-12
    assert (state in ld.DIST_ATOMS) == (name.endswith("atom"))
    pooled = pe.pooled_mass([exact], N_DRAWS)
    print(f"{name}: {len(exact)} cells, pooled mass {pooled:.4f} at {N_DRAWS} draws")
    assert pooled <= POOL_CAP
    rng = np.random.default_rng(11)
    ok = pe.gof([(0, exact, ld.simulate(ld.DIST_ATOMS, ld.DIST_LEN, ev, state, mh, N_DRAWS, rng))])
    bad = pe.gof([(0, exact, ld.simulate(ld.DIST_ATOMS, ld.DIST_LEN, ev, state, mh, N_DRAWS, rng, corrected=False))])
    print(f"{name}: mechanism {pe.describe(ok)}\n{name}: uncorrected {pe.describe(bad)}")
    assert ok["p"] > pe.ALPHA, pe.describe(ok)
    assert bad["p"] < 1e-6, pe.describe(bad)
    # the uncorrected closed form is what the uncorrected mechanism follows (the mutation is the parent's kernel, not noise)
    flat = ld.kernel(ld.DIST_ATOMS, ld.DIST_LEN, ev, state, mh, corrected=False)
    again = pe.gof([(0, flat, ld.simulate(ld.DIST_ATOMS, ld.DIST_LEN, ev, state, mh, N_DRAWS, rng, corrected=False))])
    assert again["p"] > pe.ALPHA, pe.describe(again)


# ---- host logic --------------------------------------------------------------------------------------------------
def _two_leaf_program():
    latents = [{"name": "ab", "tag": "zz"}, {"name": "qq", "tag": "x"}, {"name": "c", "tag": "x"}]
    rows = [(0, "ad", "ad", "zy"), (1, "qq", None, "x"), (1, "q", "qq", None), (2, "c", "c", "x")]
    return ld.item_program(latents, rows, ["ab", "c"], 2, tag_atoms=["x", "y"], tag_len=3, second_max_typos=1,
                           extra={"name": ["qq"], "tag": ["zz"]})


def _served(lw, cname):
    from pclean_amd.engine import Engine
    return Engine.latent_dummy_served(types.SimpleNamespace(lw=lw), cname)


def test_served_choices_are_reported():
    S = _two_leaf_program()
    assert _served(S["lw"], "Item") == ["name", "tag"]
    assert _served(S["lw"], "Obs") == []
    import helpers
    F = helpers.flights_setup()
    assert _served(F["lw"], "Flight") == []  # TimePrior choices: their MaybeSwap evidence reads a ctx slot
    R = helpers.rents_setup(n_rows=200)
    assert _served(R["lw"], "County") == []  # a keyed StringPrior


def test_excl_names_the_drawn_strings_rows_hold():
    from pclean_amd.engine import InferenceConfig
    from pclean_amd.inference import latent_current_choices
    S = _two_leaf_program()
    lw, tr = S["lw"], S["trace"]
    rows = np.arange(3)
    cfg = InferenceConfig(1, 2)
    pl = lw.latent_plans["Item"]
    assert (latent_current_choices(lw, tr, "Item", rows, cfg) == -1).all()  # flag off: as before
    excl = latent_current_choices(lw, tr, "Item", rows, cfg, ["name", "tag"])
    r_name, r_tag = pl["root_attr"].index("name"), pl["root_attr"].index("tag")
    assert excl[r_name].tolist() == [-1, ld.value_id(lw, "name", "qq"), -1]
    assert excl[r_tag].tolist() == [ld.value_id(lw, "tag", "zz"), -1, -1]
    only = latent_current_choices(lw, tr, "Item", rows, cfg, ["tag"])
    assert (only[r_name] == -1).all() and np.array_equal(only[r_tag], excl[r_tag])


def test_commit_records_the_origin_of_a_chosen_dummy():
    from pclean_amd.inference import commit_latent
    S = _two_leaf_program()
    lw, tr = S["lw"], S["trace"]
    pl = lw.latent_plans["Item"]
    nn = len(pl["nodes"])
    root = {a: pl["roots"][pl["root_attr"].index(a)] for a in ("name", "tag")}
    opt = {a: lw.option_values[("Item", a)] for a in ("name", "tag")}
    dummy = {a: int(np.flatnonzero(opt[a] == lw.latent_dom[("Item", a)].get(
        lw.model.classes["Item"].attr(a).dist.dummy_value()))[0]) for a in ("name", "tag")}
    vals = np.full((3, nn), -2, dtype=np.int32)
    vals[0, root["name"]], vals[0, root["tag"]] = dummy["name"], 0   # row 0: name takes the dummy
    vals[1, root["name"]], vals[1, root["tag"]] = 0, 1               # row 1: atoms only
    vals[2, root["name"]], vals[2, root["tag"]] = 0, dummy["tag"]    # row 2 keeps particle 0: nothing happens
    tr.row_origin[("Item", 1)] = (9, 9, 9, 0)  # an older record of a row that ends up holding no dummy
    commit_latent(lw, tr, "Item", np.arange(3), np.array([5, 1, 0]), vals, (["name", "tag"], 7))
    assert tr.row_origin == {("Item", 0): (0, 5, 7, pl["block_id"])}
    # without the flag nothing is recorded
    S2 = _two_leaf_program()
    commit_latent(S2["lw"], S2["trace"], "Item", np.arange(3), np.array([5, 1, 0]), vals)
    assert S2["trace"].row_origin == {}


def test_more_than_one_rank_is_refused():
    from pclean_amd.engine import InferenceConfig
    from pclean_amd.inference import latent_sweep, run_inference
    S = _two_leaf_program()
    eng = types.SimpleNamespace(lw=S["lw"])
    comm = types.SimpleNamespace(rank=0, world=2)
    with pytest.raises(NotImplementedError):
        latent_sweep(eng, S["trace"], "Item", InferenceConfig(1, 2), 1, 0, comm=comm, dummy_correction=True)
    with pytest.raises(NotImplementedError):
        run_inference(eng, S["trace"], InferenceConfig(1, 2), 1, comm=comm, latent_dummy_correction=True)
