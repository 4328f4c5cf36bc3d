"""IndexedProportionsParameter in its keyed form (the index observed directly) and NumberCodePrior, on the CPU: the
lowering (options, key column, equality term, refusals), the parameter state ([key][option] counts through host commits
against a brute-force recount, resample against a key-by-key restatement), the number-code densities, and the power of
the exact-posterior restatement of tests/indexed_program.py against a twin that reads theta from the wrong key."""
import math

import numpy as np
import pytest

import indexed_program as ip
import posterior_exact as pe
from pclean_amd import _lib
from pclean_amd.engine import number_code_logp
from pclean_amd.inference import commit_latent
from pclean_amd.model import (AddTypos, ChooseProportionally, ChooseUniformly, IndexedProportionsParameter, LoweredModel,
                              Model, NumberCodePrior, ProportionsParameter, Query, StringPrior, Unmodeled)
from pclean_amd.parallel import Comm, exchange_and_commit
from pclean_amd.trace import IndexedProportionsState, Trace


@pytest.fixture(scope="module")
def prog():
    return ip.draw_program()


# ---- lowering ---------------------------------------------------------------------------------------------------------
def test_keyed_options_and_equality_term(prog):
    lw = prog["lw"]
    assert lw.indexed == {("Doc", "city"): ("keyed", "state")}
    nk, nb = len(lw.latent_dom[("Doc", "state")]), len(ip.CITIES)
    assert nk == len(ip.STATES)
    vals, keys = lw.option_values[("Doc", "city")], lw.option_keycol[("Doc", "city")]
    assert np.array_equal(vals, np.tile(np.arange(nb), nk)) and np.array_equal(keys, np.repeat(np.arange(nk), nb))
    blk = lw.blocks[0]
    (leaf,) = [i for i, info in enumerate(blk["node_info"]) if info["kind"] == "leaf" and info["attr"] == "city"]
    node = blk["nodes"][leaf]
    assert node[1] == lw.option_id[("Doc", "city")] and node[8] == 0  # (two terms: no per-observed-value cache)
    terms = blk["terms"][node[2]:node[2] + node[3]]
    # the AddTypos term on the value column, then the equality term of the observed key on the key column
    assert [(t[0], t[1], t[3]) for t in terms] == [(lw.obs_index["city_obs"], 0, _lib.DENS_ADD_TYPOS),
                                                   (lw.obs_index["d.state"], 1, _lib.DENS_EQUAL)]
    assert terms[1][2] == lw.eq_pairs[("eq", ("Doc", "state"))][0]
    # a new row's columns come from column 0 of the three leaves
    assert blk["colmap"] == [1, 0, 2, 0, 3, 0]
    pl = lw.latent_plans["Doc"]
    assert pl["root_attr"] == ["npi", "state", "city"]
    lt = pl["terms"][pl["nodes"][2][2]:pl["nodes"][2][2] + pl["nodes"][2][3]]
    assert [(t[1], t[3]) for t in lt] == [(0, _lib.DENS_ADD_TYPOS), (1, _lib.DENS_EQUAL)]


def _lower(build, dirty=None, cls="Obs", bind=None):
    m = Model()
    build(m)
    dirty = dirty or {"K": ["x", "y"], "V": ["a", "b"]}
    return LoweredModel(m, Query(m, cls, bind or {"K": "d.k", "V": ("d.v", "v_obs")}), dirty)


def _doc(m, k_dist, v_index="k", prior=None, more=None, blocks=False):
    d = m.add_class("Doc")
    d.param("theta", prior or IndexedProportionsParameter())
    if blocks:
        with d.block():
            d.choice("k", k_dist)
        with d.block():
            d.choice("v", ChooseProportionally(["a", "b"], "theta", index=v_index))
    else:
        d.choice("k", k_dist)
        if more:
            more(d)
        d.choice("v", ChooseProportionally(["a", "b"], "theta", index=v_index))
    o = m.add_class("Obs")
    o.fk("d", "Doc")
    o.choice("v_obs", AddTypos("d.v"))
    return d


def test_refusals_name_the_attribute():
    def school(m):
        s = m.add_class("School")
        s.choice("name", Unmodeled())
        d = m.add_class("Doc")
        d.param("theta", IndexedProportionsParameter())
        d.fk("school", "School")
        d.choice("v", ChooseProportionally(["a", "b"], "theta", index="school.name"))
        o = m.add_class("Obs")
        o.fk("d", "Doc")
        o.choice("v_obs", AddTypos("d.v"))
    with pytest.raises(NotImplementedError, match=r"Doc\.v: an index reached through a reference \(school\.name\)"):
        _lower(school, bind={"K": "d.school.name", "V": ("d.v", "v_obs")})

    def julia(m):
        d = _doc(m, Unmodeled(), v_index="j", more=lambda d: d.julia("j", lambda k: k, ["k"]))
    with pytest.raises(NotImplementedError, match=r"Doc\.v: a JuliaNode index \(j\)"):
        _lower(julia)

    def own(m):
        d = m.add_class("Doc")
        d.choice("k", Unmodeled())
        o = m.add_class("Obs")
        o.param("theta", IndexedProportionsParameter())
        o.fk("d", "Doc")
        o.choice("u", ChooseUniformly(["a", "b"]))
        o.choice("w", ChooseProportionally(["a", "b"], "theta", index="u"))
    with pytest.raises(NotImplementedError, match=r"Obs\.w: an indexed choice among the observed class's own choices"):
        _lower(own, dirty={"K": ["x"]}, bind={"K": "d.k"})

    def chain(m):
        _doc(m, Unmodeled(), v_index="mid",
             more=lambda d: d.choice("mid", ChooseProportionally(["p", "q"], "theta", index="k")))
    with pytest.raises(NotImplementedError, match=r"Doc\.v: the index mid is itself indexed"):
        _lower(chain)

    def two(m):
        d = _doc(m, Unmodeled(), more=lambda d: (d.param("t2", IndexedProportionsParameter()),
                                               d.choice("v0", ChooseProportionally(["p", "q"], "t2", index="k"))))
    with pytest.raises(NotImplementedError, match=r"Doc\.v: k already indexes v0; two dependents on one index"):
        _lower(two)

    with pytest.raises(NotImplementedError, match=r"Doc\.v: the index k is declared in another block"):
        _lower(lambda m: _doc(m, Unmodeled(), blocks=True))

    def huge(m):
        d = m.add_class("Doc")
        d.param("theta", IndexedProportionsParameter())
        d.choice("k", ChooseUniformly(range(70000)))
        d.choice("v", ChooseProportionally(range(70000), "theta", index="k"))
        o = m.add_class("Obs")
        o.fk("d", "Doc")
    with pytest.raises(NotImplementedError, match=r"Doc\.v: the product with k has 70000 x 70000 options, more than 2\^31 - 1"):
        _lower(huge, dirty={"K": ["x"]}, bind={"K": "d.k"})

    # a sibling index whose options are no strings has no latent domain to take column 0 from
    with pytest.raises(NotImplementedError, match=r"Doc\.v: the options of the index k are not strings"):
        _lower(lambda m: _doc(m, ChooseUniformly([1, 2])), dirty={"V": ["a", "b"]}, bind={"V": ("d.v", "v_obs")})
    with pytest.raises(NotImplementedError, match=r"Doc\.v: the index k must be declared before the choice"):
        def late(m):
            d = m.add_class("Doc")
            d.param("theta", IndexedProportionsParameter())
            d.choice("v", ChooseProportionally(["a", "b"], "theta", index="k"))
            d.choice("k", ChooseUniformly(["x", "y"]))
            o = m.add_class("Obs")
            o.fk("d", "Doc")
            o.choice("v_obs", AddTypos("d.v"))
        _lower(late, dirty={"V": ["a", "b"]}, bind={"V": ("d.v", "v_obs")})
    # an index that is neither a sibling categorical choice nor observed
    with pytest.raises(NotImplementedError, match=r"Doc\.v: the index k is neither"):
        _lower(lambda m: _doc(m, StringPrior(1, 3, ["x", "y"])), dirty={"V": ["a", "b"]}, bind={"V": ("d.v", "v_obs")})
    with pytest.raises(NotImplementedError, match=r"Doc\.v: the index k is observed through d\.k, which has missing values"):
        _lower(lambda m: _doc(m, Unmodeled()), dirty={"K": ["x", None], "V": ["a", "b"]})

    def between(m):
        from pclean_amd.model import StringPrior as SP
        _doc(m, ChooseUniformly(["x", "y"]), more=lambda d: d.choice("nick", SP(1, 5, {"x": ["p"], "y": ["q"]}, keyed_by="k")))
    with pytest.raises(NotImplementedError, match=r"Doc\.v: nick, declared between the index k and the choice, reads the index"):
        _lower(between, dirty={"V": ["a", "b"]}, bind={"V": ("d.v", "v_obs")})
    with pytest.raises(ValueError, match=r"Doc\.v: index='k' needs an IndexedProportionsParameter"):
        _lower(lambda m: _doc(m, Unmodeled(), prior=ProportionsParameter()))
    with pytest.raises(ValueError, match=r"Doc\.v: the IndexedProportionsParameter theta needs index"):
        _lower(lambda m: _doc(m, Unmodeled(), v_index=None))


# ---- NumberCodePrior ----------------------------------------------------------------------------------------------------
def test_number_code_logp():
    codes = ["1", "7", "1234567893"]
    got = number_code_logp(codes)
    assert got.dtype == np.float64 and np.array_equal(got, -np.log(np.array([1.0, 7.0, 1234567893.0])))
    assert got[0] == 0.0 and (got <= 0).all()


@pytest.mark.parametrize("bad", ["0", "-3", "12a"])
def test_number_code_rejects(bad):
    with pytest.raises(ValueError, match=rf"NPI: value '{bad}' is not a decimal integer >= 1"):
        m = ip.model()
        LoweredModel(m, ip.query(m), {"NPI": ["5", bad], "State": ["CA", "NY"], "City": ["albany", None]})
    with pytest.raises(ValueError, match="is not a decimal integer >= 1"):
        number_code_logp([bad])


def test_number_code_must_be_observed():
    m = ip.model()
    q = Query(m, "Obs", {"State": "d.state", "City": ("d.city", "city_obs")})
    with pytest.raises(ValueError, match=r"Doc\.npi: a NumberCodePrior value must be observed directly"):
        LoweredModel(m, q, {"State": ["CA"], "City": ["albany"]})


# ---- parameter state ----------------------------------------------------------------------------------------------------
def _brute_counts(S, tr):
    """[state][city] counts over the live Doc rows, from the strings"""
    lw = S["lw"]
    t, ci = tr.tables["Doc"], lw.colidx["Doc"]
    kdom, vdom = lw.latent_dom[("Doc", "state")], lw.latent_dom[("Doc", "city")]
    out = np.zeros((len(kdom), len(ip.CITIES)), dtype=np.int64)
    for r in range(t.n):
        if t.live[r]:
            st, city = kdom.string(int(t.cols[ci["state"], r])), vdom.string(int(t.cols[ci["city"], r]))
            out[[kdom.string(k) for k in range(len(kdom))].index(st), ip.CITIES.index(city)] += 1
    return out


def test_counts_follow_host_commits():
    """rows created (single and bulk), references moved, rows collected, values changed by a latent commit: the
    [key][option] counts equal a recount over the live rows after every step"""
    S = ip.draw_program(seed=3)
    lw, tr = S["lw"], S["trace"]
    state = tr.params[("Doc", "theta")]
    assert isinstance(state, IndexedProportionsState) and state.counts.shape == (len(ip.STATES), len(ip.CITIES))
    assert np.array_equal(state.counts, _brute_counts(S, tr)) and state.counts.sum() == len(S["ents"])
    rng = np.random.default_rng(0)
    n = tr.cur.shape[1]
    nk, nb, nc = len(ip.STATES), len(ip.CITIES), len(lw.latent_dom[("Doc", "npi")])
    t = tr.tables["Doc"]
    created = collected = 0
    for step in range(6):
        live = np.flatnonzero(t.live[:t.n])
        choice = tr.cur.copy()
        rows = rng.choice(n, size=25, replace=False)
        new = np.sort(rows[:10])
        choice[0, rows[10:]] = rng.choice(live, size=15)
        choice[0, new] = -1
        key = rng.integers(0, nk, size=10)
        vals = np.stack([np.full(10, -1), rng.integers(0, nc, size=10), key, key * nb + rng.integers(0, nb, size=10)], axis=1)
        before = (t.n, len(t.free), int(t.live[:t.n].sum()))
        if step % 2:
            tr.commit(choice, {0: (new.astype(np.int32), vals.astype(np.int32))})
        else:  # the product's host commit of a sweep (bulk inserts and deletes)
            ch, cur = choice[0], tr.cur[0]
            delta = (np.bincount(ch[(ch != cur) & (ch >= 0)], minlength=t.n) - np.bincount(cur[ch != cur], minlength=t.n)).astype(np.int64)
            exchange_and_commit(tr, lw, Comm(), 0, choice, {0: delta}, {0: (new.astype(np.int32), vals.astype(np.int32))},
                                global_cur=True, sweep_idx=step)
        created += 10
        collected += before[2] + 10 - int(t.live[:t.n].sum())
        tr.check_consistency()
        assert np.array_equal(state.counts, _brute_counts(S, tr)), step
        # a latent commit: every third live row takes fresh values of all three choices
        live = np.flatnonzero(t.live[:t.n]).astype(np.int32)
        chosen = (np.arange(len(live)) % 3 == 0).astype(np.int32)
        key = rng.integers(0, nk, size=len(live))
        lv = np.stack([rng.integers(0, nc, size=len(live)), key, key * nb + rng.integers(0, nb, size=len(live))], axis=1)
        assert commit_latent(lw, tr, "Doc", live, chosen, lv.astype(np.int32)) > 0
        tr.check_consistency()
        assert np.array_equal(state.counts, _brute_counts(S, tr)), step
    assert collected > 0 and len(t.free) + t.n > before[0] - 1
    assert np.array_equal(tr.recount("Doc", "city"), state.counts)


def test_created_vectors_and_resample_follow_the_restatement():
    S = ip.draw_program(seed=5)
    tr = S["trace"]
    conc = 0.7
    st = IndexedProportionsState(4, 7, conc, np.random.default_rng(11))
    ref = np.random.default_rng(11)
    want = np.stack([ref.dirichlet(np.full(7, conc)) for _ in range(4)])  # created in domain order
    assert np.array_equal(st.value, want)
    st.counts[:] = tr.params[("Doc", "theta")].counts
    st.resample(np.random.default_rng(12))
    ref = np.random.default_rng(12)
    want = np.stack([ref.dirichlet(conc + st.counts[k]) for k in range(4)])
    assert np.array_equal(st.value, want) and not np.array_equal(want[0], want[1])
    # Trace.resample_parameters reaches the indexed state with the trace's generator
    g = np.random.default_rng(0)
    g.bit_generator.state = tr.rng.bit_generator.state
    tr.resample_parameters("Doc")
    c = tr.params[("Doc", "theta")].counts
    assert np.array_equal(tr.params[("Doc", "theta")].value, np.stack([g.dirichlet(1.0 + c[k]) for k in range(4)]))


def test_joint_log_prior_is_key_major():
    """what Engine.upload_trace uploads for the keyed choice: log theta_key[option] in the options' order"""
    S = ip.draw_program()
    lw, tr = S["lw"], S["trace"]
    logp = np.log(tr.params[("Doc", "theta")].value).reshape(-1)
    vals, keys = lw.option_values[("Doc", "city")], lw.option_keycol[("Doc", "city")]
    th = ip.theta_by_string(S)
    kdom = lw.latent_dom[("Doc", "state")]
    for o in range(len(vals)):
        assert logp[o] == math.log(th[kdom.string(int(keys[o]))][ip.CITIES[int(vals[o])]])


# ---- the restatement tells the right key from the wrong one --------------------------------------------------------------
def expected_outputs(S, rows, P, theta=None):
    """closed-form output distribution (posterior_exact.pg_one_block) of each of `rows` under PG with P particles"""
    out = []
    for i in rows:
        pi = pe.normalise(ip.block_scores(S, int(i), theta))
        cur = int(S["trace"].cur[0, i])
        out.append(pe.pg_one_block(pi, None if cur < 0 else cur, P))
    return out


def test_restatement_rejects_theta_of_the_wrong_key():
    """draws sampled from the exact output distributions (S_GPU per row, as the device test draws) pass gof() at the
    device test's threshold against themselves and fail it against the twin whose theta is read one key further"""
    S = ip.draw_program()
    rows = np.arange(S["trace"].cur.shape[1])
    right = expected_outputs(S, rows, 5)
    wrong = expected_outputs(S, rows, 5, ip.theta_by_string(S, shift=1))
    rng = np.random.default_rng(1)
    items_r, items_w = [], []
    for i, e, w in zip(rows, right, wrong):
        keys = list(e)
        draws = rng.choice(len(keys), size=pe.S_GPU, p=np.array([e[k] for k in keys]) / sum(e.values()))
        obs = pe.tabulate([keys[j] for j in draws])
        items_r.append((int(i), e, obs))
        items_w.append((int(i), w, obs))
    assert pe.gof(items_r)["p"] > pe.ALPHA
    assert pe.gof(items_w)["p"] < pe.ALPHA
