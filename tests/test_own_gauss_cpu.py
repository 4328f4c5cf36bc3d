"""Gaussian observations in an own block of a flat class, on the host: the lowering (the leaf's place, grid, term order,
own_leaf, specs, derived columns; every refusal by name), the fixed-point quantiser of the sufficient statistics
(include/pclean_ownq.h: a stand-alone program under sanitizers, and against its NumPy restatement), the parameter move from
statistics, the encoding of the joint leaf in Trace.own, and the exact conditional the device tests compare with."""
import math
import os
import subprocess

import numpy as np
import pytest

import own_gauss_program as ogp
import posterior_exact as pe
from pclean_amd import _lib
from pclean_amd.model import (AddNoise, AddTypos, ChooseProportionally, ChooseUniformly, IndexedLookup, IndexedMeanParameter,
                              IndexedProportionsParameter, LoweredModel, Model, ProportionsParameter, Query, Transformation,
                              TransformedGaussian, Unmodeled)
from pclean_amd.trace import MeanTableState, Trace

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "own_gauss_host", "own_gauss_host.cpp")


# ---- lowering ---------------------------------------------------------------------------------------------------------
def test_lowering_unit_only_with_a_constant_index_mean():
    S = ogp.gauss_case(0, 2, n_rows=40)
    lw, _ = ogp.lower(S)
    assert lw.flat and len(lw.blocks) == 1
    blk = lw.blocks[0]
    assert len(blk["nodes"]) == 1 and blk["nodes"][0][0] == _lib.NODE_LEAF and blk["nodes"][0][3] == 0  # no string term
    leaf = lw.own_gauss[(0, 0)]
    assert leaf["factors"] == ["unit"] and leaf["sizes"] == [2] and leaf["cols"].tolist() == [[0, 1]]
    assert leaf["table"] == blk["nodes"][0][1]
    assert lw.own_leaf == {"unit": (0, 0)} and lw.own_product == {}
    (spec,) = leaf["specs"]
    assert spec["kinds"] == [] and spec["n_mean"] == 1 and spec["transform"] == ("local", 0) and spec["n_locals"] == 1
    assert spec["t_scale"] == [1.0, 1000.0] and spec["t_lad"][0] == 0.0 and math.isclose(spec["t_lad"][1], -math.log(1000.0))
    assert spec["mean_table"] == 0 and spec["leaf"] == (0, 0) and spec["term"] == 0 and lw.gauss_specs == [spec]
    assert lw.num_cols == ["Rent"] and lw.num_derived == []


def test_lowering_room_by_unit_with_typos_and_a_nonlinear_unit():
    S = ogp.gauss_case(3, 4, n_rows=40, nonlinear=True)
    lw, _ = ogp.lower(S)
    blk = lw.blocks[0]
    assert len(blk["nodes"]) == 1, "the factors are ONE leaf"
    kind, table, tb, nt = blk["nodes"][0][:4]
    assert (kind, tb, nt) == (_lib.NODE_LEAF, 0, 1)
    assert blk["terms"][0][0] == lw.obs_index["room_obs"] and blk["terms"][0][1] == 0  # the AddTypos term on option column 0
    assert blk["terms"][0][3] == _lib.DENS_ADD_TYPOS
    leaf = lw.own_gauss[(0, 0)]
    assert leaf["factors"] == ["room", "unit"] and leaf["sizes"] == [3, 4] and table == leaf["table"] != lw.option_id[("Obs", "room")]
    assert leaf["cols"].tolist() == [[0] * 4 + [1] * 4 + [2] * 4, [0, 1, 2, 3] * 3], "the grid a * |B| + b, key-major"
    assert lw.own_leaf == {"room": (0, 0), "unit": (0, 0)} and lw.own_product == {"unit": "room"}
    assert blk["node_info"][0]["gauss"] == ("room", "unit") and blk["node_info"][0]["attr"] == "unit"
    (spec,) = leaf["specs"]
    assert spec["kinds"] == [("local", 0)] and spec["strides"] == [1] and spec["n_mean"] == 3 and spec["transform"] == ("local", 1)
    assert spec["t_linear"] == [True, True, True, False]
    # the non-linear unit reads two derived numeric columns behind the observed one
    assert spec["t_x_col"] == [-1, -1, -1, 1] and spec["t_lad_col"] == [-1, -1, -1, 2]
    assert [(s, w) for s, _, w in lw.num_derived] == [(0, "backward"), (0, "logabsderiv")] and lw.xnum.shape[0] == 3
    x = lw.xnum[0]
    ok = ~np.isnan(x)
    assert np.allclose(lw.xnum[1][ok], np.sqrt(1000.0 * x[ok])) and np.isnan(lw.xnum[1][~ok]).all()
    # the leaf stands at the place of the factor declared last: another own choice declared between the two comes first
    tr = Trace(lw, S["n_rows"], 0)
    assert [a for a, _, _ in tr.own_leaves()] == ["room", "unit"] and tr.own_device_leaves() == [(0, 0, (0, 1))]
    assert len(tr.mean_params) == 1 and tr.has_learned_parameters("Obs")


def test_lowering_directly_observed_room_and_two_terms():
    S = ogp.gauss_case(3, 2, n_rows=40, typos=True, direct=True, second="room")
    lw, _ = ogp.lower(S)
    blk = lw.blocks[0]
    assert blk["nodes"][0][2:4] == (0, 2)
    t_typos, t_eq = blk["terms"]
    assert t_typos[0] == lw.obs_index["room_obs"] and t_eq[0] == lw.obs_index["room"], "the equality term comes last"
    assert (t_typos[1], t_typos[3], t_eq[1], t_eq[3]) == (0, _lib.DENS_ADD_TYPOS, 0, _lib.DENS_EQUAL)
    leaf = lw.own_gauss[(0, 0)]
    assert [s["gauss_attr"] for s in leaf["specs"]] == ["rent", "fee"] and [s["mean_table"] for s in leaf["specs"]] == [0, 1]
    assert [s["term"] for s in leaf["specs"]] == [0, 1]
    assert leaf["specs"][1]["transform"] == ("none", -1) and leaf["specs"][1]["kinds"] == [("local", 0)]
    assert [s["param"] for s in lw.gauss_specs] == [("Obs", "avg"), ("Obs", "avg2")]
    assert len(Trace(lw, 40, 0).mean_params) == 2


def _model(build, bind, dirty):
    m = Model()
    o = m.add_class("Obs")
    o.param("p", ProportionsParameter(1.0))
    o.param("q", ProportionsParameter(1.0))
    o.param("theta", IndexedProportionsParameter(1.0))
    o.param("avg", IndexedMeanParameter(0.0, 10.0))
    o.param("avg2", IndexedMeanParameter(0.0, 10.0))
    build(m, o)
    return LoweredModel(m, Query(m, "Obs", bind), dirty)


U2 = ogp.make_units(2)
ROWS = {"R": ["ab", "cd"], "X": [1.0, 2.0], "Y": [1.0, None], "C": ["x", "y"]}


def _refused(build, bind, match, cols=("R", "X")):
    with pytest.raises(NotImplementedError, match=match):
        _model(build, bind, {c: ROWS[c] for c in cols})


def test_refusals_by_name():
    def observed_index(m, o):
        with o.block():
            o.choice("room", ChooseProportionally(["ab", "cd"], "p"))
            o.choice("c", Unmodeled())
            o.julia("base", IndexedLookup("avg"), ["c"])
            o.choice("x", AddNoise("base", 1.0))
    # (a directly observed column that is no enumerated choice cannot stand in a flat class at all: refused where it is declared)
    _refused(observed_index, {"R": "room", "C": "c", "X": "x"}, "Obs.c: a Unmodeled choice in a block without a reference slot",
             cols=("R", "C", "X"))

    def index_in_another_block(m, o):
        with o.block():
            o.choice("kind", ChooseProportionally(["k", "l"], "q"))
        with o.block():
            o.choice("room", ChooseProportionally(["ab", "cd"], "p"))
            o.julia("base", IndexedLookup("avg"), ["kind"])
            o.choice("x", AddNoise("base", 1.0))
    _refused(index_in_another_block, {"R": "room", "X": "x"}, "mean index kind is declared in another block")

    def julia_index(m, o):
        with o.block():
            o.choice("room", ChooseProportionally(["ab", "cd"], "p"))
            o.julia("up", lambda r: r.upper(), ["room"])
            o.julia("base", IndexedLookup("avg"), ["up"])
            o.choice("x", AddNoise("base", 1.0))
    _refused(julia_index, {"R": "room", "X": "x"}, "mean index up is a JuliaNode")

    def behind_reference(m, o):
        with o.block():
            o.choice("room", ChooseProportionally(["ab", "cd"], "p"))
            o.julia("base", IndexedLookup("avg"), ["other.room"])
            o.choice("x", AddNoise("base", 1.0))
    _refused(behind_reference, {"R": "room", "X": "x"}, "lies behind a reference")

    def two_strings(m, o):
        with o.block():
            o.choice("room", ChooseProportionally(["ab", "cd"], "p"))
            o.choice("kind", ChooseProportionally(["k", "l"], "q"))
            o.julia("base", IndexedLookup("avg"), ["room", "kind"])
            o.choice("x", AddNoise("base", 1.0))
    _refused(two_strings, {"R": "room", "X": "x"}, "two string factors")

    def two_units(m, o):
        with o.block():
            o.choice("room", ChooseProportionally(["ab", "cd"], "p"))
            o.choice("u1", ChooseUniformly(U2))
            o.choice("u2", ChooseUniformly(U2))
            o.julia("base", IndexedLookup("avg"), ["room"])
            o.julia("base2", IndexedLookup("avg2"), ["room"])
            o.choice("x", TransformedGaussian("base", 1.0, "u1"))
            o.choice("y", TransformedGaussian("base2", 1.0, "u2"))
    _refused(two_units, {"R": "room", "X": "x", "Y": "y"}, "more than two factors", cols=("R", "X", "Y"))

    def indexed_factor(m, o):
        with o.block():
            o.choice("kind", ChooseProportionally(["k", "l"], "q"))
            o.choice("room", ChooseProportionally(["ab", "cd"], "theta", index="kind"))
            o.julia("base", IndexedLookup("avg"), ["room"])
            o.choice("x", AddNoise("base", 1.0))
    _refused(indexed_factor, {"R": "room", "X": "x"}, "itself indexed, or that indexes")

    def indexing_factor(m, o):
        with o.block():
            o.choice("kind", ChooseProportionally(["k", "l"], "q"))
            o.choice("room", ChooseProportionally(["ab", "cd"], "theta", index="kind"))
            o.julia("base", IndexedLookup("avg"), ["kind"])
            o.choice("x", AddNoise("base", 1.0))
    _refused(indexing_factor, {"R": "room", "X": "x"}, "itself indexed, or that indexes")

    def grid_too_large(m, o):
        with o.block():
            o.choice("room", ChooseProportionally([f"w{i}" for i in range(2049)], "p"))
            o.choice("unit", ChooseUniformly(U2))
            o.julia("base", IndexedLookup("avg"), ["room"])
            o.choice("x", TransformedGaussian("base", 1.0, "unit"))
    _refused(grid_too_large, {"X": "x"}, "4098 options, more than the 4096", cols=("X",))

    def shared_parameter(m, o):
        with o.block():
            o.choice("room", ChooseProportionally(["ab", "cd"], "p"))
            o.julia("base", IndexedLookup("avg"), ["room"])
            o.julia("base2", IndexedLookup("avg"), ["room"])
            o.choice("x", AddNoise("base", 1.0))
            o.choice("y", AddNoise("base2", 1.0))
    _refused(shared_parameter, {"R": "room", "X": "x", "Y": "y"}, "only one Gaussian observation per block may read",
             cols=("R", "X", "Y"))

    def mean_is_no_lookup(m, o):
        with o.block():
            o.choice("room", ChooseProportionally(["ab", "cd"], "p"))
            o.julia("base", lambda r: 1.0, ["room"])
            o.choice("x", AddNoise("base", 1.0))
    _refused(mean_is_no_lookup, {"R": "room", "X": "x"}, "must be an IndexedLookup of an IndexedMeanParameter")

    def five_units(m, o):
        with o.block():
            o.choice("unit", ChooseUniformly(ogp.make_units(4) + ogp.make_units(1)))
            o.julia("base", IndexedLookup("avg"), [])
            o.choice("x", TransformedGaussian("base", 1.0, "unit"))
    _refused(five_units, {"X": "x"}, "more than 4 units", cols=("X",))

    def with_a_slot(m, o):
        a = m.classes  # (the latent class has to exist before the slot)
        del a
        with o.block():
            o.fk("r", "A")
            o.choice("r_obs", AddTypos("r.name"))
        with o.block():
            o.choice("room", ChooseProportionally(["ab", "cd"], "p"))
            o.julia("base", IndexedLookup("avg"), ["room"])
            o.choice("x", AddNoise("base", 1.0))

    def build_with_latent():
        m = Model()
        a = m.add_class("A")
        a.param("ap", ProportionsParameter(1.0))
        a.choice("name", ChooseProportionally(["ab", "cd"], "ap"))
        o = m.add_class("Obs")
        o.param("p", ProportionsParameter(1.0))
        o.param("avg", IndexedMeanParameter(0.0, 10.0))
        with_a_slot(m, o)
        return LoweredModel(m, Query(m, "Obs", {"R": ("r.name", "r_obs"), "X": "x"}), {c: ROWS[c] for c in ("R", "X")})
    with pytest.raises(NotImplementedError, match="own blocks are served for flat classes alone"):
        build_with_latent()


def test_a_column_not_reported_through_a_julia_node_of_the_observation_is_refused():
    def served(m, o):
        with o.block():
            o.choice("room", ChooseProportionally(["ab", "cd"], "p"))
            o.julia("base", IndexedLookup("avg"), ["room"])
            o.choice("x", AddNoise("base", 1.0))
            o.julia("x_clean", lambda x: round(x), ["x"])
            o.julia("other", lambda r: r, ["room"])
    lw = _model(served, {"R": "room", "X": ("x_clean", "x")}, {c: ROWS[c] for c in ("R", "X")})
    assert lw.own_gauss[(0, 0)]["factors"] == ["room"]
    for clean in ("x", "base", "other"):  # the raw number, the mean lookup, a JuliaNode that does not read the observation
        _refused(served, {"R": "room", "X": (clean, "x")},
                 r"Obs\.x: a Gaussian observation in a block without a reference slot is lowered only when the query reports")


def test_several_ranks_and_prior_proposals_are_refused_by_name():
    from pclean_amd import inference as inf
    from pclean_amd.engine import Engine, InferenceConfig

    class Comm:
        world, rank = 2, 0
    S = ogp.gauss_case(2, 2, n_rows=8)
    lw, _ = ogp.lower(S)

    class Eng:
        pass
    e = Eng()
    e.lw = lw
    with pytest.raises(NotImplementedError, match="swept by one rank"):
        inf.initialize_trace(e, Trace(lw, 8, 0), InferenceConfig(1, 2), 0, comm=Comm())
    e.sweep_own = Engine.sweep_own.__get__(e)
    with pytest.raises(NotImplementedError, match="use_dd_proposals=False"):
        e.sweep_own(Trace(lw, 8, 0), InferenceConfig(1, 2, use_dd_proposals=False), 0, 0)


# ---- the quantiser ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("own_gauss_host") / "own_gauss_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    return exe


def test_quantiser_under_sanitizers(host_exe):
    out = subprocess.run([host_exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-3000:])
    lines = out.stdout.splitlines()
    assert lines[-1] == "all cases passed" and "cases 13" in lines, lines[-3:]
    assert "ok n 2147483647 M 1e+15 e -19" in lines and "ok n 1 M 1e-300 e 40" in lines and "ok n 1048576 M 0 e 40" in lines


@pytest.mark.parametrize("e", [40, 17, 0, -19])
def test_quantiser_agrees_with_numpy(host_exe, e):
    rng = np.random.default_rng(e + 100)
    big = 2.0 ** (61 - e - 14)  # (10^4 values: their quantised magnitudes stay below 2^47)
    x = np.concatenate([rng.normal(0.0, big / 4, 9000), rng.uniform(-big, big, 990),
                        (rng.integers(-50, 50, 10) + 0.5) * 2.0 ** -e])  # exact ties
    text = "\n".join(f"{int(v):x}" for v in x.view(np.uint64)) + "\n"
    out = subprocess.run([host_exe, "quantise", str(e)], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = np.array([int(s) for s in out.stdout.split()], dtype=np.int64)
    want = np.rint(x * 2.0 ** e).astype(np.int64)
    assert len(got) == len(x) == 10000 and np.array_equal(got, want)
    assert (np.abs((want[-10:] % 2)) == 0).all(), "ties go to even"
    err = abs(sum(int(q) for q in want) / 2.0 ** e - math.fsum(x))
    assert err <= len(x) * 2.0 ** (-e - 1)


def test_python_exponent_restates_the_header(host_exe):
    """Trace.own_gauss_exponent on a program == the rule of the header (the program's own check is in the host program)"""
    S = ogp.gauss_case(3, 2, n_rows=50)
    lw, _ = ogp.lower(S)
    tr = Trace(lw, 50, 0)
    x = np.array([v for v in S["dirty"]["Rent"] if v is not None])
    big = max(np.abs(x).max(), np.abs(x * 1000.0).max())
    assert tr.own_gauss_exponent(0) == min(40, 62 - math.frexp(big)[1] - (50).bit_length())


# ---- the parameter move and the encoding ------------------------------------------------------------------------------
def test_resample_from_stats_equals_resample_on_integers():
    rng = np.random.default_rng(3)
    idx = rng.integers(0, 5, 400)
    bx = rng.integers(-3000, 3000, 400).astype(np.float64)  # exactly representable: the fixed-point sum is the float sum
    a = MeanTableState(5, 1500.0, 1000.0, 150.0, np.random.default_rng(0))
    b = MeanTableState(5, 1500.0, 1000.0, 150.0, np.random.default_rng(0))
    a.resample(np.random.default_rng(9), idx, bx)
    e = 40
    q = np.zeros(5, dtype=np.int64)
    np.add.at(q, idx, np.rint(bx * 2.0 ** e).astype(np.int64))
    b.resample_from_stats(np.random.default_rng(9), np.bincount(idx, minlength=5), q.astype(np.float64) / 2.0 ** e)
    assert np.array_equal(a.value.view(np.uint64), b.value.view(np.uint64))


def test_host_route_of_the_parameter_move():
    S = ogp.gauss_case(3, 2, n_rows=200, second="room")
    lw, _ = ogp.lower(S)
    tr = Trace(lw, 200, 0)
    own = np.array(S["truth"], dtype=np.int32).T.copy()
    own[:, 190:] = -1
    tr.own = own
    tr.resample_parameters()
    tr.check_consistency()
    assert np.array_equal(tr.params[("Obs", "p")].counts, np.bincount(own[0, :190], minlength=3))
    for g in (0, 1):
        count, qsum, e = tr.own_gauss_stats(g)
        c2, q2 = ogp.numpy_stats(S, lw, np.where(own[0] < 0, -1, own[0] * 2 + own[1]), g, e)
        assert np.array_equal(count, c2) and np.array_equal(qsum, q2) and e == tr.own_gauss_exponent(g)
    # the truth's units undo the transformation: the posterior means sit at the generating ones
    n, q, e = tr.own_gauss_stats(0)
    assert np.allclose(q / 2.0 ** e / n, S["mu"], atol=5 * ogp.SIGMA / np.sqrt(n.min()))


def test_trace_own_round_trips_the_joint_leaf():
    S = ogp.gauss_case(3, 4, n_rows=30)
    lw, _ = ogp.lower(S)
    tr = Trace(lw, 30, 0)
    rng = np.random.default_rng(1)
    own = np.stack([rng.integers(0, 3, 30), rng.integers(0, 4, 30)]).astype(np.int32)
    own[:, 5] = -1
    tr.own = own
    joint = tr.own_joint(tr._own, 0, 1)
    assert joint[5] == -1 and np.array_equal(joint[own[0] >= 0], (own[0] * 4 + own[1])[own[0] >= 0])
    a, b = tr.own_split(joint, 1)
    assert np.array_equal(a, own[0]) and np.array_equal(b, own[1])
    assert np.array_equal(tr.own_counts(0), np.bincount(own[0][own[0] >= 0], minlength=3))
    assert np.array_equal(tr.own_counts(1), np.bincount(own[1][own[1] >= 0], minlength=4))
    own[1, 7] = -1
    with pytest.raises(ValueError, match="only one of the own choices room and unit is set"):
        tr.own_joint(own, 0, 1)


# ---- the exact conditional ------------------------------------------------------------------------------------------
def test_exact_conditional_and_its_float64_draws_pass_the_goodness_of_fit():
    S, pis = ogp.dist_case()
    for i in (0, 3, 5, 27):
        s, mag = ogp.exact_scores(S, i)
        assert s.shape == (6,) and np.isfinite(s).all() and (mag >= np.abs(s) - 1e-9).all()
        assert math.isclose(sum(pis[i].values()), 1.0, rel_tol=1e-12)
    # a row whose number is missing does not tell the units apart
    i = next(i for i in range(S["n_rows"]) if S["dirty"]["Rent"][i] is None and S["dirty"]["RoomObs"][i] is not None)
    assert all(math.isclose(pis[i][2 * a], pis[i][2 * a + 1], rel_tol=1e-12) for a in range(3))
    assert max(len([v for v in pi.values() if v > 0.01]) for pi in pis) >= 3, "the case does not spread"
    rng = np.random.default_rng(ogp.DIST_SEED)
    items = []
    for i, pi in enumerate(pis):
        keys = list(pi)
        cnt = rng.multinomial(ogp.S_DRAWS, np.array([pi[k] for k in keys]))
        items.append((i, pi, {k: int(c) for k, c in zip(keys, cnt) if c}))
    res = pe.gof(items)
    assert res["p"] > pe.ALPHA, pe.describe(res)
    # ... and draws from another distribution (the units swapped) do not
    bad = [(i, pi, {k ^ 1: c for k, c in obs.items()}) for i, pi, obs in items]
    assert pe.gof(bad)["p"] < pe.ALPHA
