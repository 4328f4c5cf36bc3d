"""AddNoise (add_noise.jl:1-7): lowering, refusals, and the C++ oracle's reading of the lowered spec — against the
TransformedGaussian twin with one identity unit (tests/addnoise_program.py) and against the written-out Normal density."""
import numpy as np
import pytest

import addnoise_program as ap
from pclean_amd._lib import InferConfig
from pclean_amd.engine import make_gauss
from pclean_amd.inference import build_evidence, latent_current_choices
from pclean_amd.model import LoweredModel

import helpers


def test_addnoise_lowering():
    S = ap.setup(ap.addnoise_model, 300)
    lw = S["lw"]
    spec = lw.gauss_spec
    assert spec["gauss_attr"] == "rent" and spec["param"] == ("Obs", "avg_rent")
    assert spec["locals"] == ["br"] and spec["local_n"] == [5] and spec["local_obs"] == [lw.obs_index["br"]]
    assert spec["t_local"] is None and spec["t_scale"] == [1.0] and spec["t_lad"] == [0.0]
    assert spec["t_x_col"] == [-1] and spec["t_lad_col"] == [-1] and spec["sigma"] == 150.0
    assert lw.locals == {0: ["br"]} and lw.xnum.shape == (1, 300) and not lw.num_derived
    root = lw.gauss[(0, 0)]
    assert root["n_locals"] == 1 and root["transform"] == ("none", -1)
    assert [k[0] for k in root["kinds"]] == ["cand", "cand", "local"]
    # the latent County plan: the evidence rows' br held at its current value, still no Transformation to choose
    lat = [g for (b, _), g in lw.gauss.items() if b == lw.latent_plans["County"]["block_id"]]
    assert len(lat) == 1 and lat[0]["n_locals"] == 0 and lat[0]["transform"] == ("none", -1)
    assert ("evctx", 0) in lat[0]["kinds"]
    g = make_gauss(root)
    assert (g.transform_src_kind, g.transform_src, g.n_locals) == (-1, -1, 1)
    assert list(g.t_scale) == [1.0] * 4 and list(g.t_logabsderiv) == [0.0] * 4 and list(g.t_x_col) == [-1] * 4
    # the host's backward(x) is x itself
    rows = np.flatnonzero(~np.isnan(lw.xnum[0]))[:20]
    assert np.array_equal(lw.gauss_backward(rows, np.zeros(len(rows), dtype=np.int32)), lw.xnum[0, rows])


def test_addnoise_with_a_candidate_side_mean_lowers_without_own_choices():
    """mean indexed by the referent's values alone: one combination per candidate, no own choices to track"""
    S = ap.setup(ap.candidate_mean_model, 300)
    lw, tr = S["lw"], S["trace"]
    root = lw.gauss[(0, 0)]
    assert root["n_locals"] == 0 and root["locals"] == [] and root["transform"] == ("none", -1)
    assert [k[0] for k in root["kinds"]] == ["cand", "cand"]
    assert lw.locals == {} and lw.gauss_block == 0 and lw.latent_ev_locals == {}
    lat = [g for (b, _), g in lw.gauss.items() if b == lw.latent_plans["County"]["block_id"]]
    assert len(lat) == 1 and lat[0]["n_locals"] == 0 and all(k[0] != "evctx" for k in lat[0]["kinds"])
    g = make_gauss(root)
    assert (g.n_locals, g.transform_src_kind) == (0, -1)
    rows, idx, x = tr.gaussian_index()
    ok = ~np.isnan(lw.xnum[0])
    assert np.array_equal(rows, np.flatnonzero(ok)) and np.array_equal(x, lw.xnum[0, ok])
    t = tr.tables["County"]
    st, ck = (t.cols[lw.colidx["County"][c], tr.cur[0, rows]] for c in ("state", "countykey"))
    assert np.array_equal(idx, root["strides"][0] * st + root["strides"][1] * ck)


def test_addnoise_refusals():
    dirty, _ = ap.ex.rents_data()
    dirty = {c: v[:200] for c, v in dirty.items()}
    # two Gaussian observations in one block
    m, o = ap._county_and_obs(dirty)
    o.julia("rent_base", ap.IndexedLookup("avg_rent"), ["county.state", "br"])
    o.choice("rent", ap.AddNoise("rent_base", 150.0))
    o.choice("rent_ad", ap.AddNoise("rent_base", 300.0))
    q = ap.Query(m, "Obs", {"CountyKey": "county.countykey", "County": ("county.name", "county_name"),
                            "Monthly Rent": ("rent_base", "rent"),
                            "Rent Ad": ("rent_base", "rent_ad")})
    dirty["Rent Ad"] = dirty["Monthly Rent"]
    with pytest.raises(NotImplementedError, match="one Gaussian observation per block"):
        LoweredModel(m, q, dirty)


def _world(oracle, S):
    lw, tr, obs = S["lw"], S["trace"], S["obs"]
    return helpers.mirror_world(oracle, lw, obs, tr, None, 1, helpers.option_logp_cpu(oracle, lw, tr))


@pytest.mark.parametrize("model", ["addnoise_model", "candidate_mean_model"])
def test_oracle_scores_addnoise_as_the_written_out_density(oracle, model):
    """score of candidate k for a row whose br is observed = (the same score without the number) - log 5 +
    logpdf(Normal(avg_rent[state_k, countykey_k, br], 150), x); without br: + logpdf(Normal(avg_rent[state_k, countykey_k], 150), x)"""
    fn = getattr(ap, model)
    S = ap.setup(fn, 600)
    lw, tr = S["lw"], S["trace"]
    w = _world(oracle, S)
    S0 = ap.setup(fn, 600)
    S0["lw"].xnum[:] = np.nan
    w0 = _world(oracle, S0)
    t = tr.tables["County"]
    spec = lw.gauss_spec
    mu = tr.mean_param.value
    has_br = "br" in lw.obs_index
    br = S["obs"][lw.obs_index["br"]] if has_br else np.zeros(600, dtype=np.int32)
    rows = [i for i in range(600) if br[i] >= 0 and lw.xnum[0, i] == lw.xnum[0, i]][:60]
    assert len(rows) == 60
    n_checked = 0
    for i in rows:
        _, a = w.eval_tree(0, 0, i, np.zeros(2, np.int32), int(tr.cur[0, i]), t.n + 1)
        _, b = w0.eval_tree(0, 0, i, np.zeros(2, np.int32), int(tr.cur[0, i]), t.n + 1)
        a, b = np.asarray(a).reshape(-1)[:t.n], np.asarray(b).reshape(-1)[:t.n]
        assert np.array_equal(np.isfinite(a), np.isfinite(b))
        for k in np.flatnonzero(np.isfinite(a)):
            st, ck = t.cols[lw.colidx["County"]["state"], k], t.cols[lw.colidx["County"]["countykey"], k]
            idx = spec["strides"][0] * st + spec["strides"][1] * ck + (spec["strides"][2] * br[i] if has_br else 0)
            want = (-np.log(5.0) if has_br else 0.0) + ap.addnoise_logpdf(lw.xnum[0, i], mu[idx], 150.0)
            assert abs((a[k] - b[k]) - want) <= 1e-9 * max(1.0, abs(want)), (i, k, a[k] - b[k], want)
            n_checked += 1
    assert n_checked >= 40


TWINS = {"own_br": ("addnoise_model", "identity_unit_model"),
         "candidate_only": ("candidate_mean_model", "identity_unit_candidate_model")}


@pytest.mark.parametrize("twins", sorted(TWINS))
@pytest.mark.parametrize("particles,mh,dd", [(2, True, True), (6, False, True), (2, True, False), (4, False, False)])
def test_oracle_addnoise_equals_the_identity_unit_twin(oracle, particles, mh, dd, twins):
    """observed and latent sweeps of the AddNoise program and of its TransformedGaussian twin: same bits"""
    A, B = (ap.setup(getattr(ap, f), 600) for f in TWINS[twins])
    assert np.array_equal(A["obs"], B["obs"]) and np.array_equal(A["lw"].xnum, B["lw"].xnum, equal_nan=True)
    assert np.array_equal(A["trace"].mean_param.value, B["trace"].mean_param.value)
    cfg = InferConfig(1, particles, int(dd), 1, int(mh), 50, 100)
    out = []
    for S in (A, B):
        lw, tr = S["lw"], S["trace"]
        w = _world(oracle, S)
        if lw.locals:
            loc0 = lw.locals[0]
            tr.locals[0][:, :len(loc0)] = [[(i % 5 if name == "br" else 0) for name in loc0] for i in range(tr.cur.shape[1])]
            w.set_cur_locals(0, tr.locals[0])
        choice, chosen, logml, _ = w.sweep_batched(cfg, 11, 0, tr.cur)
        loc = w.get_locals(0, tr.cur.shape[1]) if lw.locals else None
        pl = lw.latent_plans["County"]
        live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "County")
        excl = (np.full((len(pl["roots"]), len(live)), -1, dtype=np.int32) if dd
                else latent_current_choices(lw, tr, "County", live, cfg))
        lat = w.sweep_latent(cfg, 11, 0, pl["block_id"], pl["roots"], live, ev_off, ev_rows, ev_ctx, excl, len(pl["nodes"]))
        out.append((choice, chosen, logml, loc, lat))
    (ca, pa, la, loa, lta), (cb, pb, lb, lob, ltb) = out
    assert np.array_equal(ca, cb) and np.array_equal(pa, pb)
    assert np.array_equal(la, lb)
    if twins == "own_br":
        assert np.array_equal(loa[:, 0], lob[:, 0]) and (loa[:, 1] == -1).all() and (lob[:, 1] == 0).all()
    assert np.array_equal(lta[0], ltb[0]) and np.array_equal(lta[1], ltb[1])
    assert (la != 0).any()


def test_mean_parameter_statistics_of_addnoise():
    """gaussian_index: the host's sufficient statistics read x itself (no unit) and equal the twin's"""
    A, B = ap.setup(ap.addnoise_model, 600), ap.setup(ap.identity_unit_model, 600)
    for S in (A, B):
        S["trace"].locals[0][:, 0] = np.arange(600) % 5
        if S["lw"].locals[0] == ["br", "unit"]:
            S["trace"].locals[0][:, 1] = 0
    ra, ia, xa = A["trace"].gaussian_index()
    rb, ib, xb = B["trace"].gaussian_index()
    assert np.array_equal(ra, rb) and np.array_equal(ia, ib) and np.array_equal(xa, xb)
    assert np.array_equal(xa, A["lw"].xnum[0, ra]) and len(ra) > 500
    A["trace"].resample_parameters("Obs")
    B["trace"].resample_parameters("Obs")
    assert np.array_equal(A["trace"].mean_param.value, B["trace"].mean_param.value)
