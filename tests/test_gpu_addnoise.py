"""GPU runs of the AddNoise program (tests/addnoise_program.py: rents with `rent ~ AddNoise(rent_base, 150.0)`): observed
and latent sweeps bit for bit against the C++ oracle, the same bits as the TransformedGaussian twin with one identity unit,
and inference end to end."""
import numpy as np
import pytest

import addnoise_program as ap
import helpers
from pclean_amd._lib import InferConfig
from pclean_amd.analysis import evaluate_accuracy, reconstructed_pool_ids
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import build_evidence, commit_latent, initialize_trace, latent_current_choices, run_inference
from pclean_amd.trace import Trace
from test_gpu_rents import oracle_sweep

pytestmark = pytest.mark.gpu


def _lowered(model_fn, n_rows):
    S = ap.setup(model_fn, n_rows)
    return S["dirty"], S["clean"], S["lw"], S["obs"]


@pytest.mark.parametrize("model", ["addnoise_model", "candidate_mean_model"])
@pytest.mark.parametrize("particles,mh,dd", [(2, True, True), (20, False, True), (2, True, False), (6, False, False)])
def test_addnoise_sweep_and_latent_parity(oracle, particles, mh, dd, model):
    """candidate_mean_model: the mean indexed by the referent's values alone, nothing own enumerated (n_locals = 0)"""
    dirty, clean, lw, obs = _lowered(getattr(ap, model), 3000)
    assert lw.xnum.shape == (1, 3000) and lw.gauss[(0, 0)]["transform"] == ("none", -1)
    eng = Engine(lw, obs, dist_mode=1)
    try:
        cfg0 = InferenceConfig(1, particles, use_mh_instead_of_pg=mh, rejuv_frequency=500)
        cfg = InferenceConfig(1, particles, use_mh_instead_of_pg=mh, rejuv_frequency=500, use_dd_proposals=dd)
        tr = Trace(lw, obs.shape[1], 2)
        initialize_trace(eng, tr, cfg0, 2, max_batch=512)
        tr.check_consistency()
        if lw.locals:
            assert (tr.locals[0][:, 0] >= 0).all() and (tr.locals[0][:, 1] == -1).all()
        else:
            assert tr.locals == {}
        n_nodes = [len(b["nodes"]) for b in lw.blocks]
        for sweep in range(2):
            pl = lw.latent_plans["County"]
            live, ev_off, ev_rows, ev_ctx = build_evidence(lw, tr, "County")
            excl = (np.full((len(pl["roots"]), len(live)), -1, dtype=np.int32) if dd
                    else latent_current_choices(lw, tr, "County", live, cfg))
            eng.upload_trace(tr)
            eng.hip.set_active_rows(0, -1)
            world = helpers.mirror_world(oracle, lw, obs, tr, eng)
            got = eng.hip.sweep_latent(cfg.as_c(), 5, sweep, pl["block_id"], pl["roots"], live, ev_off, ev_rows, ev_ctx,
                                       excl, len(pl["nodes"]))
            c = InferConfig(1, particles, int(dd), 1, int(mh), 50, 100)
            want = world.sweep_latent(c, 5, sweep, pl["block_id"], pl["roots"], live, ev_off, ev_rows, ev_ctx, excl,
                                      len(pl["nodes"]))
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
            commit_latent(lw, tr, "County", live, got[0], got[1])
            tr.check_consistency()
            eng.upload_trace(tr)
            world = helpers.mirror_world(oracle, lw, obs, tr, eng)
            if lw.locals:
                world.set_cur_locals(0, tr.locals[0])
            choice, chosen, logml, new_rows = eng.sweep(tr, cfg, 5, sweep)
            locals_gpu = tr.pending_locals[0].copy() if lw.locals else None
            o = oracle_sweep(oracle, world, cfg, 5, sweep, tr.cur, n_nodes)
            assert np.array_equal(choice, o[0]) and np.array_equal(chosen, o[1])
            assert np.array_equal(logml, o[2])
            assert set(new_rows) == set(o[3])
            for b in new_rows:
                assert np.array_equal(new_rows[b][0], o[3][b][0]) and np.array_equal(new_rows[b][1], o[3][b][1])
            if lw.locals:
                assert np.array_equal(locals_gpu, o[4]), "own choice (br) differs"
            tr.commit_locals()
            tr.commit(choice, new_rows)
            tr.resample_parameters()
            tr.check_consistency()
    finally:
        eng.close()


TWINS = {"own_br": ("addnoise_model", "identity_unit_model"),
         "candidate_only": ("candidate_mean_model", "identity_unit_candidate_model")}


@pytest.mark.parametrize("twins", sorted(TWINS))
@pytest.mark.parametrize("particles,mh,dd", [(2, True, True), (6, False, False)])
def test_addnoise_equals_the_identity_unit_twin_on_the_gpu(particles, mh, dd, twins):
    out = []
    for fn in (getattr(ap, f) for f in TWINS[twins]):
        dirty, clean, lw, obs = _lowered(fn, 3000)
        eng = Engine(lw, obs, dist_mode=1)
        try:
            cfg0 = InferenceConfig(1, particles, use_mh_instead_of_pg=mh, rejuv_frequency=500)
            cfg = InferenceConfig(1, particles, use_mh_instead_of_pg=mh, rejuv_frequency=500, use_dd_proposals=dd)
            tr = Trace(lw, obs.shape[1], 4)
            initialize_trace(eng, tr, cfg0, 4, max_batch=512)
            eng.upload_trace(tr)
            choice, chosen, logml, _ = eng.sweep(tr, cfg, 9, 0)
            out.append((tr.cur.copy(), tr.mean_param.value.copy(), choice, chosen, logml)
                       + ((tr.locals[0][:, 0].copy(), tr.pending_locals[0][:, 0].copy()) if twins == "own_br" else ()))
        finally:
            eng.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def _end_to_end(seed, model=ap.addnoise_model):
    dirty, clean, lw, obs = _lowered(model, 4000)
    eng = Engine(lw, obs, dist_mode=1)
    try:
        cfg = InferenceConfig(2, 2, use_mh_instead_of_pg=True, rejuv_frequency=500)
        tr = Trace(lw, obs.shape[1], seed)
        initialize_trace(eng, tr, cfg, seed, max_batch=1024)
        run_inference(eng, tr, cfg, seed)
        tr.check_consistency()
        return dirty, clean, lw, tr
    finally:
        eng.close()


def test_addnoise_end_to_end():
    dirty, clean, lw, tr = _end_to_end(7)
    _, _, _, tr2 = _end_to_end(7)
    # reproducible bit for bit
    assert np.array_equal(tr.cur, tr2.cur) and np.array_equal(tr.locals[0], tr2.locals[0])
    assert np.array_equal(tr.mean_param.value, tr2.mean_param.value)
    # the query's numeric column is reported: round(x) (no unit to repair), the others as for rents
    ours = reconstructed_pool_ids(lw, tr)
    assert isinstance(ours["Monthly Rent"], tuple)
    x = lw.xnum[0]
    ok = ~np.isnan(x)
    assert np.array_equal(ours["Monthly Rent"][1][ok], np.round(x[ok]))
    acc = evaluate_accuracy(lw, tr, dirty, clean)
    assert acc["imputed"] > 300 and acc["correctly_imputed"] > 0.25 * acc["imputed"] and acc["f1"] > 0.25
    # the mean parameter's Gibbs draw (add_noise.jl:74-82) given the final assignment: every cell with 20 or more rows lies
    # within 6 posterior standard deviations of its rows' mean (prior 1500 +- 1000, sigma 150)
    tr.resample_parameters("Obs")
    rows, idx, xs = tr.gaussian_index()
    n = np.bincount(idx, minlength=len(tr.mean_param.value))
    sm = np.bincount(idx, weights=xs, minlength=len(tr.mean_param.value))
    cells = np.flatnonzero(n >= 20)
    assert len(cells) >= 5
    var = 1.0 / (1.0 / 1000.0 ** 2 + n[cells] / 150.0 ** 2)
    post = var * (1500.0 / 1000.0 ** 2 + sm[cells] / 150.0 ** 2)
    assert (np.abs(tr.mean_param.value[cells] - post) <= 6 * np.sqrt(var)).all()


def test_addnoise_with_a_candidate_side_mean_end_to_end():
    dirty, clean, lw, tr = _end_to_end(5, ap.candidate_mean_model)
    _, _, _, tr2 = _end_to_end(5, ap.candidate_mean_model)
    assert np.array_equal(tr.cur, tr2.cur) and np.array_equal(tr.mean_param.value, tr2.mean_param.value)
    assert tr.locals == {}
    ours = reconstructed_pool_ids(lw, tr)
    ok = ~np.isnan(lw.xnum[0])
    assert np.array_equal(ours["Monthly Rent"][1][ok], np.round(lw.xnum[0][ok]))
    acc = evaluate_accuracy(lw, tr, dirty, clean)
    assert acc["f1"] > 0.25
    tr.resample_parameters("Obs")
    rows, idx, xs = tr.gaussian_index()
    assert len(rows) == ok.sum()  # every assigned row with a number feeds its (state, countykey) cell
    n = np.bincount(idx, minlength=len(tr.mean_param.value))
    sm = np.bincount(idx, weights=xs, minlength=len(tr.mean_param.value))
    cells = np.flatnonzero(n >= 20)
    assert len(cells) >= 5
    var = 1.0 / (1.0 / 1000.0 ** 2 + n[cells] / 150.0 ** 2)
    post = var * (1500.0 / 1000.0 ** 2 + sm[cells] / 150.0 ** 2)
    assert (np.abs(tr.mean_param.value[cells] - post) <= 6 * np.sqrt(var)).all()
