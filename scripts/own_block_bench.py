"""pclean_sweep_own at scale: 10^6 rows of the synthetic hospital generator's City column as one own block
(`city ~ ChooseProportionally(clean cities, city_p); city_obs ~ AddTypos(city)`), 20 particles, after initialize_trace.

Reports, as one JSON line: milliseconds per pclean_sweep_own (HIP events around the call's launches, and the host clock around
the whole call, which ends in a stream synchronisation), the distinct observed tuples, the workgroups launched and the bytes
of its own byte model.  Baseline — the only way the code without own blocks computes these numbers: the same rows scored by
the generic leaf path, pclean_score_node with one draw on the new-row leaf of the twin program (the choice behind a slot;
host clock around the call).  Warm-up discarded, median of --runs runs (default 7).

--marginals: also times pclean_own_marginals on the same rows (top = 1 without and with the probability of the current value,
top = 8), every run right after a pclean_sweep_own of the same build so that the two see the same clocks: 2 warm-up rounds
discarded, then --runs rounds; medians and ranges go into the JSON line under "marginals" and the whole line into --out
(default profiles/own_marginals_bench.json; the committed file collects three such lines, alternated with the parent
commit's, under "this_commit").

usage: own_block_bench.py [--rows N] [--runs R] [--particles P] [--marginals [--out FILE]]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import initialize_trace
from pclean_amd.model import AddTypos, ChooseProportionally, LoweredModel, Model, ProportionsParameter, Query
from pclean_amd.synth import synth_hospital
from pclean_amd.trace import Trace


def _arg(name, default):
    a = sys.argv[1:]
    return int(a[a.index(name) + 1]) if name in a else default


def flat(words):
    m = Model()
    o = m.add_class("Obs")
    o.param("city_p", ProportionsParameter(1.0))
    with o.block():
        o.choice("city", ChooseProportionally(words, "city_p"))
        o.choice("city_obs", AddTypos("city"))
    return m, Query(m, "Obs", {"City": ("city", "city_obs")})


def twin(words):
    m = Model()
    a = m.add_class("A")
    a.param("city_p", ProportionsParameter(1.0))
    a.choice("x", ChooseProportionally(words, "city_p"))
    o = m.add_class("Obs")
    o.fk("r", "A")
    o.choice("city_obs", AddTypos("r.x"))
    return m, Query(m, "Obs", {"City": ("r.x", "city_obs")})


def byte_model(n_rows, K, n_groups, n_terms=1):
    """bytes pclean_sweep_own has to move: per workgroup the option list (logp 8, value 4, per term a pair byte and a length
    2) and its offsets; per row the row id 4, chosen + keep read 8 (written once: 8), logml read + write 16 (zeroed: 8), the
    current value read by the choice 4 and written by the draw 4"""
    per_group = K * (8 + 4 + n_terms * (1 + 2)) + 8 + 4 * n_terms
    per_row = 4 + 8 + 8 + 16 + 8 + 4 + 4
    return n_groups * per_group + n_rows * per_row


def _summary(xs):
    return dict(median=round(float(np.median(xs)), 3), min=round(float(min(xs)), 3), max=round(float(max(xs)), 3),
                all=[round(float(x), 3) for x in xs])


def time_marginals(hip, c, n, runs):
    """device ms (HIP events around the launch) and call ms (host clock, outputs copied back) of pclean_own_marginals, each
    round: one pclean_sweep_own, then the three marginal calls"""
    cases = {"top1": (1, False), "top1_with_current": (1, True), "top8": (8, False)}
    dev = {k: [] for k in ("sweep_own", *cases)}
    call = {k: [] for k in cases}
    for r in range(runs + 2):
        hip.sweep_own(c, 2, r, n)
        dev["sweep_own"].append(hip.get_timing().total_ms)
        for name, (top, cur) in cases.items():
            t0 = time.perf_counter()
            hip.own_marginals(0, 0, top, n, want_current=cur)
            call[name].append(1e3 * (time.perf_counter() - t0))
            dev[name].append(hip.get_timing().total_ms)
    st = hip.get_own_stats()
    out = dict(warmup_rounds=2, rounds=runs, workgroups=int(st.n_workgroups), variant="lds" if st.variants == 1 else "chunked",
               device_ms={k: _summary(v[2:]) for k, v in dev.items()}, call_ms={k: _summary(v[2:]) for k, v in call.items()})
    out["top1_over_sweep_own"] = round(out["device_ms"]["top1"]["median"] / out["device_ms"]["sweep_own"]["median"], 3)
    return out


def main():
    n, runs, P = _arg("--rows", 1_000_000), _arg("--runs", 7), _arg("--particles", 20)
    t0 = time.time()
    dirty, clean, _ = synth_hospital(n_rows=n, n_hosp=max(n // 100, 10))
    dirty, words = {"City": dirty["City"]}, list(dict.fromkeys(clean["City"]))
    t_gen = time.time() - t0
    m, q = flat(words)
    lw = LoweredModel(m, q, dirty)
    eng = Engine(lw, lw.encode_observations(dirty))
    tr = Trace(lw, n, 0)
    cfg = InferenceConfig(1, P)
    t0 = time.time()
    initialize_trace(eng, tr, cfg, 0)
    t_init = time.time() - t0
    hip, c = eng.hip, cfg.as_c()
    hip.set_active_rows(0, n)
    dev_ms, host_ms = [], []
    for r in range(runs + 2):
        t0 = time.perf_counter()
        hip.sweep_own(c, 1, r, n)  # (with its outputs: chosen particle and logml of every row come back, as the baseline's do)
        host_ms.append(1e3 * (time.perf_counter() - t0))
        dev_ms.append(float(hip.get_timing().total_ms))
    st = hip.get_own_stats()
    marg = time_marginals(hip, c, n, runs) if "--marginals" in sys.argv else None
    p = tr.params[("Obs", "city_p")].value.copy()
    tr.refresh_own_counts()  # (the timed calls went past Engine.sweep_own, which keeps the counts current)
    tr.check_consistency()
    eng.close()

    mt, qt = twin(words)
    lwt = LoweredModel(mt, qt, dirty)
    engt = Engine(lwt, lwt.encode_observations(dirty))
    trt = Trace(lwt, n, 0)
    trt.params[("A", "city_p")].value = p
    engt.upload_trace(trt)
    rows = np.arange(n, dtype=np.int32)
    base_ms = []
    for r in range(runs + 2):
        t0 = time.perf_counter()
        engt.hip.score_node(0, 1, rows, seed=1, sweep=r, n_draws=1)
        base_ms.append(1e3 * (time.perf_counter() - t0))
    engt.close()
    K = len(words)
    out = dict(rows=n, options=K, particles=P, runs=runs, distinct_tuples=int(st.n_runs), longest_run=int(st.longest_run),
               workgroups=int(st.n_workgroups), variant="lds" if st.variants == 1 else "chunked",
               sweep_own_device_ms=round(float(np.median(dev_ms[2:])), 3), sweep_own_device_ms_all=[round(x, 3) for x in dev_ms[2:]],
               sweep_own_call_ms=round(float(np.median(host_ms[2:])), 3), sweep_own_call_ms_all=[round(x, 3) for x in host_ms[2:]],
               generic_leaf_call_ms=round(float(np.median(base_ms[2:])), 3), generic_leaf_call_ms_all=[round(x, 3) for x in base_ms[2:]],
               model_bytes=int(byte_model(n, K, st.n_workgroups)), generate_s=round(t_gen, 1), initialize_s=round(t_init, 2))
    out["model_gb_per_s"] = round(out["model_bytes"] / (1e6 * out["sweep_own_device_ms"]), 1) if out["sweep_own_device_ms"] else None
    if marg is not None:
        out["marginals"] = marg
        a = sys.argv[1:]
        path = a[a.index("--out") + 1] if "--out" in a else os.path.join(
            os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "own_marginals_bench.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
