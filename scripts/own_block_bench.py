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

--product: City x State of the same generator as ONE product leaf (`state ~ ChooseProportionally(states, theta, index="city")`,
both observed through AddTypos) — own_product_kernel.  The trace starts from the clean values (the sweep's cost does not
depend on them) and one parameter move; device ms of pclean_sweep_own by HIP events, 2 warm-ups and --runs runs, with the
grid size, the distinct tuples, the longest run and the byte model.  If the grid exceeded OWN_MAX_OPTIONS the least
frequent cities (and their rows) would be dropped until it fits; the generator's 3 657 x 50 needs none dropped.
--product --alternate N: N rounds of fresh processes of this build, the default path, PCLEAN_NO_OWN_PRODUCT=1 (the generic
own_leaf_kernel: the only way the code computed these numbers before) and PCLEAN_NO_OWN_SKIP=1 (the product kernel
without its exact skip: what the skip buys) in turns, on one generated data set; the lines and
the verdict (the product kernel's median below the baseline's fastest run) go into --out (default
profiles/own_product_bench.json).

--gauss: a Gaussian leaf (own_gauss_kernel): synthetic rows `room ~ ChooseProportionally; room_obs ~ AddTypos(room);
unit ~ ChooseUniformly; rent ~ TransformedGaussian(avg[room], 150, unit)` in two shapes, 5 rooms x 2 units and 1000 x 4.  Per
shape and process: device ms of pclean_sweep_own (HIP events, 2 warm-ups and --runs runs) and of pclean_own_gauss_stats, a
byte and fp64-operation model, and the yardstick — the parent cannot run this program at all, so it is the SAME build's
string-only sweep of the same rows and string factor with the Gaussian terms left off (`room`, `room_obs` alone: the
nearest thing the parent computes); the ratio is stated, not asserted.  --processes N (default 3) fresh processes; the
lines go into --out (default profiles/own_gauss_bench.json).

--star: City with State and CountyName as its dependents (a star: own_star_kernel), one process; --star --alternate N: N
rounds of fresh processes — the star, the star with PCLEAN_NO_OWN_SKIP=1, and the two one-dependent programs City x State and
City x CountyName through own_product_kernel, whose device times summed are the nearest computation without the star — into
profiles/own_star_bench.json.

usage: own_block_bench.py [--rows N] [--runs R] [--particles P] [--marginals [--out FILE]] [--product [--alternate N] [--out FILE]]
                          [--star [--alternate N] [--out FILE]]
                          [--gauss [--processes N] [--out FILE]]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import initialize_trace
from pclean_amd.model import (OWN_MAX_OPTIONS, AddTypos, ChooseProportionally, IndexedProportionsParameter, LoweredModel, Model,
                              ProportionsParameter, Query)
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


def product_byte_model(n_rows, na, nb, n_groups):
    """bytes own_product_kernel has to move: per workgroup the two factors' values once (value 4, pair byte 1, length 2 each)
    and the grid's priors twice at most (8 per option and pass; the weight pass skips the chunks far below the maximum);
    per row what byte_model counts"""
    per_group = (na + nb) * (4 + 1 + 2) + 2 * na * nb * 8 + 8 + 8
    per_row = 4 + 8 + 8 + 16 + 8 + 4 + 4
    return n_groups * per_group + n_rows * per_row


def product_data(n):
    dirty, clean, _ = synth_hospital(n_rows=n, n_hosp=max(n // 100, 10))
    cities, states = list(dict.fromkeys(clean["City"])), list(dict.fromkeys(clean["State"]))
    dropped = 0
    if len(cities) * len(states) > OWN_MAX_OPTIONS:  # the stated rule: the most frequent cities that fit, their rows alone
        keep = OWN_MAX_OPTIONS // len(states)
        freq = {}
        for c in clean["City"]:
            freq[c] = freq.get(c, 0) + 1
        kept = set(sorted(cities, key=lambda c: -freq[c])[:keep])
        rows = [i for i, c in enumerate(clean["City"]) if c in kept]
        dropped = len(cities) - keep
        dirty = {k: [dirty[k][i] for i in rows] for k in ("City", "State")}
        clean = {k: [clean[k][i] for i in rows] for k in ("City", "State")}
        cities = [c for c in cities if c in kept]
    return dict(dirty={k: dirty[k] for k in ("City", "State")}, clean={k: clean[k] for k in ("City", "State")}, cities=cities,
                states=states, dropped_cities=dropped)


def product_run(D, runs, P):
    """one process: the JSON line of --product"""
    cities, states, dirty = D["cities"], D["states"], D["dirty"]
    n = len(dirty["City"])
    m = Model()
    o = m.add_class("Obs")
    o.param("city_p", ProportionsParameter(1.0))
    o.param("theta", IndexedProportionsParameter(1.0))
    with o.block():
        o.choice("city", ChooseProportionally(cities, "city_p"))
        o.choice("state", ChooseProportionally(states, "theta", index="city"))
        o.choice("city_obs", AddTypos("city"))
        o.choice("state_obs", AddTypos("state"))
    lw = LoweredModel(m, Query(m, "Obs", {"City": ("city", "city_obs"), "State": ("state", "state_obs")}), dirty)
    eng = Engine(lw, lw.encode_observations(dirty))
    try:
        tr = Trace.from_clean_values(lw, {0: {"city": D["clean"]["City"], "state": D["clean"]["State"]}}, n)
        tr.resample_parameters()
        eng.upload_trace(tr)
        eng._push_own(tr)
        hip, c = eng.hip, InferenceConfig(1, P).as_c()
        hip.set_active_rows(0, n)
        dev_ms = []
        for r in range(runs + 2):
            hip.sweep_own(c, 1, r, n)
            dev_ms.append(float(hip.get_timing().total_ms))
        st = hip.get_own_stats()
        vals = hip.get_own(0, 1, n)[0]
        assert vals.min() >= 0 and vals.max() < len(cities) * len(states)
    finally:
        eng.close()
    na, nb = len(cities), len(states)
    out = dict(rows=n, grid=[na, nb], options=na * nb, dropped_cities=D["dropped_cities"], particles=P, warmups=2, runs=runs,
               path="generic (PCLEAN_NO_OWN_PRODUCT)" if os.environ.get("PCLEAN_NO_OWN_PRODUCT") else (
                   "product kernel without the skip (PCLEAN_NO_OWN_SKIP)" if os.environ.get("PCLEAN_NO_OWN_SKIP") else "default"),
               variants=int(st.variants), distinct_tuples=int(st.n_runs), longest_run=int(st.longest_run),
               workgroups=int(st.n_workgroups), sweep_own_device_ms=_summary(dev_ms[2:]),
               model_bytes=int(product_byte_model(n, na, nb, st.n_workgroups)),
               checksum=int(np.bitwise_xor.reduce(vals.astype(np.int64) * (np.arange(n) + 1))))
    out["model_gb_per_s"] = round(out["model_bytes"] / (1e6 * out["sweep_own_device_ms"]["median"]), 1)
    return out


def product_main():
    import pickle
    import subprocess
    import tempfile
    a = sys.argv[1:]
    n, runs, P = _arg("--rows", 1_000_000), _arg("--runs", 7), _arg("--particles", 20)
    if "--data" in a:  # a child of --alternate
        with open(a[a.index("--data") + 1], "rb") as f:
            D = pickle.load(f)
        print(json.dumps(product_run(D, runs, P)))
        return
    D = product_data(n)
    pairs = _arg("--alternate", 0)
    if not pairs:
        print(json.dumps(product_run(D, runs, P)))
        return
    lines = {"default": [], "generic": [], "no_skip": []}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "data.pkl")
        with open(path, "wb") as f:
            pickle.dump(D, f)
        for k in range(pairs):
            for name in lines:
                env = dict(os.environ)
                env.pop("PCLEAN_NO_OWN_PRODUCT", None)
                env.pop("PCLEAN_NO_OWN_SKIP", None)
                if name == "generic":
                    env["PCLEAN_NO_OWN_PRODUCT"] = "1"
                if name == "no_skip":  # the product kernel without its exact skip of the groups far below the maximum
                    env["PCLEAN_NO_OWN_SKIP"] = "1"
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--product", "--data", path, "--runs", str(runs),
                                    "--particles", str(P)], env=env, stdout=subprocess.PIPE, text=True, timeout=900, check=True)
                lines[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(f"[{name} {k}] {lines[name][-1]['sweep_own_device_ms']}", flush=True)
    med = float(np.median([x["sweep_own_device_ms"]["median"] for x in lines["default"]]))
    fastest = min(x["sweep_own_device_ms"]["min"] for x in lines["generic"])
    no_skip = float(np.median([x["sweep_own_device_ms"]["median"] for x in lines["no_skip"]]))
    out = dict(product_median_ms=round(med, 3), baseline_fastest_run_ms=round(fastest, 3), product_below_baseline=bool(med < fastest),
               product_without_skip_median_ms=round(no_skip, 3),
               same_values=len({x["checksum"] for v in lines.values() for x in v}) == 1, **lines)
    dst = a[a.index("--out") + 1] if "--out" in a else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "own_product_bench.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("product_median_ms", "baseline_fastest_run_ms", "product_below_baseline",
                                          "product_without_skip_median_ms", "same_values")}))


# ---- --star: City with State and CountyName as its dependents --------------------------------------------------------------
def star_data(n):
    """City, State and CountyName of the synthetic generator (both determined by the city).  The stated rule: the most
    frequent cities such that K_a <= 4096 and K_a x max(K_state, K_county) <= OWN_MAX_OPTIONS, their rows alone."""
    dirty, clean, _ = synth_hospital(n_rows=n, n_hosp=max(n // 100, 10))
    cols = ("City", "State", "CountyName")
    freq = {}
    for c in clean["City"]:
        freq[c] = freq.get(c, 0) + 1
    order = sorted(freq, key=lambda c: -freq[c])
    county_of = dict(zip(clean["City"], clean["CountyName"]))
    n_states = len(set(clean["State"]))
    keep = min(len(order), 4096)
    while keep * max(n_states, len({county_of[c] for c in order[:keep]})) > OWN_MAX_OPTIONS:
        keep -= 1
    kept = set(order[:keep])
    rows = [i for i, c in enumerate(clean["City"]) if c in kept]
    dirty = {k: [dirty[k][i] for i in rows] for k in cols}
    clean = {k: [clean[k][i] for i in rows] for k in cols}
    return dict(dirty=dirty, clean=clean, vocab={k: list(dict.fromkeys(clean[k])) for k in cols}, dropped_cities=len(order) - keep)


def star_run(D, runs, P, what):
    """one process: the JSON line of --star.  what: "star" (both dependents, own_star=True) or the name of ONE dependent (the
    one-dependent program through own_product_kernel: the nearest computation without the star)"""
    from pclean_amd import experiments as ex
    deps = ("State", "CountyName") if what == "star" else (what,)
    cols = ("City",) + deps
    dirty = {k: D["dirty"][k] for k in cols}
    vocab = {k: D["vocab"][k] for k in cols}
    n = len(dirty["City"])
    m = ex.flat_model(vocab, star=("City", deps)) if what == "star" else ex.flat_model(vocab, dependent=("City", what))
    lw = LoweredModel(m, ex.flat_query(m, cols), dirty, own_star=what == "star")
    eng = Engine(lw, lw.encode_observations(dirty))
    try:
        tr = Trace.from_clean_values(lw, {0: {k: D["clean"][k] for k in cols}}, n)
        tr.resample_parameters()
        eng.upload_trace(tr)
        eng._push_own(tr)
        hip, c = eng.hip, InferenceConfig(1, P).as_c()
        hip.set_active_rows(0, n)
        dev_ms = []
        for r in range(runs + 2):
            hip.sweep_own(c, 1, r, n)
            dev_ms.append(float(hip.get_timing().total_ms))
        st = hip.get_own_stats()
        vals = hip.get_own(0, len(cols) if what == "star" else 1, n)
        assert vals.min() >= 0
    finally:
        eng.close()
    mix = np.zeros(n, dtype=np.int64)
    for v in vals:
        mix = mix * 1000003 + v
    return dict(rows=n, what=what, sizes=[len(vocab[k]) for k in cols], dropped_cities=D["dropped_cities"], particles=P, warmups=2,
                runs=runs, no_skip=bool(os.environ.get("PCLEAN_NO_OWN_SKIP")), variants=int(st.variants), distinct_tuples=int(st.n_runs),
                longest_run=int(st.longest_run), workgroups=int(st.n_workgroups), star_weighed=int(st.star_weighed),
                star_skipped=int(st.star_skipped), sweep_own_device_ms=_summary(dev_ms[2:]),
                checksum=int(np.bitwise_xor.reduce(mix * (np.arange(n) + 1))))


def star_main():
    import pickle
    import subprocess
    import tempfile
    a = sys.argv[1:]
    n, runs, P = _arg("--rows", 1_000_000), _arg("--runs", 7), _arg("--particles", 20)
    if "--data" in a:  # a child of --alternate
        with open(a[a.index("--data") + 1], "rb") as f:
            D = pickle.load(f)
        print(json.dumps(star_run(D, runs, P, a[a.index("--what") + 1])))
        return
    D = star_data(n)
    rounds = _arg("--alternate", 0)
    if not rounds:
        print(json.dumps(star_run(D, runs, P, "star")))
        return
    lines = {"star": [], "star_no_skip": [], "State": [], "CountyName": []}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "data.pkl")
        with open(path, "wb") as f:
            pickle.dump(D, f)
        for k in range(rounds):
            for name in lines:
                env = dict(os.environ)
                env.pop("PCLEAN_NO_OWN_PRODUCT", None)
                env.pop("PCLEAN_NO_OWN_SKIP", None)
                if name == "star_no_skip":
                    env["PCLEAN_NO_OWN_SKIP"] = "1"
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--star", "--data", path, "--what",
                                    "star" if name.startswith("star") else name, "--runs", str(runs), "--particles", str(P)], env=env,
                                   stdout=subprocess.PIPE, text=True, timeout=900, check=True)
                lines[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
                print(f"[{name} {k}] {lines[name][-1]['sweep_own_device_ms']}", flush=True)
    med = {name: float(np.median([x["sweep_own_device_ms"]["median"] for x in v])) for name, v in lines.items()}
    pairs = med["State"] + med["CountyName"]
    out = dict(star_median_ms=round(med["star"], 3), star_without_skip_median_ms=round(med["star_no_skip"], 3),
               two_pairs_summed_median_ms=round(pairs, 3), star_within_1_1_of_the_pairs=bool(med["star"] <= 1.1 * pairs),
               same_values_with_and_without_skip=len({x["checksum"] for k in ("star", "star_no_skip") for x in lines[k]}) == 1, **lines)
    dst = a[a.index("--out") + 1] if "--out" in a else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "own_star_bench.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k not in lines}))


GAUSS_SHAPES = ((5, 2), (1000, 4))


def gauss_data(n, na, nb, seed=0):
    """n synthetic rows: a room (Zipf-like frequencies), its name with a typo in a fifth of the rows and missing in 2 %, a rent
    around the room's mean stated in a unit other than the first in a tenth of the rows and missing in 5 %"""
    rng = np.random.default_rng(seed)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    rooms = list(dict.fromkeys("".join(rng.choice(letters, 8)) for _ in range(2 * na)))[:na]
    p = 1.0 / np.arange(1, na + 1)
    a = rng.choice(na, size=n, p=p / p.sum())
    b = np.where(rng.random(n) < 0.1, rng.integers(1, max(nb, 2), n), 0) if nb > 1 else np.zeros(n, np.int64)
    scale = np.array([1.0, 1000.0, 12.0, 7.0])[:nb]
    rent = rng.normal(1500.0 + 1500.0 * (a % 50), 150.0) / scale[b]
    typo, miss = rng.random(n) < 0.2, rng.random(n) < 0.02
    pos, ch = rng.integers(0, 2, n), rng.choice(letters[:4], n)  # (few distinct typos: a pair table takes 65 535 observed strings)
    obs = [None if miss[i] else (rooms[a[i]][:pos[i]] + ch[i] + rooms[a[i]][pos[i] + 1:] if typo[i] else rooms[a[i]]) for i in range(n)]
    xmiss = rng.random(n) < 0.05
    return rooms, {"Room": obs, "Rent": [None if xmiss[i] else float(rent[i]) for i in range(n)]}


def gauss_models(rooms, nb):
    from pclean_amd.model import ChooseUniformly, IndexedLookup, IndexedMeanParameter, Transformation, TransformedGaussian
    sc = [1.0, 1000.0, 12.0, 7.0][:nb]
    units = [Transformation(lambda x, c=c: x / c, lambda x, c=c: x * c, lambda x, c=c: 1.0 / c) for c in sc]
    out = []
    for with_gauss in (True, False):
        m = Model()
        o = m.add_class("Obs")
        o.param("room_p", ProportionsParameter(1.0))
        o.param("avg", IndexedMeanParameter(1500.0, 100000.0))
        with o.block():
            o.choice("room", ChooseProportionally(rooms, "room_p"))
            o.choice("room_obs", AddTypos("room"))
            if with_gauss:
                o.choice("unit", ChooseUniformly(units))
                o.julia("base", IndexedLookup("avg"), ["room"])
                o.choice("rent", TransformedGaussian("base", 150.0, "unit"))
                o.julia("corrected", lambda unit, rent: round(unit.backward(rent)), ["unit", "rent"])
        bind = {"Room": ("room", "room_obs")}
        if with_gauss:
            bind["Rent"] = ("corrected", "rent")
        out.append((m, Query(m, "Obs", bind)))
    return out


def gauss_models_bytes(n, na, nb, n_groups, n_present):
    """bytes and fp64 operations of one sweep of the Gaussian leaf.  Bytes: per workgroup the grid's priors and value columns
    (8 + 8 per option) and the string term's pair bytes and lengths per room (3); per row what byte_model counts plus the
    number (8).  Operations per row and option: the prior and the string term (1 add), the Gaussian term where the number is
    present (mul, sub, div, 2 mul, 3 sub: 8), one subtraction and one exp (about 30) for the weight, the maximum; a draw
    evaluates one step of at most 64 options again."""
    K = na * nb
    bytes_ = n_groups * (K * 16 + na * 3 + 16) + n * (4 + 8 + 8 + 16 + 8 + 4 + 4 + 8)
    ops = n * K * (1 + 1 + 31) + n_present * K * 8 + n * min(K, 64) * 31
    return int(bytes_), int(ops)


def gauss_run(n, runs, P):
    """one process: both shapes, the Gaussian leaf and the string-only yardstick"""
    out = []
    for na, nb in GAUSS_SHAPES:
        rooms, dirty = gauss_data(n, na, nb)
        line = dict(rows=n, grid=[na, nb], options=na * nb, particles=P, warmups=2, runs=runs)
        for name, (m, q) in zip(("gauss", "string_only"), gauss_models(rooms, nb)):
            d = {c: dirty[c] for c in q.obsmap}
            lw = LoweredModel(m, q, d)
            eng = Engine(lw, lw.encode_observations(d))
            try:
                tr = Trace(lw, n, 0)
                cfg = InferenceConfig(1, P)
                initialize_trace(eng, tr, cfg, 0)
                hip, c = eng.hip, cfg.as_c()
                eng.upload_trace(tr)
                hip.set_active_rows(0, n)
                dev = []
                for r in range(runs + 2):
                    hip.sweep_own(c, 1, r, n, want_outputs=False)
                    dev.append(float(hip.get_timing().total_ms))
                st = hip.get_own_stats()
                line[name] = dict(variants=int(st.variants), distinct_tuples=int(st.n_runs), longest_run=int(st.longest_run),
                                  workgroups=int(st.n_workgroups), sweep_own_device_ms=_summary(dev[2:]))
                if name == "gauss":
                    sd = []
                    for r in range(runs + 2):
                        hip.own_gauss_stats(0, 0, 0, na)
                        sd.append(float(hip.get_timing().total_ms))
                    n_present = sum(v is not None for v in dirty["Rent"])
                    mb, ops = gauss_models_bytes(n, na, nb, st.n_workgroups, n_present)
                    med = line[name]["sweep_own_device_ms"]["median"]
                    line[name].update(own_gauss_stats_device_ms=_summary(sd[2:]), model_bytes=mb, model_fp64_ops=ops,
                                      model_gb_per_s=round(mb / (1e6 * med), 1), model_gflop_per_s=round(ops / (1e6 * med), 1))
            finally:
                eng.close()
        line["gauss_over_string_only"] = round(line["gauss"]["sweep_own_device_ms"]["median"] /
                                               line["string_only"]["sweep_own_device_ms"]["median"], 3)
        out.append(line)
    return out


def gauss_main():
    import subprocess
    a = sys.argv[1:]
    n, runs, P = _arg("--rows", 1_000_000), _arg("--runs", 7), _arg("--particles", 20)
    if "--child" in a:
        print(json.dumps(gauss_run(n, runs, P)))
        return
    procs = []
    for k in range(_arg("--processes", 3)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--gauss", "--child", "--rows", str(n), "--runs", str(runs),
                            "--particles", str(P)], stdout=subprocess.PIPE, text=True, timeout=1100, check=True)
        procs.append(json.loads(r.stdout.strip().splitlines()[-1]))
        for line in procs[-1]:
            print(f"[process {k}] {line['grid']}: gauss {line['gauss']['sweep_own_device_ms']['median']} ms, string only "
                  f"{line['string_only']['sweep_own_device_ms']['median']} ms, stats "
                  f"{line['gauss']['own_gauss_stats_device_ms']['median']} ms", flush=True)
    out = dict(profiled=False, note="device ms by HIP events; the yardstick is the same build's string-only sweep of the same "
               "rows and string factor (the parent cannot run the Gaussian program); the ratio is stated, not asserted",
               processes=procs)
    dst = a[a.index("--out") + 1] if "--out" in a else os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "own_gauss_bench.json")
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


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
    if "--gauss" in sys.argv[1:]:
        gauss_main()
    else:
        star_main() if "--star" in sys.argv[1:] else product_main() if "--product" in sys.argv[1:] else main()
