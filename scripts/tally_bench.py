"""What the cleaned table and its accuracy cost at the bench shape (bench.py's workload: synthetic hospital, 10^6 rows x 15
queried columns): the host path — analysis.accuracy_counts including the pull of the device-resident state it triggers —
against tally.CellTally on the device, and add + consensus at keep 16.  Median of five calls after one warm-up; an
observed-class sweep runs before every call, so that the device is ahead of the host arrays as it is during a run.
Kernel figures are host-clock times of calls that end in a stream synchronisation (launch and synchronisation included);
bytes are what the algorithm has to move, computed from the shapes.  Writes profiles/tally_bench.json.

    python scripts/tally_bench.py [--rows N] [--keep K] [--out FILE]

`--program rents` times the shipped rents program instead (all of its rows unless --rows says otherwise): accuracy_counts
and add + consensus once through the mixed path (CellTally(eng, tr): three columns on the device, room types and the rent
on the host, reading the trace) and once with own=True (all five on the device).  The own=True calls run with Engine.pull
made to raise, and both paths' counters must equal the host's.  Writes profiles/tally_bench_rents.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HBM_PEAK = 8.0e12  # bytes/s, MI355X specification


def main_rents(args):
    from pclean_amd import analysis
    from pclean_amd import experiments as ex
    from pclean_amd import inference as inf
    from pclean_amd.engine import Engine, InferenceConfig
    from pclean_amd.model import LoweredModel
    from pclean_amd.tally import CellTally
    from pclean_amd.trace import Trace

    dirty, clean = ex.rents_data()
    (dirty, clean), _ = ex.shuffle_rows([dirty, clean], 0)
    if args.rows:
        dirty = {c: v[:args.rows] for c, v in dirty.items()}
        clean = {c: v[:args.rows] for c, v in clean.items()}
    m = ex.rents_model(dirty)
    lw = LoweredModel(m, ex.rents_query(m), dirty)
    obs = lw.encode_observations(dirty)
    n = obs.shape[1]
    eng = Engine(lw, obs)
    cfg = InferenceConfig(1, 2, use_mh_instead_of_pg=True, rejuv_frequency=500)
    tr = Trace(lw, n, 0)
    inf.initialize_trace(eng, tr, cfg, 0, max_batch=2048)
    inf.run_inference(eng, tr, cfg, 0)
    sweep = [0]

    def advance():
        sweep[0] += 1
        inf.observed_sweep(eng, tr, cfg, 0, sweep[0])

    pulls = [0]
    real_pull = Engine.pull

    def counting_pull(self, trace):
        pulls[0] += 1
        return real_pull(self, trace)

    def refusing_pull(self, trace):
        raise AssertionError("Engine.pull called on the own=True path")

    def timed(fn, own):
        """a tally call alone sees the counted / refused Engine.pull: the sweeps between the calls pull as they always do
        (rents' parameter moves read the trace)"""
        Engine.pull = refusing_pull if own else counting_pull
        try:
            t0 = time.perf_counter()
            out = fn()
            return out, 1e3 * (time.perf_counter() - t0)
        finally:
            Engine.pull = real_pull

    res = {"program": "rents", "rows": n, "queried_columns": len(lw.query.cleanmap), "keep": args.keep, "calls": args.calls,
           "note": "milliseconds, median of `calls` calls after one warm-up; an observed-class sweep before every call"}
    for own in (False, True):
        tally = CellTally(eng, tr, keep=args.keep, own=own)
        pulls[0] = 0
        cnt_ms, both = [], []
        for i in range(args.calls + 1):
            advance()
            dev_counts, d = timed(lambda: tally.accuracy_counts(tr, dirty, clean), own)
            if i:
                cnt_ms.append(d)
        for _ in range(args.keep):
            advance()
            timed(lambda: tally.add(tr), own)
        for i in range(args.calls + 1):
            advance()
            _, a = timed(lambda: tally.add(tr), own)
            _, f = timed(tally.consensus, own)
            if i:
                both.append(a + f)
        advance()
        dev_counts, _ = timed(lambda: tally.accuracy_counts(tr, dirty, clean), own)
        cacc, _ = timed(lambda: tally.consensus_accuracy(dirty, clean), own)
        n_pulls = pulls[0]
        same = bool(np.array_equal(dev_counts, analysis.accuracy_counts(lw, tr, dirty, clean)))
        if not same:
            raise SystemExit(f"[tally_bench] own={own}: the tally's counters differ from analysis.accuracy_counts")
        res["own" if own else "mixed"] = {"columns_on_device": len(tally.columns), "equals_host_counts": same,
                                          "pulls": n_pulls, "accuracy_counts_ms": statistics.median(cnt_ms),
                                          "add_plus_consensus_ms": statistics.median(both), "n_kept": tally.n_kept,
                                          "f1_consensus": cacc["f1"]}
        print(f"[tally_bench] rents own={own}: {res['own' if own else 'mixed']}", file=sys.stderr, flush=True)
        tally.close()
    res["f1_last_sample"] = analysis.evaluate_accuracy(lw, tr, dirty, clean)["f1"]
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--program", choices=["hospital", "rents"], default="hospital")
    ap.add_argument("--rows", type=int, default=None)
    ap.add_argument("--hospitals", type=int, default=10_000)
    ap.add_argument("--particles", type=int, default=20)
    ap.add_argument("--seed", type=int, default=20250926)
    ap.add_argument("--keep", type=int, default=16)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "tally_bench.json" if args.program == "hospital" else "tally_bench_rents.json")
    if args.program == "rents":
        res = main_rents(args)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(res))
        return
    if args.rows is None:
        args.rows = 1_000_000

    import bench
    from pclean_amd import _lib, analysis
    from pclean_amd import inference as inf
    from pclean_amd.engine import Engine, InferenceConfig
    from pclean_amd.tally import CellTally
    from pclean_amd.trace import Trace

    dirty, clean, lw, obs = bench.build_workload(args.rows, args.hospitals, args.seed)
    # (restricted-distance pair tables: half a second of table build instead of half a minute; nothing measured here reads them)
    eng = Engine(lw, obs, dist_mode=_lib.DIST_OSA)
    cfg = InferenceConfig(1, args.particles)
    tr = Trace(lw, args.rows, args.seed)
    inf.initialize_trace(eng, tr, cfg, args.seed, max_batch=32768)
    eng.prepare(tr)
    inf.run_inference(eng, tr, cfg, args.seed)
    sweep = [0]

    def advance():
        sweep[0] += 1
        inf.observed_sweep(eng, tr, cfg, args.seed, sweep[0])
        return tr._dev is eng

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return out, 1e3 * (time.perf_counter() - t0)

    n, c = args.rows, len(lw.query.cleanmap)
    res = {"rows": n, "queried_columns": c, "keep": args.keep, "calls": args.calls, "hbm_peak_bytes_per_s": HBM_PEAK,
           "note": "milliseconds, median of `calls` calls after one warm-up; an observed-class sweep before every call"}

    # ---- host path: pull + analysis.accuracy_counts -----------------------------------------------------------------
    pulls, counts_ms, ahead = [], [], []
    for i in range(args.calls + 1):
        ahead.append(advance())
        _, p = timed(tr._sync)
        host_counts, h = timed(lambda: analysis.accuracy_counts(lw, tr, dirty, clean))
        analysis.f1_from_counts(host_counts)
        if i:
            pulls.append(p)
            counts_ms.append(h)
        print(f"[tally_bench] host call {i}: pull {p:.1f} ms, counts {h:.1f} ms", file=sys.stderr, flush=True)
    res["host"] = {"device_was_ahead": all(ahead), "pull_ms": statistics.median(pulls),
                   "accuracy_counts_ms": statistics.median(counts_ms),
                   "total_ms": statistics.median([a + b for a, b in zip(pulls, counts_ms)])}

    # ---- device path ------------------------------------------------------------------------------------------------
    tally = CellTally(eng, tr, keep=args.keep)
    dev_ms, recon_ms, cnt_ms = [], [], []
    for i in range(args.calls + 1):
        advance()
        dev_counts, d = timed(lambda: tally.accuracy_counts(tr, dirty, clean))
        _, r = timed(lambda: eng.hip.recon_run(len(tally.columns), n, fetch=False))
        _, k = timed(lambda: eng.hip.recon_counts(len(tally.columns)))
        if i:
            dev_ms.append(d)
            recon_ms.append(r)
            cnt_ms.append(k)
        print(f"[tally_bench] device call {i}: {d:.2f} ms (reconstruction {r:.3f}, counters {k:.3f})", file=sys.stderr, flush=True)
    still_ahead = tr._dev is eng
    same = bool(np.array_equal(dev_counts, analysis.accuracy_counts(lw, tr, dirty, clean)))
    nb = len(lw.blocks)
    recon_bytes = 4 * n * (nb + len(tally.columns))  # referents read once per block + one store per cell (table gathers hit cache)
    cnt_bytes = 3 * 4 * n * len(tally.columns)
    res["device"] = {"columns_on_device": len(tally.columns), "equals_host_counts": same, "no_pull": still_ahead,
                     "accuracy_counts_ms": statistics.median(dev_ms),
                     "recon_kernel": {"ms": statistics.median(recon_ms), "bytes": recon_bytes,
                                      "frac_hbm_peak": recon_bytes / (1e-3 * statistics.median(recon_ms)) / HBM_PEAK},
                     "counts_kernel": {"ms": statistics.median(cnt_ms), "bytes": cnt_bytes,
                                       "frac_hbm_peak": cnt_bytes / (1e-3 * statistics.median(cnt_ms)) / HBM_PEAK}}
    res["host_over_device"] = res["host"]["total_ms"] / res["device"]["accuracy_counts_ms"]

    # ---- ring: add + consensus --------------------------------------------------------------------------------------
    for _ in range(args.keep):
        advance()
        tally.add(tr)
    both, add_ms, cons_ms, kern_ms = [], [], [], []
    for i in range(args.calls + 1):
        advance()
        _, a = timed(lambda: tally.add(tr))
        _, f = timed(tally.consensus)
        _, k = timed(lambda: eng.hip.ring_consensus(tally._ring, fetch=False))
        if i:
            add_ms.append(a)
            cons_ms.append(f)
            kern_ms.append(k)
            both.append(a + f)
        print(f"[tally_bench] ring call {i}: add {a:.3f} ms, consensus with copy-back {f:.2f} ms, kernel {k:.3f} ms", file=sys.stderr,
              flush=True)
    cells = n * len(tally.columns)
    cons_bytes = 4 * cells * (tally.n_kept + 2)
    res["ring"] = {"n_kept": tally.n_kept, "ring_bytes": 4 * cells * args.keep, "add_ms": statistics.median(add_ms),
                   "consensus_with_copy_back_ms": statistics.median(cons_ms), "add_plus_consensus_ms": statistics.median(both),
                   "consensus_kernel": {"ms": statistics.median(kern_ms), "bytes": cons_bytes,
                                        "frac_hbm_peak": cons_bytes / (1e-3 * statistics.median(kern_ms)) / HBM_PEAK},
                   "add_kernel": {"ms": statistics.median(add_ms), "bytes": recon_bytes,
                                  "frac_hbm_peak": recon_bytes / (1e-3 * statistics.median(add_ms)) / HBM_PEAK}}
    last = analysis.f1_from_counts(analysis.accuracy_counts(lw, tr, dirty, clean))
    res["f1_last_sample"] = last["f1"]
    res["f1_consensus"] = tally.consensus_accuracy(dirty, clean)["f1"]
    tally.close()
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
