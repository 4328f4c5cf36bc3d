"""Time one evaluation of a 51 x 4 800 product leaf with two AddTypos terms over 2 600 items (the bench's new rows per
sweep) through enum_product_kernel and through the generic kernels (PCLEAN_NO_PRODUCT_LEAF=1: the switch is read once per
process, so each path runs in a child process on the same inputs).  One call = pclean_score_node with one draw per item.
The figure is the wall clock of the synchronous call: it starts after a synchronising call and ends when the library's
stream has been synchronised and log-marginals and draws are on the host — END TO END (ctypes, scratch, the copy back of
2 600 doubles and ints), not an event bracket around the launch alone.  Median of five calls after a warm-up, on one GPU;
all five values are kept.  Writes profiles/product_leaf_bench.json.

    python scripts/product_leaf_bench.py
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NA, NB, ITEMS, CALLS = 51, 4800, 2600, 5


def child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import hashlib

    import numpy as np

    import indexed_program as ip
    from pclean_amd.engine import Engine
    S = ip.product_shape_program(NA, NB, n_rows=ITEMS)
    eng = Engine(S["lw"], S["obs"], dist_mode=1)
    try:
        eng.upload_trace(S["trace"])
        rows = np.arange(ITEMS, dtype=np.int32)
        eng.hip.set_profiling(True)
        lse, _, draws = eng.hip.score_node(0, 1, rows, n_cand=NA * NB, n_draws=1, seed=1)  # warm-up (synchronises)
        phases = sorted(p for p in eng.hip.get_profile() if p.startswith("enum_leaf"))
        eng.hip.set_profiling(False)
        ms = []
        for _ in range(CALLS):
            t0 = time.perf_counter()
            lse, _, draws = eng.hip.score_node(0, 1, rows, n_cand=NA * NB, n_draws=1, seed=1)
            ms.append(1e3 * (time.perf_counter() - t0))
        h = hashlib.sha256(np.ascontiguousarray(lse).tobytes() + np.ascontiguousarray(draws).tobytes()).hexdigest()
        print("RESULT", json.dumps(dict(ms=ms, median_ms=statistics.median(ms), phases=phases, digest=h)))
    finally:
        eng.close()


def main():
    out = {}
    for name, extra in (("product_kernel", {}), ("generic_kernels", {"PCLEAN_NO_PRODUCT_LEAF": "1"})):
        env = dict(os.environ)
        env.pop("PCLEAN_NO_PRODUCT_LEAF", None)
        env.update(extra)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.exit(r.stderr[-3000:])
        out[name] = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT")][-1][7:])
    res = dict(shape=[NA, NB], options=NA * NB, items=ITEMS, terms=2, calls=CALLS,
               what="pclean_score_node of the leaf, one draw per item, wall clock of a synchronous call (ms)",
               identical_outputs=out["product_kernel"]["digest"] == out["generic_kernels"]["digest"],
               ratio_generic_over_product=out["generic_kernels"]["median_ms"] / out["product_kernel"]["median_ms"], **out)
    path = os.path.join(ROOT, "profiles", "product_leaf_bench.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
