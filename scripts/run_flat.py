"""A flat program on the HIP path: the City, State and Condition columns of datasets/hospital_*.csv as three own blocks of
one observed class (experiments.flat_model) — the vocabulary of a column is the clean file's distinct values, every dirty
cell an AddTypos observation of its row's choice.  initialize_trace + run_inference + accuracy.

--map: after the last sweep, the exact conditional of every cell given the final parameters (Engine.own_marginals) — the
accuracy and F1 of its most probable value next to the last sample's, and with the cells whose MAP probability lies below
0.5 / 0.9 left at their dirty value.

usage: run_flat.py [particles] [pg|mh] [iterations] [rows] [--map]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pclean_amd import experiments as ex
from pclean_amd.analysis import evaluate_accuracy, evaluate_map_accuracy, map_table, reconstructed_table
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import initialize_trace, run_inference
from pclean_amd.model import LoweredModel
from pclean_amd.trace import Trace


def main(particles=20, mh=False, iters=5, n_rows=None, seed=0, verbose=True, with_map=False):
    dirty, clean = ex.hospital_data()
    cols = ex.FLAT_COLUMNS
    n = len(dirty[cols[0]]) if n_rows is None else int(n_rows)
    dirty = {c: dirty[c][:n] for c in cols}
    clean = {c: clean[c][:n] for c in cols}
    m = ex.flat_model(ex.flat_vocabulary(clean))
    lw = LoweredModel(m, ex.flat_query(m), dirty)
    eng = Engine(lw, lw.encode_observations(dirty))
    try:
        tr = Trace(lw, n, seed)
        cfg = InferenceConfig(iters, particles, use_mh_instead_of_pg=mh)
        t0 = time.time()
        initialize_trace(eng, tr, cfg, seed)
        t1 = time.time()
        run_inference(eng, tr, cfg, seed)
        t2 = time.time()
        tr.check_consistency()
        acc = evaluate_accuracy(lw, tr, dirty, clean)
        acc["accuracy"] = ex.cell_accuracy(reconstructed_table(lw, tr, dirty), clean)
        if verbose:
            st = eng.hip.get_own_stats()
            print(f"{n} rows, {iters} iterations, {particles} particles ({'MH' if mh else 'PG'}): init {t1 - t0:.2f}s, "
                  f"inference {t2 - t1:.2f}s; last window: {st.n_runs} tuple runs, longest {st.longest_run} rows")
            print(f"accuracy {acc['accuracy']:.4f} (dirty: {ex.cell_accuracy(dirty, clean):.4f})  F1 {acc['f1']:.4f}")
            print(acc)
        if with_map:
            marg = eng.own_marginals(tr, top=1)
            acc["map"] = {}
            for thr in (0.0, 0.5, 0.9):
                table, conf = map_table(lw, marg, dirty, min_confidence=thr)
                a = evaluate_map_accuracy(lw, marg, dirty, clean, min_confidence=thr)
                a["accuracy"] = ex.cell_accuracy(table, clean)
                present = {c: np.array([v is not None for v in dirty[c]]) for c in cols}
                a["left_dirty"] = sum(int(((conf[c] < thr) & present[c]).sum()) for c in cols) / float(n * len(cols))
                acc["map"][thr] = a
                if verbose:
                    what = "MAP" if thr == 0.0 else f"MAP at min_confidence {thr}"
                    print(f"{what}: accuracy {a['accuracy']:.4f}  F1 {a['f1']:.4f}" +
                          (f"  ({100 * a['left_dirty']:.2f} % of the cells left at their dirty value)" if thr else ""))
        return acc
    finally:
        eng.close()


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if x != "--map"]
    main(with_map="--map" in sys.argv[1:], particles=int(a[0]) if a else 20, mh=(a[1] == "mh") if len(a) > 1 else False, iters=int(a[2]) if len(a) > 2 else 5,
         n_rows=int(a[3]) if len(a) > 3 else None)
