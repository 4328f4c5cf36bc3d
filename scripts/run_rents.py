"""experiments/rents/run.jl on the HIP path.
`--consensus K` keeps the cleaned table of the last K iterations on the device (pclean_amd.tally.CellTally with own=True:
room types and the unit-corrected rent included) and prints the F1 of their per-cell consensus next to the last sample's."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from pclean_amd import experiments as ex
from pclean_amd.analysis import evaluate_accuracy
from pclean_amd.engine import Engine, InferenceConfig
from pclean_amd.inference import initialize_trace, run_inference
from pclean_amd.model import LoweredModel
from pclean_amd.trace import Trace


def main(n_rows=None, particles=2, mh=True, iters=1, seed=0, shuffle=True, consensus=0):
    dirty, clean = ex.rents_data()
    if shuffle:  # random row order for the batched initialisation (experiments.shuffle_rows)
        (dirty, clean), _ = ex.shuffle_rows([dirty, clean], seed)
    if n_rows:
        dirty = {c: v[:n_rows] for c, v in dirty.items()}
        clean = {c: v[:n_rows] for c, v in clean.items()}
    m = ex.rents_model(dirty)
    q = ex.rents_query(m)
    lw = LoweredModel(m, q, dirty)
    obs = lw.encode_observations(dirty)
    eng = Engine(lw, obs)
    tr = Trace(lw, obs.shape[1], seed)
    cfg = InferenceConfig(iters, particles, use_mh_instead_of_pg=mh, rejuv_frequency=500)
    t0 = time.time()
    initialize_trace(eng, tr, cfg, seed, max_batch=2048)
    tr.check_consistency()
    t1 = time.time()
    acc0 = evaluate_accuracy(lw, tr, dirty, clean)
    print(f"init {t1 - t0:.2f}s F1 {acc0['f1']:.4f}", {c: (t.n, t.n_live) for c, t in tr.tables.items()}, flush=True)
    tally = None
    if consensus:
        from pclean_amd.tally import CellTally
        tally = CellTally(eng, tr, keep=consensus, own=True)
    run_inference(eng, tr, cfg, seed, verbose=True, tally=tally, tally_from=max(0, iters - consensus))
    t2 = time.time()
    acc = evaluate_accuracy(lw, tr, dirty, clean)
    print(f"inference {t2 - t1:.2f}s", {c: (t.n, t.n_live) for c, t in tr.tables.items()})
    print(acc)
    if tally is not None:
        cacc = tally.consensus_accuracy(dirty, clean)
        print(f"last-sample F1 {acc['f1']:.4f}; consensus F1 over the last {tally.n_kept} iterations {cacc['f1']:.4f}")
        print("consensus:", cacc)
        acc = dict(acc, consensus=cacc)
        tally.close()
    eng.close()
    return acc


if __name__ == "__main__":
    a = sys.argv[1:]
    k = 0
    if "--consensus" in a:  # --consensus K: iterations kept for the per-cell consensus (at most 32)
        i = a.index("--consensus")
        k = int(a[i + 1])
        del a[i:i + 2]
    main(consensus=k, n_rows=int(a[0]) if a and int(a[0]) > 0 else None, particles=int(a[1]) if len(a) > 1 else 2,
         mh=(a[2] == "mh") if len(a) > 2 else True, iters=int(a[3]) if len(a) > 3 else 1,
         shuffle="sorted" not in a)
