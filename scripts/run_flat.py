"""A flat program on the HIP path: the City, State and Condition columns of datasets/hospital_*.csv as three own blocks of
one observed class (experiments.flat_model) — the vocabulary of a column is the clean file's distinct values, every dirty
cell an AddTypos observation of its row's choice.  initialize_trace + run_inference + accuracy.

--map: after the last sweep, the exact conditional of every cell given the final parameters (Engine.own_marginals) — the
accuracy and F1 of its most probable value next to the last sample's, and with the cells whose MAP probability lies below
0.5 / 0.9 left at their dirty value.

--dependent: the same run twice, first as above and then with State indexed by City (experiments.flat_model(dependent=("City",
"State")): the two choices share one block and one product leaf, State's parameter is an IndexedProportionsParameter), and
the accuracy of the two models side by side — of the last sample and, with the joint MAP repair (Engine.own_marginals:
for the pair these are JOINT probabilities), per column.

--star: City with State AND CountyName as its dependents (experiments.flat_model(star=("City", ("State", "CountyName"))),
lowered with own_star=True: a head node and two arm nodes, enumerated collapsed by own_star_kernel) next to the independent
model over the same four columns: accuracy of the last sample and of the MAP repair (the index's exact marginal; a
dependent's most probable value GIVEN the index's most probable value).  Reported, not asserted.

--numeric: another table — Room Type and Monthly Rent of datasets/rents_*.csv as ONE own block with a Gaussian observation
(experiments.flat_numeric_model: the rent's mean depends on the room type, some rents are stated in thousands): no latent
class.  Prints the accuracy and F1 of the last sample and of the MAP repair (the numeric cell under the MAP unit); the
figures are reported, not asserted.

usage: run_flat.py [particles] [pg|mh] [iterations] [rows] [--map] [--dependent] [--star] [--numeric]"""
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


def main(particles=20, mh=False, iters=5, n_rows=None, seed=0, verbose=True, with_map=False, dependent=None, star=None,
         cols=ex.FLAT_COLUMNS):
    dirty, clean = ex.hospital_data()
    n = len(dirty[cols[0]]) if n_rows is None else int(n_rows)
    dirty = {c: dirty[c][:n] for c in cols}
    clean = {c: clean[c][:n] for c in cols}
    m = ex.flat_model(ex.flat_vocabulary(clean, cols), dependent=dependent, star=star)
    lw = LoweredModel(m, ex.flat_query(m, cols), dirty, own_star=star is not None)
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
        acc["accuracy"] = ex.cell_accuracy(reconstructed_table(lw, tr, dirty), clean, cols)
        if verbose:
            st = eng.hip.get_own_stats()
            print(f"{n} rows, {iters} iterations, {particles} particles ({'MH' if mh else 'PG'}): init {t1 - t0:.2f}s, "
                  f"inference {t2 - t1:.2f}s; last window: {st.n_runs} tuple runs, longest {st.longest_run} rows")
            print(f"accuracy {acc['accuracy']:.4f} (dirty: {ex.cell_accuracy(dirty, clean, cols):.4f})  F1 {acc['f1']:.4f}")
            print(acc)
        if with_map:
            marg = eng.own_marginals(tr, top=1)
            acc["map"] = {}
            for thr in (0.0, 0.5, 0.9):
                table, conf = map_table(lw, marg, dirty, min_confidence=thr)
                a = evaluate_map_accuracy(lw, marg, dirty, clean, min_confidence=thr)
                a["accuracy"] = ex.cell_accuracy(table, clean, cols)
                a["by_column"] = {c: ex.cell_accuracy(table, clean, (c,)) for c in cols}
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


def numeric(particles=20, mh=False, iters=5, n_rows=None, seed=0, verbose=True):
    dirty, clean = ex.rents_data()
    cols = ex.FLAT_NUMERIC_COLUMNS
    n = len(dirty[cols[0]]) if n_rows is None else int(n_rows)
    dirty = {c: dirty[c][:n] for c in cols}
    clean = {c: clean[c][:n] for c in cols}
    rooms = list(dict.fromkeys(v for v in clean["Room Type"] if v is not None))
    m = ex.flat_numeric_model(rooms)
    lw = LoweredModel(m, ex.flat_numeric_query(m), dirty)
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

        def numbers(table):  # (the clean file holds the rents as integers in text, the cleaned table as numbers)
            same = lambda a, b: (a is None and b is None) or (a is not None and b is not None and float(a) == float(b))  # noqa: E731
            return {"Room Type": sum(a == b for a, b in zip(table["Room Type"], clean["Room Type"])) / float(n),
                    "Monthly Rent": sum(same(a, b) for a, b in zip(table["Monthly Rent"], clean["Monthly Rent"])) / float(n)}
        acc = evaluate_accuracy(lw, tr, dirty, clean)
        acc["by_column"] = numbers(reconstructed_table(lw, tr, dirty))
        marg = eng.own_marginals(tr, top=1)
        table, conf = map_table(lw, marg, dirty)
        acc["map"] = evaluate_map_accuracy(lw, marg, dirty, clean)
        acc["map"]["by_column"] = numbers(table)
        acc["mean_rent"] = dict(zip(rooms, (float(v) for v in tr.mean_params[0].value)))
        if verbose:
            st = eng.hip.get_own_stats()
            print(f"{n} rows, {iters} iterations, {particles} particles ({'MH' if mh else 'PG'}): init {t1 - t0:.2f}s, "
                  f"inference {t2 - t1:.2f}s; kernel variants of the last call {st.variants}")
            print(f"dirty: {numbers(dirty)}")
            print(f"last sample: F1 {acc['f1']:.4f}  {acc['by_column']}")
            print(f"MAP:         F1 {acc['map']['f1']:.4f}  {acc['map']['by_column']}")
            print(f"mean rent per room type: {acc['mean_rent']}")
        return acc
    finally:
        eng.close()


def compare(star=False, **kw):
    """the independent model and the one with State indexed by City, side by side; star: over City, State, CountyName and
    Condition, the independent model, State | City alone, and the star State, CountyName | City"""
    out = {}
    cols = ex.FLAT_STAR_COLUMNS if star else ex.FLAT_COLUMNS
    runs = [("independent", {}), ("State | City", dict(dependent=("City", "State")))]
    if star:
        runs.append(("State, County | City", dict(star=ex.FLAT_STAR)))
    for name, how in runs:
        print(f"---- {name}")
        out[name] = main(with_map=True, cols=cols, **how, **kw)
    print(f"{'model':<22} {'sample acc':>10} {'MAP acc':>8} {'MAP F1':>7}  " + "  ".join(f"{c:>10}" for c in cols))
    for name, a in out.items():
        m0 = a["map"][0.0]
        print(f"{name:<22} {a['accuracy']:>10.4f} {m0['accuracy']:>8.4f} {m0['f1']:>7.4f}  " +
              "  ".join(f"{m0['by_column'][c]:>10.4f}" for c in cols))
    return out


if __name__ == "__main__":
    a = [x for x in sys.argv[1:] if x not in ("--map", "--dependent", "--numeric", "--star")]
    kw = dict(particles=int(a[0]) if a else 20, mh=(a[1] == "mh") if len(a) > 1 else False, iters=int(a[2]) if len(a) > 2 else 5,
              n_rows=int(a[3]) if len(a) > 3 else None)
    if "--numeric" in sys.argv[1:]:
        numeric(**kw)
    elif "--star" in sys.argv[1:]:
        compare(star=True, **kw)
    elif "--dependent" in sys.argv[1:]:
        compare(**kw)
    else:
        main(with_map="--map" in sys.argv[1:], **kw)
