"""evaluate_accuracy and evaluate_accuracy_up_to (src/analysis.jl:36-143) over the flat trace, vectorised.

Counts follow the reference exactly: `errors` over every column common to the
dirty and clean tables (queried or not), `changed` / `cleaned` over queried
columns, imputations for missing dirty cells; F1 = harmonic mean.
"""
import numpy as np


def reconstructed_pool_ids(lowered, trace, row_slice=None, columns=None):
    """{query column: pool id of the value PClean currently believes, per local row}.  columns: only those (default all)."""
    lw = lowered
    m, q = lw.model, lw.query
    ocls = m.classes[q.cls]
    fk_block = {blk["root_fk"]: bi for bi, blk in enumerate(lw.blocks) if not blk.get("score")}
    out = {}
    for col, ref in q.cleanmap.items():
        if columns is not None and col not in columns:
            continue
        own = ocls.attr(ref) if "." not in ref else None
        if own is not None and ref in getattr(lw, "own_leaf", {}):  # own choice of a flat class: a row of trace.own
            li = [a for a, _, _ in trace.own_leaves()].index(ref)
            v = trace.own[li]  # (pulled from the device when the sweeps left it ahead)
            out[col] = np.where(v >= 0, lw.latent_dom[(q.cls, ref)].id_array()[np.maximum(v, 0)], -1)
            continue
        if own is not None and own.kind == "choice":  # own discrete choice (e.g. br): option -> string
            bi = next(iter(lw.locals))
            li = lw.locals[bi].index(ref)
            dom = lw.latent_dom[(q.cls, ref)]
            # (own choices are host-owned even while device commits are ahead of the trace's other arrays: no pull)
            loc = getattr(trace, "_locals", None) or trace.locals
            out[col] = dom.id_array()[np.maximum(loc[bi][:, li], 0)]
            continue
        gi = None
        if own is not None and own.kind == "julia":  # a queried numeric column is reported through its own Gaussian term
            gi = next((g for g, sp in enumerate(lw.gauss_specs) if sp["gauss_attr"] == q.obsmap[col]), None)
        if gi is not None:
            # corrected = round(unit.backward(x)) (experiments/rents/run.jl:25): numeric, compared as a number
            spec = lw.gauss_specs[gi]
            if "leaf" in spec:  # a flat class: the unit is an own choice, a row of trace.own (a row without values: option 0)
                n = trace._own.shape[1]
                u = np.zeros(n, dtype=np.int32)
                if spec["t_local"] is not None:
                    unit = spec["locals"][spec["t_local"]]
                    u = np.maximum(trace.own[[a for a, _, _ in trace.own_leaves()].index(unit)], 0)
                out[col] = ("numeric", np.round(lw.gauss_backward(np.arange(n), u, gi)))
                continue
            bi = lw.gauss_block
            u = (np.zeros(trace.cur.shape[1], dtype=np.int32) if spec["t_local"] is None  # AddNoise: round(x)
                 else np.maximum(trace.locals[bi][:, spec["t_local"]], 0))
            out[col] = ("numeric", np.round(lw.gauss_backward(np.arange(trace.cur.shape[1]), u, gi)))
            continue
        if "." in ref:
            head, rest = ref.split(".", 1)
            bi = fk_block[head]
            cname = lw.blocks[bi]["root_class"]
            t = trace.tables[cname]
            vals = t.cols[lw.colidx[cname][rest], trace.cur[bi]]
            c2, a2 = m.resolve(cname, rest)
            out[col] = lw.latent_dom[(c2, a2.name)].id_array()[vals]
        else:
            j = ocls.attr(ref)  # julia node: recompute from its arguments
            parts = []
            for arg in j.args:
                head, rest = arg.split(".", 1)
                bi = fk_block[head]
                cname = lw.blocks[bi]["root_class"]
                t = trace.tables[cname]
                c2, a2 = m.resolve(cname, rest)
                dom = lw.latent_dom[(c2, a2.name)]
                parts.append([dom.string(v) for v in t.cols[lw.colidx[cname][rest], trace.cur[bi]]])
            strs = [j.fn(*xs) for xs in zip(*parts)]
            out[col] = np.array([lw.pool.index.get(s, -2) for s in strs], dtype=np.int64)
    return out


def _pool_ids(index, values, unknown, missing):
    """Pool id of every value (object array of str / None): `unknown` for strings outside the pool,
    `missing` for None — looked up once per distinct value."""
    import pandas as pd
    codes, uniques = pd.factorize(values, use_na_sentinel=True)
    table = np.array([index.get(u, unknown) for u in uniques] + [missing], dtype=np.int64)
    return table[codes]  # code -1 (None) selects the last entry


def accuracy_counts(lowered, trace, dirty, clean, skip=()):
    """The five counters of evaluate_accuracy for the rows held by `trace`.  skip: columns left out altogether (somebody
    else counts them: tally.CellTally, on the device)."""
    lw = lowered
    ours = reconstructed_pool_ids(lw, trace, columns=None if not skip else
                                  [c for c in lw.query.cleanmap if c not in skip])
    cur = getattr(trace, "_cur", None)  # (the shape only: no pull of a trace the device is ahead of)
    n = (trace.cur if cur is None else cur).shape[1]
    return counts_given(lw, ours, n, dirty, clean, skip)


def counts_given(lowered, ours, n, dirty, clean, skip=()):
    """The five counters for a cleaned table given as `ours` (what reconstructed_pool_ids returns: pool ids per string
    column, ("numeric", values) per numeric one) over the first n rows; columns of `skip` are left out altogether."""
    return _counts_up_to(lowered, ours, n, dirty, clean, n, skip)[:5]


def counts_given_up_to(lowered, ours, n, dirty, clean, n_up_to, skip=()):
    """counts_given when only the first n_up_to of the n rows have been cleaned (evaluate_accuracy_up_to,
    analysis.jl:90-143): six counters [errors, changed, cleaned, imputed, imputed_ok, missing].  Rows >= n_up_to add to
    `errors` and `missing` only; `missing` = every missing dirty cell of a queried column whose clean cell is present."""
    return _counts_up_to(lowered, ours, n, dirty, clean, n_up_to, skip)


def _counts_up_to(lowered, ours, n, dirty, clean, n_up_to, skip=()):
    lw = lowered
    errors = changed = cleaned = imputed = imputed_ok = missing = 0
    done = np.arange(n) < n_up_to  # rows the cleaned table holds (`ours !== nothing`)
    for col in clean:
        if col not in dirty or col in skip:
            continue
        d = np.asarray(dirty[col][:n], dtype=object)
        c = np.asarray(clean[col][:n], dtype=object)
        dmiss = np.equal(d, None)
        ne = d != c  # element-wise Python comparison (None == None, None != any string)
        errors += int(np.sum(ne & ~dmiss))
        if col not in ours:
            continue
        if isinstance(ours[col], tuple):  # numeric column: compare numbers (Float64 == Int in the reference)
            o = ours[col][1]
            dn = np.array([np.nan if v is None else float(v) for v in d])
            cn = np.array([np.nan if v is None else float(v) for v in c])
            errors -= int(np.sum(ne & ~dmiss))
            errors += int(np.sum((dn != cn) & ~dmiss))
            ch = done & (~dmiss) & (o != dn)
            changed += int(np.sum(ch))
            cleaned += int(np.sum(ch & (o == cn)))
            imputed += int(np.sum(done & dmiss & ~np.isnan(cn)))  # analysis.jl:52-60 counts numeric imputations too
            imputed_ok += int(np.sum(done & dmiss & (o == cn)))
            missing += int(np.sum(dmiss & ~np.isnan(cn)))
            continue
        d_id = _pool_ids(lw.pool.index, d, -3, -4)
        c_id = _pool_ids(lw.pool.index, c, -5, -6)
        o = ours[col]
        cmiss = c_id == -6
        imputed += int(np.sum(done & dmiss & ~cmiss))
        imputed_ok += int(np.sum(done & dmiss & ~cmiss & (o == c_id)))
        missing += int(np.sum(dmiss & ~cmiss))
        ch = done & (~dmiss) & (o != d_id)
        changed += int(np.sum(ch))
        cleaned += int(np.sum(ch & (o == c_id)))
    return np.array([errors, changed, cleaned, imputed, imputed_ok, missing], dtype=np.int64)


def f1_from_counts(cnt):
    errors, changed, cleaned, imputed, imputed_ok = [float(x) for x in cnt]
    num = cleaned + imputed_ok
    precision = num / (changed + imputed) if (changed + imputed) > 0 else float("nan")
    recall = num / (errors + imputed) if (errors + imputed) > 0 else float("nan")
    f1 = 2.0 / (1 / precision + 1 / recall) if num > 0 else 0.0
    return dict(f1=f1, errors=int(errors), changed=int(changed), cleaned=int(cleaned), precision=precision,
                recall=recall, imputed=int(imputed), correctly_imputed=int(imputed_ok))


def evaluate_accuracy(lowered, trace, dirty, clean):
    return f1_from_counts(accuracy_counts(lowered, trace, dirty, clean))


def f1_from_counts_up_to(cnt):
    """The fields evaluate_accuracy_up_to returns (analysis.jl:137-142) from its six counters: recall is taken over
    errors + missing — every missing cell, cleaned yet or not — while `imputed` counts the cleaned rows' only."""
    errors, changed, cleaned, imputed, imputed_ok, missing = [float(x) for x in cnt]
    num = cleaned + imputed_ok
    precision = num / (changed + imputed) if (changed + imputed) > 0 else float("nan")
    recall = num / (errors + missing) if (errors + missing) > 0 else float("nan")
    f1 = 2.0 / (1 / precision + 1 / recall) if num > 0 else 0.0
    return dict(f1=f1, errors=int(errors), changed=int(changed), cleaned=int(cleaned), precision=precision,
                recall=recall, imputed=int(imputed), correctly_imputed=int(imputed_ok))


def accuracy_counts_up_to(lowered, trace, dirty, clean, n, skip=()):
    """The six counters of evaluate_accuracy_up_to for the rows held by `trace` when only the first n have been cleaned
    (n beyond the trace's rows: all of them)."""
    lw = lowered
    ours = reconstructed_pool_ids(lw, trace, columns=None if not skip else
                                  [c for c in lw.query.cleanmap if c not in skip])
    cur = getattr(trace, "_cur", None)  # (the shape only, as accuracy_counts)
    rows = (trace.cur if cur is None else cur).shape[1]
    return counts_given_up_to(lw, ours, rows, dirty, clean, n, skip)


def evaluate_accuracy_up_to(lowered, trace, dirty, clean, n):
    """evaluate_accuracy_up_to(dirty, clean, table, query, N) (analysis.jl:90-143): the accuracy when only the first n rows
    have been cleaned — the "F1 against rows processed" curve of the initialisation."""
    return f1_from_counts_up_to(accuracy_counts_up_to(lowered, trace, dirty, clean, n))


def _render_numbers(values):
    return [None if np.isnan(v) else (int(v) if float(v).is_integer() else float(v)) for v in values]


def reconstructed_table(lowered, trace, dirty):
    """The cleaned table: every queried column replaced by what PClean believes, the others copied
    (the DataFrame save_results writes, analysis.jl:21-30).  Values come back as strings / numbers."""
    lw = lowered
    ours = reconstructed_pool_ids(lw, trace)
    n = trace.cur.shape[1]
    out = {}
    for col, vals in dirty.items():
        if col not in ours:
            out[col] = list(vals[:n])
        elif isinstance(ours[col], tuple):
            out[col] = _render_numbers(ours[col][1])
        else:
            out[col] = [lw.pool.strings[i] if i >= 0 else None for i in ours[col]]
    return out


def consensus_table(lowered, tally, dirty):
    """The cleaned table from the per-cell consensus of `tally` (tally.CellTally) instead of the last sample: every queried
    string column holds its most frequent value over the kept samples and is followed by `<column>__support`, the number
    of kept samples that agree with it (of tally.n_kept).  A tally made with own=True serves the numeric queried columns
    too (the number under the most frequent Transformation option, rendered as reconstructed_table renders it, and its
    support); without it they are not tallied: like the columns that are not queried they are copied from `dirty`."""
    ids, support = tally.consensus()
    n = len(support[next(iter(support))]) if ids else 0
    strings = lowered.pool.strings
    out = {}
    for col, vals in dirty.items():
        if col not in ids:
            out[col] = list(vals[:n]) if ids else list(vals)
            continue
        out[col] = (_render_numbers(ids[col][1]) if isinstance(ids[col], tuple)
                    else [strings[i] if i >= 0 else None for i in ids[col]])
        out[col + "__support"] = [int(v) for v in support[col]]
    return out


def _map_columns(lowered, marginals):
    """[(query column, own choice)] of the queried own choices that `marginals` (Engine.own_marginals) covers"""
    return [(col, ref) for col, ref in lowered.query.cleanmap.items() if ref in marginals]


def map_pool_ids(lowered, marginals):
    """{query column: pool id of the most probable option of its own choice per row} from Engine.own_marginals — the
    encoding counts_given takes; -1 where no option is possible."""
    out = {}
    for col, ref in _map_columns(lowered, marginals):
        k = np.asarray(marginals[ref][0][0])
        out[col] = np.where(k >= 0, lowered.latent_dom[(lowered.query.cls, ref)].id_array()[np.maximum(k, 0)], -1)
    return out


def _thresholded_ids(lowered, marginals, dirty, min_confidence):
    """map_pool_ids with the cells whose MAP probability is below min_confidence put back to their dirty value (-3: a
    dirty string outside the pool, as counts_given reads it); a missing dirty cell always takes the MAP value.  Also
    {query column: MAP probability}."""
    ids, conf = map_pool_ids(lowered, marginals), {}
    for col, ref in _map_columns(lowered, marginals):
        conf[col] = np.asarray(marginals[ref][1][0], dtype=np.float64)
        d = np.asarray(dirty[col][:len(ids[col])], dtype=object)
        keep_dirty = (conf[col] < min_confidence) & ~np.equal(d, None)
        ids[col] = np.where(keep_dirty, _pool_ids(lowered.pool.index, d, -3, -4), ids[col])
    return ids, conf


def _map_numeric(lowered, marginals, dirty, min_confidence=0.0):
    """{query column: (values float64, MAP probability)} of the queried numeric columns of a flat class whose Gaussian term
    chooses a unit: round(unit.backward(x)) under the MAP unit — the unit of the most probable option of the Gaussian leaf,
    so the confidence is that option's JOINT probability (Engine.own_marginals) — where it is >= min_confidence, the dirty
    number otherwise; NaN where the number is missing."""
    lw = lowered
    ocls = lw.model.classes[lw.query.cls]
    out = {}
    for col, ref in lw.query.cleanmap.items():
        if "." in ref or ocls.attr(ref).kind != "julia":
            continue
        gi = next((g for g, sp in enumerate(lw.gauss_specs) if sp["gauss_attr"] == lw.query.obsmap[col] and "leaf" in sp), None)
        if gi is None or lw.gauss_specs[gi]["t_local"] is None:
            continue
        spec = lw.gauss_specs[gi]
        unit = spec["locals"][spec["t_local"]]
        if unit not in marginals:
            continue
        k = np.asarray(marginals[unit][0][0])
        conf = np.asarray(marginals[unit][1][0], dtype=np.float64)
        n = len(k)
        vals = np.round(lw.gauss_backward(np.arange(n), np.maximum(k, 0), gi))
        x = lw.xnum[spec["x_col"], :n]
        out[col] = (np.where((k < 0) | (conf < min_confidence), x, vals), conf)
    return out


def map_table(lowered, marginals, dirty, min_confidence=0.0):
    """(table, confidence): the cleaned table whose queried own choices hold their most probable option (the MAP string
    of the cell's exact conditional) where its probability is >= min_confidence and the dirty cell otherwise — a missing
    dirty cell always takes the MAP value; every other column is copied.  confidence {query column: MAP probability}.
    A choice indexed by a sibling choice and that index (one product leaf): the two cells hold the most probable PAIR, and
    the confidence of both is the pair's JOINT probability, not a per-column marginal (Engine.own_marginals) — so
    min_confidence keeps or drops the two cells of a row on the same number.  A Gaussian leaf of a flat class (a string
    choice and a unit, or one of them): the string cell holds the string of the most probable option, and the queried
    numeric cell is reported under that option's unit, round(unit.backward(x)), with the same joint confidence
    (_map_numeric)."""
    ids, conf = _thresholded_ids(lowered, marginals, dirty, min_confidence)
    nums = _map_numeric(lowered, marginals, dirty, min_confidence)
    for col, (_, p) in nums.items():
        conf[col] = p
    n = len(next(iter(conf.values()))) if conf else None
    strings = lowered.pool.strings
    out = {}
    for col, vals in dirty.items():
        if col in nums:
            out[col] = _render_numbers(nums[col][0])
            continue
        if col not in ids:
            out[col] = list(vals[:n])
            continue
        out[col] = [vals[i] if k == -3 else (strings[k] if k >= 0 else None) for i, k in enumerate(ids[col])]
    return out, conf


def evaluate_map_accuracy(lowered, marginals, dirty, clean, min_confidence=0.0):
    """evaluate_accuracy of map_table(lowered, marginals, dirty, min_confidence); for the two columns of a product leaf
    min_confidence is compared with the pair's joint probability (see map_table)"""
    ids, conf = _thresholded_ids(lowered, marginals, dirty, min_confidence)
    for col, (vals, p) in _map_numeric(lowered, marginals, dirty, min_confidence).items():
        ids[col], conf[col] = ("numeric", vals), p
    n = len(next(iter(conf.values())))
    return f1_from_counts(counts_given(lowered, ids, n, dirty, clean))


def latent_table(lowered, trace, cname):
    """One inferred latent table (save_tables, analysis.jl:8-13): row id + the value of every own attribute and
    reference slot of the class (flattened copies of referents' values are left out, as the reference does
    for its '#'-named inlined nodes)."""
    lw = lowered
    t = trace.tables[cname]
    live = np.nonzero(t.live[:t.n])[0]
    out = {"id": [int(k) for k in live]}
    for j, c in enumerate(lw.layout[cname]):
        if "." in c.name:
            continue
        if c.kind == "fk":
            out[c.name] = [int(v) for v in t.cols[j, live]]
        else:
            dom = lw.latent_dom[(cname, c.name)]
            out[c.name] = [dom.string(v) for v in t.cols[j, live]]
    return out


def map_confidence_table(lowered, marginals, dirty):
    """map_table with every queried own column followed by `<column>__confidence`, its MAP probability"""
    table, conf = map_table(lowered, marginals, dirty)
    out = {}
    for col, vals in table.items():
        out[col] = vals
        if col in conf:
            out[col + "__confidence"] = [float(p) for p in conf[col]]
    return out


def save_results(directory, name, lowered, trace, dirty, timestamp=True, tally=None, marginals=None):
    """save_results (analysis.jl:15-33): reconstructed_<class>.csv + inferred_<class>.csv per latent class; with a
    tally (tally.CellTally) also consensus_<class>.csv (consensus_table); with marginals (Engine.own_marginals of a flat
    class) also map_<class>.csv (map_confidence_table)."""
    import datetime
    import os

    import pandas as pd
    d = os.path.join(directory, f"{name}-{datetime.datetime.now().isoformat()}" if timestamp else name)
    os.makedirs(d, exist_ok=True)
    pd.DataFrame(reconstructed_table(lowered, trace, dirty)).to_csv(
        os.path.join(d, f"reconstructed_{lowered.query.cls}.csv"), index=False)
    if tally is not None:
        pd.DataFrame(consensus_table(lowered, tally, dirty)).to_csv(
            os.path.join(d, f"consensus_{lowered.query.cls}.csv"), index=False)
    if marginals is not None:
        pd.DataFrame(map_confidence_table(lowered, marginals, dirty)).to_csv(
            os.path.join(d, f"map_{lowered.query.cls}.csv"), index=False)
    for cname in trace.tables:
        pd.DataFrame(latent_table(lowered, trace, cname)).to_csv(os.path.join(d, f"inferred_{cname}.csv"), index=False)
    return d
