"""The cleaned table where the sweeps leave their state, and a per-cell consensus over the last samples.

`analysis.reconstructed_pool_ids` walks the trace's host arrays; once sweeps are committed on the device that starts with
a pull of every latent table.  `CellTally` serves the same columns from the device-resident referents and tables
(csrc/recon.hip): the reconstruction, the five counters of evaluate_accuracy (analysis.jl:36-88), a ring of the last
`keep` reconstructions and, per cell, the most frequent kept value with its support — one posterior sample is a noisy
point estimate, and the sampler visits many states per run.  With own=True the observed class's own enumerated choices
and its numeric columns (reported through a Gaussian term) are served from the device as well, and `accuracy_up_to` gives
evaluate_accuracy_up_to (analysis.jl:90-143) from the same counter kernels with a row bound.
"""
import collections

import numpy as np

from . import _lib, analysis


def mode_support(snapshots):
    """Per cell of snapshots [S][M] (oldest first): (mode, support) = the most frequent value and how many snapshots hold
    it; among equally frequent values the one whose latest occurrence is the most recent snapshot wins (S = 1: the last
    sample; all distinct: the newest).  Host twin of the consensus kernel, used for the columns that stay on the host."""
    snaps = np.asarray(snapshots)
    s_n = snaps.shape[0]
    mode = snaps[s_n - 1].copy()
    support = np.zeros(snaps.shape[1:], dtype=np.int32)
    for s in range(s_n - 1, -1, -1):  # newest first: only a strictly larger count replaces what a newer value holds
        cnt = (snaps == snaps[s]).sum(axis=0).astype(np.int32)
        better = cnt > support
        mode[better] = snaps[s][better]
        support[better] = cnt[better]
    return mode, support


class ReconPlan:
    """Which queried columns the device reconstructs and how (pclean_recon_set_plan).
    columns: their names in plan order (the columns of one block follow each other, function-table columns last);
    cols / id_map: the C descriptors; host_strings: queried string columns that stay on the host (own enumerated choices,
    JuliaNodes without a function table); numeric: queried numeric columns (reported through a Gaussian term).
    own=True also plans the own enumerated choices of the observed class (kind "own": the option's pool id, from the own
    choices CellTally uploads) and the numeric columns (kind "num": the cell is the Transformation option the row holds,
    its value round(backward_u(x)) is materialised on the device) — after the path and function-table columns, in that
    order; `device_numeric` names the latter, and host_strings keeps only JuliaNodes without a function table."""

    def __init__(self, lowered, own=False):
        lw = lowered
        self.own = bool(own)
        m, q = lw.model, lw.query
        ocls = m.classes[q.cls]
        fk_block = {blk["root_fk"]: bi for bi, blk in enumerate(lw.blocks) if not blk.get("score")}
        paths, fns, owns, nums = [], [], [], []
        self.host_strings, self.numeric, self.device_numeric = [], [], []
        for col, ref in q.cleanmap.items():
            if "." in ref:
                head, rest = ref.split(".", 1)
                bi = fk_block[head]
                cname = lw.blocks[bi]["root_class"]
                c2, a2 = m.resolve(cname, rest)
                paths.append((bi, col, dict(kind=_lib.RECON_PATH, block=bi, table=lw.table_id[cname], col=lw.colidx[cname][rest]),
                              lw.latent_dom[(c2, a2.name)].id_array()))
                continue
            own = ocls.attr(ref)
            if own.kind == "julia" and any(sp["gauss_attr"] == q.obsmap[col] for sp in lw.gauss_specs):
                if self.own:  # term g of the block sits on its root node (0), in declaration order
                    if getattr(lw, "own_gauss", None):
                        raise NotImplementedError(f"{col}: the numeric column of a flat class (a Gaussian observation in an own "
                                                  "block) is not tallied on the device; CellTally(own=False) leaves it to the host")
                    g = next(g for g, sp in enumerate(lw.gauss_specs) if sp["gauss_attr"] == q.obsmap[col])
                    nums.append((col, dict(kind=_lib.RECON_NUM, block=lw.gauss_block, table=0, col=g), np.zeros(0, np.int32)))
                    self.device_numeric.append(col)
                else:
                    self.numeric.append(col)
                continue
            if ref in getattr(lw, "own_leaf", {}):  # own choice of a flat class: not served on the device, the host counts it
                self.host_strings.append(col)
                continue
            if self.own and own.kind == "choice":
                bi = next(iter(lw.locals))
                owns.append((col, dict(kind=_lib.RECON_OWN, block=bi, table=-1, col=lw.locals[bi].index(ref)),
                             lw.latent_dom[(q.cls, ref)].id_array()))
                continue
            ft = self._fn_table_of(lw, own, fk_block) if own.kind == "julia" else None
            if ft is None:
                self.host_strings.append(col)
            else:
                fns.append((col, ft[0], ft[1]))
        paths.sort(key=lambda p: p[0])  # (stable: one block's columns together, in query order)
        self.columns, self.cols, maps, off = [], [], [], 0
        for col, desc, idmap in [(p[1], p[2], p[3]) for p in paths] + fns + owns + nums:
            idmap = np.ascontiguousarray(idmap, dtype=np.int32)
            rc = _lib.ReconCol(block_b=-1, table_b=-1, col_b=-1, fn_table=-1)
            for k, v in desc.items():
                setattr(rc, k, int(v))
            rc.map_off, rc.map_len = off, len(idmap)
            off += len(idmap)
            maps.append(idmap)
            self.columns.append(col)
            self.cols.append(rc)
        self.id_map = np.concatenate(maps) if maps else np.zeros(0, dtype=np.int32)
        names = {_lib.RECON_PATH: "path", _lib.RECON_FN: "fn", _lib.RECON_OWN: "own", _lib.RECON_NUM: "num"}
        self.kinds = {c: names[rc.kind] for c, rc in zip(self.columns, self.cols)}
        # blocks whose own choices the device needs: every OWN column's, and a NUM column's unless its term has no Transformation
        self.local_blocks = sorted({rc.block for rc in self.cols if rc.kind == _lib.RECON_OWN} |
                                   {rc.block for rc in self.cols if rc.kind == _lib.RECON_NUM
                                    and lw.gauss_specs[rc.col]["t_local"] is not None})

    @staticmethod
    def _fn_table_of(lw, j, fk_block):
        """(descriptor, id map) of JuliaNode j when the lowering keeps its function table: f(one value of an earlier slot,
        one value of a later slot), tabulated over the two latent domains (fn[earlier][later] -> value of the node's own
        domain).  None: the node is recomputed on the host."""
        if len(j.args) != 2:
            return None
        for (obs, dom_key), (pid, _odom, jdom) in lw.pair_id.items():
            if dom_key != ("julia", j.name) or not hasattr(jdom, "id_array"):
                continue
            for ct in lw.cross_terms:
                if ct["pair"] != pid:
                    continue
                ca, cb = lw.blocks[ct["ctx_block"]]["root_class"], lw.blocks[ct["local_block"]]["root_class"]
                desc = dict(kind=_lib.RECON_FN, fn_table=ct["fn"],
                            block=ct["ctx_block"], table=lw.table_id[ca], col=lw.colidx[ca][ct["ctx_path"]],
                            block_b=ct["local_block"], table_b=lw.table_id[cb], col_b=lw.colidx[cb][ct["local_path"]])
                return desc, jdom.id_array()
        return None


def truth_ids(pool_index, dirty_col, clean_col):
    """(dirty ids, clean ids) of one column with the encoding of analysis.accuracy_counts: dirty -3 / -4 for a string
    outside the pool / a missing cell, clean -5 / -6.  A clean string outside the pool that equals its dirty cell is sent
    as -3: then "dirty != clean" is exactly "the ids differ" (pool strings are unique), and -3 equals no reconstruction."""
    d = np.asarray(dirty_col, dtype=object)
    c = np.asarray(clean_col, dtype=object)
    d_id = analysis._pool_ids(pool_index, d, -3, -4)
    c_id = analysis._pool_ids(pool_index, c, -5, -6)
    both = np.flatnonzero((d_id == -3) & (c_id == -5))
    if len(both):
        same = both[d[both] == c[both]]
        c_id[same] = -3
    return d_id.astype(np.int32), c_id.astype(np.int32)


class CellTally:
    """Device-side cleaned table, accuracy counters and per-cell consensus of one engine's observed rows.

    keep: how many of the last reconstructions the ring holds, 1 <= keep <= 32 (ValueError beyond).  The ring lives in HBM,
    int32 [keep][C][N] for C device-served columns and N rows: 4 * keep * C * N bytes — 1.9 GB at keep 32, 15 columns,
    10^6 rows — allocated by the first `add`.  Nothing here changes the trace or the sampler's state.

    The kept values are string pool ids.  When the lowered model is rebuilt (LoweredModel.relower, after strings were
    drawn for chosen dummy values) the pool is rebuilt too: after every Engine.reload the tally uploads its plan again and,
    unless the old pool's strings are a prefix of the new one's, translates the kept snapshots to the new ids.

    own=True (opt-in; without it plan, columns and answers are what they always were): the own enumerated choices of the
    observed class and the numeric columns reported through a Gaussian term are served from the device too
    (ReconPlan(lowered, own=True)).  The own choices are host-owned and always current (the engine writes them into the
    trace after every sweep, also while device commits are ahead): the tally uploads them — 8 bytes per row — into a
    buffer of the reconstruction state whenever they changed since its last upload; no Engine.pull.  A numeric column's
    kept cells are Transformation option indices: its consensus is the number under the most frequent option."""

    def __init__(self, engine, trace, keep=16, own=False):
        keep = int(keep)
        if not 1 <= keep <= _lib.RING_MAX_KEEP:
            raise ValueError(f"keep must be in 1..{_lib.RING_MAX_KEEP}, got {keep}")
        self.engine, self.lw, self.keep, self.own = engine, engine.lw, keep, bool(own)
        self.n_rows = int(trace._cur.shape[1])
        if engine.obs.shape[1] != self.n_rows or engine.row_offset:
            raise ValueError("CellTally needs an engine that holds every observed row of the trace")
        self._ring = None
        self._host_ring = collections.deque(maxlen=keep)  # {column: pool ids} of the host-only string columns
        self._adds = 0
        import weakref
        self._trace = weakref.ref(trace)  # (a numeric column's plan needs the Gaussian terms loaded: _upload_plan)
        self._install()

    # -- plan / pool bookkeeping --------------------------------------------------------------------------------------
    def _install(self):
        self.plan = ReconPlan(self.lw, own=True) if self.own else ReconPlan(self.lw)
        self.columns = list(self.plan.columns)
        self._num = [self.columns.index(c) for c in self.plan.device_numeric]  # plan positions of the numeric columns
        if self.columns:
            self._upload_plan()
        self._hip, self._reloads = self.engine.hip, self.engine.reloads
        self._pool = self.lw.pool  # (relower makes a new pool object: this one keeps the ids the kept snapshots hold)

    def _upload_plan(self):
        hip = self.engine.hip
        if self._num and getattr(self.engine, "_gauss_pending", False):
            # the library checks a numeric column against its Gaussian term, which a fresh context gets with the first
            # upload of a trace (it needs the mean tables)
            tr = self._trace()
            if tr is None or tr._dev is not None:
                raise _lib.PCleanHipError("CellTally(own=True): the engine has not loaded the Gaussian terms yet and the trace "
                                          "that would bring them is gone or ahead on a device")
            self.engine.upload_trace(tr)
        hip.recon_set_plan(self.plan.cols, self.plan.id_map)
        hip._recon_truth = None  # (a context's dirty / clean ids go with its plan; tallies of one engine share them)
        hip._recon_own = self.own

    def _ensure_plan(self):
        """tallies of one engine share its context's plan: put this one's back when a tally of the other kind (own or
        not) uploaded its own since"""
        if self.columns and getattr(self.engine.hip, "_recon_own", self.own) != self.own:
            self._upload_plan()

    def _refresh(self):
        """after an Engine.reload: the plan goes into the fresh context, kept snapshots follow the pool's ids"""
        if self._hip is self.engine.hip and self._reloads == self.engine.reloads and self._pool is self.lw.pool:
            return
        old = self._pool.strings
        self._install()
        new = self.lw.pool
        if new.strings[:len(old)] == old:
            return
        o2n = np.array([new.index.get(s, -2) for s in old], dtype=np.int32)
        if self._ring is not None:
            self.engine.hip.ring_remap(self._ring, o2n)
        for snap in self._host_ring:
            for col, ids in snap.items():
                snap[col] = np.where(ids >= 0, o2n[np.clip(ids, 0, max(len(o2n) - 1, 0))], ids) if len(o2n) else ids

    def _current(self, trace):
        if trace._cur.shape[1] != self.n_rows:
            raise ValueError("the trace holds another number of rows than the tally was made for")
        self._refresh()
        self._ensure_plan()
        self.engine.make_device_current(trace)
        if self.plan.local_blocks:
            hip = self.engine.hip
            sent = hip.__dict__.setdefault("_recon_locals", {})
            for bi in self.plan.local_blocks:
                loc = trace._locals[bi]  # (host-owned and current even while device commits are ahead: no pull)
                if bi not in sent or not np.array_equal(sent[bi], loc):
                    hip.recon_set_locals(bi, loc)
                    sent[bi] = np.array(loc, dtype=np.int32, copy=True)

    def _ensure_truth(self, dirty, clean):
        self._ensure_plan()
        have = getattr(self.engine.hip, "_recon_truth", None)
        if have is not None and have[0] is dirty and have[1] is clean:
            return
        n, index = self.n_rows, self.lw.pool.index
        d = np.full((len(self.columns), n), -4, dtype=np.int32)
        c = np.full((len(self.columns), n), -6, dtype=np.int32)
        counted = np.zeros(len(self.columns), dtype=bool)
        for i, col in enumerate(self.columns):
            if col in dirty and col in clean and i not in self._num:
                d[i], c[i] = truth_ids(index, dirty[col][:n], clean[col][:n])
                counted[i] = True
        self.engine.hip.recon_set_truth(d, c)
        if self._num:  # numeric columns are counted from numbers, NaN = a missing cell
            dn = np.full((len(self._num), n), np.nan)
            cn = np.full((len(self._num), n), np.nan)
            for k, i in enumerate(self._num):
                col = self.columns[i]
                if col in dirty and col in clean:
                    dn[k] = [np.nan if v is None else float(v) for v in dirty[col][:n]]
                    cn[k] = [np.nan if v is None else float(v) for v in clean[col][:n]]
                    counted[i] = True
            self.engine.hip.recon_set_truth_num(dn, cn)
        self.engine.hip._recon_truth = (dirty, clean, counted)

    def close(self):
        if self._ring is not None:
            self.engine.hip.ring_destroy(self._ring)
            self._ring = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- last sample --------------------------------------------------------------------------------------------------
    def reconstruct(self, trace):
        """{column: int32[n] pool ids} of `.columns`: analysis.reconstructed_pool_ids computed on the device, from the
        device-resident state when device commits are ahead of the host arrays (no pull), else after uploading what moved.
        A row without a referent in a column's block holds -1.  A numeric column (own=True) comes as the host gives it:
        ("numeric", float64[n]), bit for bit np.round(lowered.gauss_backward(...))."""
        if not self.columns:
            return {}
        self._current(trace)
        out = self.engine.hip.recon_run(len(self.columns), self.n_rows)
        got = {col: out[i] for i, col in enumerate(self.columns)}
        self._put_values(got, None)
        return got

    def _put_values(self, into, ring):
        if self._num:
            vals = self.engine.hip.recon_values(len(self._num), self.n_rows, ring)
            for k, i in enumerate(self._num):
                into[self.columns[i]] = ("numeric", vals[k])

    def _device_counts(self, ring=None, n_up_to=None):
        if n_up_to is None:
            per_col = self.engine.hip.recon_counts(len(self.columns), ring)
        else:
            per_col = self.engine.hip.recon_counts_up_to(len(self.columns), n_up_to, ring)
        return per_col[self.engine.hip._recon_truth[2]].sum(axis=0).astype(np.int64)

    def accuracy_counts(self, trace, dirty, clean):
        """analysis.accuracy_counts(lowered, trace, dirty, clean): `.columns` are reconstructed and counted on the device
        (dirty / clean ids are uploaded once per pair of tables), the remaining columns by the host code, and added.
        With own=True the host is left with the columns that are not queried and JuliaNodes without a function table:
        for a program without such nodes nothing reads the trace."""
        total = np.zeros(5, dtype=np.int64)
        if self.columns:
            self._current(trace)
            self._ensure_truth(dirty, clean)
            self.engine.hip.recon_run(len(self.columns), self.n_rows, fetch=False)
            total += self._device_counts()
        return total + analysis.accuracy_counts(self.lw, trace, dirty, clean, skip=set(self.columns))

    def accuracy_counts_up_to(self, trace, dirty, clean, n):
        """analysis.accuracy_counts_up_to(lowered, trace, dirty, clean, n): six counters, the same counter kernels with a
        row bound (`.columns` on the device, the rest on the host)."""
        n = max(0, min(int(n), self.n_rows))
        total = np.zeros(6, dtype=np.int64)
        if self.columns:
            self._current(trace)
            self._ensure_truth(dirty, clean)
            self.engine.hip.recon_run(len(self.columns), self.n_rows, fetch=False)
            total += self._device_counts(n_up_to=n)
        return total + analysis.accuracy_counts_up_to(self.lw, trace, dirty, clean, n, skip=set(self.columns))

    def accuracy_up_to(self, trace, dirty, clean, n):
        """analysis.evaluate_accuracy_up_to(lowered, trace, dirty, clean, n) with the device's counters"""
        return analysis.f1_from_counts_up_to(self.accuracy_counts_up_to(trace, dirty, clean, n))

    # -- kept samples -------------------------------------------------------------------------------------------------
    @property
    def n_kept(self):
        return min(self._adds, self.keep)

    def add(self, trace):
        """Keep the cleaned table of the trace's current state: the device columns are reconstructed straight into the
        ring's next slot, the host-only string columns are kept as host arrays."""
        self._current(trace)
        if self.columns:
            if self._ring is None:
                self._ring = self.engine.hip.ring_create(self.keep)
            self.engine.hip.ring_add(self._ring)
        if self.plan.host_strings:
            snap = analysis.reconstructed_pool_ids(self.lw, trace, columns=self.plan.host_strings)
            self._host_ring.append({c: np.asarray(v, dtype=np.int64) for c, v in snap.items()})
        self._adds += 1

    def _host_consensus(self):
        ids, support = {}, {}
        for col in self.plan.host_strings:
            ids[col], support[col] = mode_support(np.stack([snap[col] for snap in self._host_ring]))
        return ids, support

    def consensus(self):
        """(ids, support): per queried STRING column the most frequent pool id of every cell over the `n_kept` kept samples
        and the number of kept samples holding it; ties go to the value seen most recently.  Host-only string columns
        are tallied from host snapshots with the same rule.  Numeric queried columns are left out — unless the tally was
        made with own=True: then a numeric column comes as ("numeric", float64 values), the number under the Transformation
        option most of the kept samples hold (a mode of the discrete choice, not of real-valued draws), with that option's
        support."""
        if not self._adds:
            raise ValueError("nothing kept yet: CellTally.add first")
        self._refresh()
        ids, support = self._host_consensus()
        if self.columns:
            self._ensure_plan()
            mode, sup = self.engine.hip.ring_consensus(self._ring)
            for i, col in enumerate(self.columns):
                ids[col], support[col] = mode[i], sup[i]
            self._put_values(ids, self._ring)
        order = [c for c in self.lw.query.cleanmap if c in ids]
        return {c: ids[c] for c in order}, {c: support[c] for c in order}

    def consensus_accuracy(self, dirty, clean):
        """evaluate_accuracy of the consensus table, with the same counters (the device's for `.columns`).  Numeric queried
        columns are counted from their consensus values by a tally made with own=True; otherwise they are not tallied and
        stand at their dirty values (nothing changed, nothing imputed correctly)."""
        if not self._adds:
            raise ValueError("nothing kept yet: CellTally.add first")
        self._refresh()
        total = np.zeros(5, dtype=np.int64)
        if self.columns:
            self._ensure_truth(dirty, clean)
            self.engine.hip.ring_consensus(self._ring, fetch=False)
            total += self._device_counts(self._ring)
        ours = dict(self._host_consensus()[0])
        n = self.n_rows
        for col in self.plan.numeric:
            if col in dirty:
                ours[col] = ("numeric", np.array([np.nan if v is None else float(v) for v in dirty[col][:n]]))
        total += analysis.counts_given(self.lw, ours, n, dirty, clean, skip=set(self.columns))
        return analysis.f1_from_counts(total)
