"""Host driver of the HIP path: uploads a lowered model + trace and runs batched
rejuvenation sweeps of the observed class (pgibbs_sweep!'s loop over the rows of
the observed class, src/inference/inference.jl:60-81 + row_inference.jl:108-187).
"""
import os
import re

import numpy as np

from . import _lib
from ._lib import HipContext, InferConfig
from .encode import lm_log_tables
from .model import ChooseProportionally, ChooseUniformly, NumberCodePrior, StringPrior, TimePrior, Unmodeled, number_code

# time_prior.jl:10 — atoms matching this pattern score -log(1440), everything else -Inf
_TIME_RE = re.compile(r"^[0-9]?[0-9]:[0-9][0-9] [ap]\.m\.$")


def make_gauss(spec, mean_table_id=None):
    """pclean_gauss from a lowered Gaussian spec (model.LoweredModel.gauss / gauss_more); the block's g-th Gaussian
    observation reads mean table g."""
    if mean_table_id is None:
        mean_table_id = spec.get("mean_table", 0)
    g = _lib.Gauss()
    g.x_col, g.mean_table, g.n_dims = spec["x_col"], mean_table_id, len(spec["kinds"])
    for i, (kind, payload) in enumerate(spec["kinds"]):
        g.src_kind[i], g.src[i], g.stride[i] = _lib.GSRC[kind], int(payload), int(spec["strides"][i])
    g.n_locals = spec["n_locals"]
    for l in range(2):
        g.local_n[l] = spec["local_n"][l] if l < len(spec["local_n"]) else 1
        g.local_obs_col[l] = spec["local_obs"][l] if l < len(spec["local_obs"]) else -1
    kind, src = spec["transform"]  # ("none", -1): AddNoise, no Transformation to choose (option 0, the identity)
    g.transform_src_kind, g.transform_src = (-1, -1) if kind == "none" else (_lib.GSRC[kind], int(src))
    for u in range(4):
        g.t_scale[u] = spec["t_scale"][u] if u < len(spec["t_scale"]) else 1.0
        g.t_logabsderiv[u] = spec["t_lad"][u] if u < len(spec["t_lad"]) else 0.0
        g.t_x_col[u] = spec["t_x_col"][u] if u < len(spec.get("t_x_col", ())) else -1  # (non-linear units: derived columns)
        g.t_lad_col[u] = spec["t_lad_col"][u] if u < len(spec.get("t_lad_col", ())) else -1
    g.sigma = spec["sigma"]
    return g


def class_density_rows(rule, strings, options=None, counts=None):
    """T[value][class 0, 1, 2, missing observation] of a tabulated term, float64 [n][4] (pclean_set_class_density).
    ExpandOnShortVersion (expand_on_short_version.jl:30-41): -log(#options the value is a short version of) when it is
    a short version of the observed string, -1000 when not; missing: 0 if the value is one of the options (string
    membership), else -1000.  FormatName (format_name.jl:33-55): log(0.9999) / log(0.0001) / -1000 for equal / initial /
    neither, all -1000 for the empty name; missing: 0 for the empty name, -1000 for a name holding "*", else -5."""
    T = np.full((len(strings), 4), -1000.0)
    if rule == _lib.CLASS_SHORT_VERSION:
        opts = set(options)
        c = np.asarray(counts, dtype=np.float64)
        # (count 0: the value is a short version of no option, so of no observed string either — never looked up)
        T[:, 0] = np.where(c > 0, -np.log(np.maximum(c, 1.0)), -1000.0)
        T[:, 3] = [0.0 if s in opts else -1000.0 for s in strings]
    else:
        for v, s in enumerate(strings):
            if s != "":
                T[v, 0], T[v, 1] = np.log(0.9999), np.log(0.0001)
            T[v, 3] = 0.0 if s == "" else (-1000.0 if "*" in s else -5.0)
    return T


def number_code_logp(codes):
    """logdensity(NumberCodePrior(), code) = -log(code) of the observed code strings (number_code_prior.jl:10-14), float64"""
    vals = []
    for s in codes:
        v = number_code(s)
        if v is None:
            raise ValueError(f"NumberCodePrior: value {s!r} is not a decimal integer >= 1")
        vals.append(float(v))
    return -np.log(np.array(vals, dtype=np.float64))


def lw_locals(lw):
    return getattr(lw, "locals", {})


def _logsumexp(x):
    if len(x) == 0:  # (a key without atoms: all of the mass is its dummy's)
        return -np.inf
    m = np.max(x)
    if not np.isfinite(m):
        return m
    return m + np.log(np.sum(np.exp(x - m)))


class InferenceConfig:
    """src/inference/infer_config.jl:1-16 — same 7 fields, same defaults."""

    def __init__(self, num_iters, num_particles, use_dd_proposals=True, use_lo_sweeps=True,
                 use_mh_instead_of_pg=False, rejuv_frequency=50, reporting_frequency=100):
        if use_mh_instead_of_pg:
            num_particles = 2
        self.num_iters, self.num_particles = int(num_iters), int(num_particles)
        self.use_dd_proposals, self.use_lo_sweeps = bool(use_dd_proposals), bool(use_lo_sweeps)
        self.use_mh_instead_of_pg = bool(use_mh_instead_of_pg)
        self.rejuv_frequency, self.reporting_frequency = int(rejuv_frequency), int(reporting_frequency)

    def as_c(self):
        return InferConfig(self.num_iters, self.num_particles, int(self.use_dd_proposals), int(self.use_lo_sweeps),
                           int(self.use_mh_instead_of_pg), self.rejuv_frequency, self.reporting_frequency)


def option_prior(lw, trace, cname, aname):
    """log prior of every option of the ChooseProportionally choice cname.aname, in option order: logprobs() (utils.jl:33-36);
    an IndexedProportionsParameter: log theta_key[option], key-major as the options; a product leaf: the joint prior
    log pA(a) + log theta_a[b], added in that order; an arm of a star (LoweredModel.own_star): log theta_a[b] ALONE, key-major —
    log pA(a) belongs to the star's head"""
    m = lw.model
    d = m.classes[cname].attr(aname).dist
    with np.errstate(divide="ignore"):
        logp = np.log(trace.params[(cname, d.param)].value)
        ix = getattr(lw, "indexed", {}).get((cname, aname), ("", ""))
        if ix[0] == "product":
            da = m.classes[cname].attr(ix[1]).dist
            la = (np.log(trace.params[(cname, da.param)].value) if isinstance(da, ChooseProportionally)
                  else np.full(len(da.options), -np.log(len(da.options))))
            logp = la[:, None] + logp
        return logp.reshape(-1)


def own_gauss_prior(lw, trace, leaf):
    """log prior of every option of a Gaussian leaf (LoweredModel.own_gauss): log p(a) + log p(b) over the factors' grid,
    added in that order, key-major; one factor: that choice's own log prior (ChooseProportionally: logprobs() of its
    parameter; ChooseUniformly: -log(#options))"""
    cls = lw.query.cls
    parts = []
    for f in leaf["factors"]:
        d = lw.model.classes[cls].attr(f).dist
        parts.append(option_prior(lw, trace, cls, f) if isinstance(d, ChooseProportionally)
                     else np.full(len(d.options), -np.log(len(d.options))))
    return parts[0] if len(parts) == 1 else (parts[0][:, None] + parts[1][None, :]).reshape(-1)


class Engine:
    def __init__(self, lowered, obs, device=0, dist_mode=_lib.DIST_DL, row_offset=0):
        self.lw = lowered
        self.obs = np.ascontiguousarray(obs, dtype=np.int32)
        self.device, self.row_offset = device, row_offset
        self.hip = HipContext(device)
        self.dist_mode = dist_mode
        self.option_logp = {}
        self._uploaded_shape = {}
        self._last_upload = {}
        self._dc = None  # state of the device-resident commit (enable_device_commit)
        self.latent_dummy_keyed = False  # latent_dummy_served: keyed choices too (inference.latent_sweep turns it on)
        self.reloads = 0  # how often reload() replaced the context (what lives in a context, e.g. tally.CellTally's plan, follows)
        self._upload_static()
        if row_offset:
            _lib.check(self.hip.h, self.hip.lib.pclean_set_row_offset(self.hip.h, _lib.C.c_int64(row_offset)),
                       "pclean_set_row_offset")

    def _sync_ahead_trace(self):
        """A trace the device-resident commit left behind (Trace._dev is this engine) holds its only current copy in this
        engine's HBM: pull it before the context goes away (close / reload)."""
        ref = getattr(self, "_ahead", None)
        tr = ref() if ref is not None else None
        if tr is not None and getattr(tr, "_dev", None) is self:
            tr._sync()
        self._ahead = None
        ref = getattr(self, "_own_ahead", None)  # (the own choices of a flat class: sweep_own)
        tr = ref() if ref is not None else None
        if tr is not None and getattr(tr, "_own_dev", None) is self:
            tr._sync_own()
        self._own_ahead, self._own_key = None, None

    def close(self):
        self._sync_ahead_trace()
        self.hip.close()

    def reload(self):
        """The lowered model grew (LoweredModel.relower: strings drawn for chosen dummy values joined latent
        domains): a fresh context with the new string pool, pair / fn / option tables and plans.  Rare (a
        ProposalDummyValue is only ever chosen for unobserved or very short strings), so nothing is patched
        incrementally.  A device-side RCCL communicator bound with init_device_comm is re-bound to the new context —
        collectively: every rank reloads at the same point (the dummy draws are replicated)."""
        self._sync_ahead_trace()
        self.hip.close()
        self.hip = HipContext(self.device)
        self.option_logp = {}
        self._uploaded_shape = {}
        self._last_upload = {}
        self._upload_static()
        if self.row_offset:
            _lib.check(self.hip.h, self.hip.lib.pclean_set_row_offset(self.hip.h, _lib.C.c_int64(self.row_offset)),
                       "pclean_set_row_offset")
        self._dev_comm = False
        if getattr(self, "_comm", None) is not None:
            self.init_device_comm(self._comm)
        self._dc = None  # (a fresh context: the device-resident commit is set up again on demand)
        self.reloads += 1

    def sample_prior_strings(self, dist, n, seed, stream):
        """n draws of random(StringPrior) (string_prior.jl:28-40: length uniform on [min, max], bigram letters) or
        random(TimePrior) (time_prior.jl:21-23) by the device samplers, as strings; counter = (seed, stream, i)."""
        from . import sampling
        if isinstance(dist, TimePrior):
            return sampling.random_time_prior(self.hip, n, seed=seed, stream=stream)
        return sampling.random_string_prior(self.hip, n, dist.min_len, dist.max_len, seed=seed, stream=stream)

    def sample_prior_strings_at(self, dist, seeds, elems):
        """random(StringPrior) with the private streams the sweep used for the weights of the particles that chose the
        dummy (pclean_dummy_seed keys, global observed rows): the strings those particles' new rows hold."""
        from . import sampling
        if isinstance(dist, TimePrior):  # (the times a latent sweep with dummy_correction weighed: element = the latent row)
            return sampling.random_time_prior_at(self.hip, seeds, elems)
        return sampling.random_string_prior_at(self.hip, seeds, elems, dist.min_len, dist.max_len)

    # -- static data ----------------------------------------------------------
    def _upload_gauss(self):
        lw, hip = self.lw, self.hip
        for (bid, nid), spec in getattr(lw, "gauss", {}).items():
            hip.set_node_gauss(bid, nid, make_gauss(spec))
            for more in getattr(lw, "gauss_more", {}).get((bid, nid), ()):
                hip.add_node_gauss(bid, nid, make_gauss(more))

    def _upload_static(self):
        lw, hip = self.lw, self.hip
        sym, off, lm, _ = lw.pool.arrays()
        hip.load_strings(sym, off)
        from .encode import load_lm_params
        hip.set_lm_tables(*load_lm_params(), lw.pool.letter_symbols())
        hip.load_columns(self.obs)
        import time
        t0 = time.perf_counter()
        self.pair_cells = 0  # DP cells of the AddTypos pair tables: sum over tables of (sum of obs lengths) x (sum of latent lengths)
        self.pair_count = 0
        for key, (pid, odom, ldom) in lw.pair_id.items():
            oi, li = odom.id_array(), ldom.id_array()
            hip.build_pair_table(pid, oi, li, self.dist_mode)
            self.pair_cells += int(lw.pool.lens[oi].astype(np.int64).sum()) * int(lw.pool.lens[li].astype(np.int64).sum())
            self.pair_count += len(oi) * len(li)
        self.pair_build_s = time.perf_counter() - t0
        for fid, fn in lw.fn_tables.items():
            hip.set_fn_table(fid, fn)
        for key, (pid, n) in lw.eq_pairs.items():  # equality constraints: 0 on the diagonal, 1 elsewhere
            hip.set_pair_table(pid, (1 - np.eye(n, dtype=np.uint8)))
        for pid, (odom, vdom) in lw.same_pairs.items():  # MaybeSwap: 0 iff the observed string is the latent value
            hip.set_pair_table(pid, lw.same_pair_table(pid))
            hip.set_pair_strings(pid, odom.id_array(), vdom.id_array())  # (a drawn time is compared with the strings)
        hip.set_time_symbols([lw.pool.symbol_of(ch) for ch in "0123456789: ap.m"])
        self._upload_class_tables()
        if getattr(lw, "xnum", None) is not None and lw.xnum.shape[0]:
            hip.load_numeric_columns(lw.xnum)
        init_l, trans_l = lm_log_tables()
        m = lw.model
        for (cname, aname), dom in lw.latent_dom.items():
            d = m.classes[cname].attr(aname).dist
            tid = lw.option_id[(cname, aname)]
            if isinstance(d, TimePrior):
                # per key: its atoms' scores + that key's dummy mass (time_prior.jl:8-22)
                vals = lw.option_values[(cname, aname)]
                keys = lw.option_keycol[(cname, aname)]
                dummy = dom.get(d.dummy_value())
                scores = np.array([-np.log(1440.0) if _TIME_RE.match(dom.string(v)) else -np.inf for v in vals])
                logp = scores.copy()
                for k in np.unique(keys):
                    sel = (keys == k) & (vals != dummy)
                    with np.errstate(divide="ignore"):
                        logp[(keys == k) & (vals == dummy)] = np.log1p(-np.exp(_logsumexp(scores[sel])))
                self.option_logp[(cname, aname)] = logp
                hip.set_options_cols(tid, np.stack([vals, keys, lw.option_ncol[(cname, aname)]]), logp)
                continue
            if isinstance(d, NumberCodePrior):  # (never among the observed class's own choices: the lowering refuses that)
                logp = number_code_logp([dom.string(v) for v in range(len(dom))])
            elif d is None or isinstance(d, Unmodeled) or not isinstance(d, (StringPrior, ChooseUniformly, ChooseProportionally)):
                if cname == lw.query.cls:
                    continue  # own choices of the observed class are enumerated as locals, not as leaves
                logp = np.zeros(len(dom))  # Unmodeled: logdensity 0 (unmodeled.jl:7-10)
            elif isinstance(d, StringPrior) and d.keyed_by:
                # per key: scores of its atoms + that key's dummy mass (string_prior.jl:16-22)
                vals = lw.option_values[(cname, aname)]
                keys = lw.option_keycol[(cname, aname)]
                ids = dom.id_array()[vals]
                offs = np.zeros(len(ids) + 1, dtype=np.int64)
                np.cumsum(lw.pool.lens[ids], out=offs[1:])
                lmcat = np.concatenate([lm[off[i]:off[i + 1]] for i in ids])
                scores = hip.string_prior_scores(lmcat, offs, d.min_len, d.max_len, init_l, trans_l)
                logp = scores.copy()
                dummy = dom.get(d.dummy_value())
                for k in np.unique(keys):
                    sel = (keys == k) & (vals != dummy)
                    with np.errstate(divide="ignore"):
                        logp[(keys == k) & (vals == dummy)] = np.log1p(-np.exp(_logsumexp(scores[sel])))
                self.option_logp[(cname, aname)] = logp
                hip.set_options_cols(tid, np.stack([vals, keys]), logp)
                continue
            elif isinstance(d, StringPrior):
                # discrete_proposal(::StringPrior): atom scores + dummy mass (string_prior.jl:16-22)
                ids = dom.id_array()[:dom.n_base() - 1]  # the atoms (the dummy is the last value before any drawn string)
                offs = np.zeros(len(ids) + 1, dtype=np.int64)
                lens = lw.pool.lens[ids]
                np.cumsum(lens, out=offs[1:])
                lmcat = np.concatenate([lm[off[i]:off[i + 1]] for i in ids]) if len(ids) else np.zeros(0, np.uint8)
                scores = hip.string_prior_scores(lmcat, offs, d.min_len, d.max_len, init_l, trans_l)
                with np.errstate(divide="ignore"):
                    dummy = np.log1p(-np.exp(_logsumexp(scores)))
                logp = np.concatenate([scores, [dummy]])
            elif isinstance(d, ChooseUniformly):
                logp = np.full(len(dom), -np.log(len(d.options)))
            elif isinstance(d, ChooseProportionally):
                continue  # depends on the parameter value: uploaded with the trace
            else:
                raise NotImplementedError(type(d))
            self.option_logp[(cname, aname)] = logp
            hip.set_options(tid, lw.option_values[(cname, aname)], logp)
        lw.load_blocks_into(hip)
        self._gauss_pending = bool(getattr(lw, "gauss", {}))
        self._own_gauss_pending = bool(getattr(lw, "own_gauss", {}))  # (pclean_load_own_block forgot the terms)
        self._own_star_pending = bool(getattr(lw, "own_star", {}))  # (... and the stars: linked once the option tables are set)

    def _upload_class_tables(self):
        """Tabulated terms (ExpandOnShortVersion / FormatName): the class table of every such pair, built on the device
        (for FormatName(first, middle, last) the prefix and suffix tables), and its densities T[value][class 0..2, missing], evaluated here once in float64 (class_density_rows)."""
        lw, hip = self.lw, self.hip
        if not getattr(lw, "class_pairs", None):
            return
        hip.set_fold_table(lw.pool.fold_symbols())
        for pid, (rule, odom, ldom, options) in lw.class_pairs.items():
            li = ldom.id_array()
            if rule in (_lib.CLASS_NAME_PREFIX, _lib.CLASS_NAME_SUFFIX):
                # the two byte tables of a three-name FormatName: the separator is the space; no class densities (the
                # term's two constants travel with set_term_name3, LoweredModel.load_blocks_into)
                hip.build_class_table(pid, odom.id_array(), li, rule, lw.pool.symbol_of(" "))
                continue
            hip.build_class_table(pid, odom.id_array(), li, rule, lw.pool.symbol_of("."))
            strings = [ldom.string(v) for v in range(len(ldom))]
            counts = None
            if options is not None:
                counts = hip.count_short_versions(lw.pool.add_all(options), li)
            hip.set_class_density(pid, class_density_rows(rule, strings, options, counts))

    # -- dynamic data ---------------------------------------------------------
    def upload_trace(self, trace):
        """Latent tables, parameter-dependent option priors and parameter tables of `trace` -> device.  Whatever is
        byte-identical to the last upload is skipped: besides the copies that keeps the device-side versions — and
        with them the per-value caches of option-list marginals and the compact byte tables — valid (between two
        observed-class sweeps of one rejuvenation period only the root tables' counts move)."""
        lw, hip = self.lw, self.hip
        m = lw.model
        last = self._last_upload
        dc = getattr(self, "_dc", None)
        dbg = os.environ.get("PCLEAN_DEBUG_UPLOAD")  # diagnostic: uploads of a table that take more than a millisecond
        t_dbg = None
        for cname, t in trace.tables.items():
            if dbg:
                t_dbg = self._debug_upload(t_dbg, cname)
            cols, counts = t.view()
            cap = t.n
            in_dc = dc is not None and cname in dc["tables"]
            if in_dc:
                # device-resident commit: the table is uploaded with spare rows (count 0: dead candidates, weight exactly 0)
                # so that the device can create rows without changing any array's shape
                cap = dc["cap"].get(cname, 0)
                grown = max(0, t.n - dc["alloc"].get(cname, (t.n, 0))[0])  # what the host added to the high-water mark
                dc["created"][cname] = max(grown, dc["created"].get(cname, 0))
                if t.n + self._slack_min(cname, t) > cap:
                    cap = dc["cap"][cname] = self._capacity(cname, t)
            key = (cname, cap)
            prev = last.get(("table", cname))
            alloc = (t.n, len(t.free))
            need_cols = t.cols_dirty or self._uploaded_shape.get(cname) != key
            # (the comparison comes before any padding: most tables of most sub-batches have not moved)
            if not need_cols and prev is not None and prev[1] == (t.strength, t.discount) and len(prev[0]) >= t.n \
                    and np.array_equal(prev[0][:t.n], counts) and not prev[0][t.n:].any() \
                    and (not in_dc or dc["alloc"].get(cname) == alloc):
                continue  # nothing moved in this table
            if in_dc and cap > t.n:
                pk = np.zeros(cap, dtype=np.int64)
                pk[:t.n] = counts
                counts = pk
                if need_cols:
                    pc = np.zeros((t.n_cols, cap), dtype=np.int32)
                    pc[:, :t.n] = cols
                    cols = pc
            if need_cols:
                hip.set_table(lw.table_id[cname], np.ascontiguousarray(cols), counts, t.strength, t.discount)
                t.cols_dirty = False
                self._uploaded_shape[cname] = key
            else:  # only reference counts moved: keep the device columns and their compact byte tables
                hip.set_table(lw.table_id[cname], None, counts, t.strength, t.discount, n_cols=t.n_cols)
            last[("table", cname)] = (counts.copy(), (t.strength, t.discount))
            if in_dc:
                hip.commit_set_table_state(lw.table_id[cname], t.n, t.free)
                dc["alloc"][cname] = alloc
        if dbg:
            self._debug_upload(t_dbg, None)
        for (cname, aname), dom in lw.latent_dom.items():
            d = m.classes[cname].attr(aname).dist
            if isinstance(d, ChooseProportionally):
                logp = option_prior(lw, trace, cname, aname)
                self.option_logp[(cname, aname)] = logp
                prev = last.get(("options", cname, aname))
                if prev is not None and np.array_equal(prev, logp):
                    continue
                if (cname, aname) in getattr(lw, "option_cols", {}):
                    hip.set_options_cols(lw.option_id[(cname, aname)], lw.option_cols[(cname, aname)], logp)
                elif (cname, aname) in getattr(lw, "indexed", {}):
                    hip.set_options_cols(lw.option_id[(cname, aname)], np.stack([lw.option_values[(cname, aname)],
                                                                                 lw.option_keycol[(cname, aname)]]), logp)
                else:
                    hip.set_options(lw.option_id[(cname, aname)], lw.option_values[(cname, aname)], logp)
                last[("options", cname, aname)] = logp.copy()
        if getattr(self, "_own_star_pending", False):  # after pclean_load_own_block and the nodes' option tables
            for (bi, head), arms in lw.own_star.items():
                hip.link_own_star(bi, head, arms)
            self._own_star_pending = False
        if lw.prob_spec is not None:
            pt = trace.prob_table()
            if last.get("prob") is None or not np.array_equal(last["prob"], pt):
                hip.set_prob_table(pt)
                last["prob"] = pt.copy()
        if getattr(lw, "gauss", None) or getattr(lw, "own_gauss", None):
            for g, mp in enumerate(trace.mean_params):  # term g reads mean table g
                mv, key = mp.value, "mean" if g == 0 else ("mean", g)
                if last.get(key) is None or not np.array_equal(last[key], mv):
                    hip.set_mean_table(g, mv)
                    last[key] = mv.copy()
            if self._gauss_pending:  # needs the mean table to exist
                self._upload_gauss()
                self._gauss_pending = False
        for (bi, nid), leaf in getattr(lw, "own_gauss", {}).items():
            # a Gaussian leaf of a flat class: the joint prior over the factors' grid, on the leaf's own option table
            logp = own_gauss_prior(lw, trace, leaf)
            prev = last.get(("own_gauss", bi, nid))
            if prev is None or not np.array_equal(prev, logp):
                hip.set_options_cols(leaf["table"], leaf["cols"], logp)
                last[("own_gauss", bi, nid)] = logp.copy()
        if getattr(self, "_own_gauss_pending", False):  # after pclean_load_own_block, the option tables and the numeric columns
            for (bi, nid), leaf in lw.own_gauss.items():
                for spec in leaf["specs"]:
                    hip.add_own_gauss(bi, nid, make_gauss(spec))
            self._own_gauss_pending = False

    @staticmethod
    def _debug_upload(prev, cname):
        """PCLEAN_DEBUG_UPLOAD: prints the table whose upload just ended when it took more than a millisecond"""
        import time
        now = time.perf_counter()
        if prev is not None and now - prev[1] > 1e-3:
            print(f"[upload] {prev[0]}: {1e3 * (now - prev[1]):.1f} ms", flush=True)
        return (cname, now)

    def _upload_cur_locals(self, trace, cfg):
        """prior proposals (use_dd_proposals = false) of a class with own enumerated choices: the retained particle keeps the
        row's current ones (block_proposal.jl:42-56) — the data-driven proposal enumerates them and needs none"""
        if cfg.use_dd_proposals or not self.lw.locals:
            return
        loc = trace._locals  # (host-owned even while the device is ahead of the trace: sweep_commit_device keeps it current)
        for bi in self.lw.locals:
            self.hip.set_cur_locals(bi, loc[bi])

    def _refuse_prior_product(self, cfg, who, infos):
        """use_dd_proposals = false on a plan holding a product leaf: the prior proposal would have to sample the index and
        then the choice from theta[index]; the option table holds their joint prior only.  Refused HERE, by the Python
        driver: the C ABI has no mark for such a leaf"""
        if not cfg.use_dd_proposals and any("product" in info for info in infos):
            raise _lib.PCleanHipError(f"{who}: a product leaf (an indexed ChooseProportionally enumerated jointly with its "
                                      "index) under use_dd_proposals = false (prior proposals) is not supported")

    def sweep(self, trace, config, seed, sweep_idx, lo=0, hi=None, reuse_buffers=False, light=False):
        """One batched sweep over the observed rows [lo, hi) of the trace (default: all of them).
        Returns (choice, chosen_particle, logml, new_rows), all indexed relative to lo.  reuse_buffers:
        trace.cur is passed in place (page-locked once) and the results are views of page-locked buffers
        that the next sweep overwrites (callers that commit the result right away: inference.py, bench.py).
        light: no per-row outputs are copied back (choice / chosen / logml are None); the commit reads the
        moved rows (sweep_moved) and the new-row records only."""
        cfg = config.as_c() if isinstance(config, InferenceConfig) else config
        self._refuse_prior_product(cfg, "Engine.sweep", [i for blk in self.lw.blocks for i in blk["node_info"]])
        hi = trace.cur.shape[1] if hi is None else hi
        if hi <= lo:  # a rank may own no row of a small batch
            for bi in self.lw.locals:
                trace.pending_locals[bi] = np.zeros((0, 2), dtype=np.int32)
            self._empty_sweep = True
            nb = trace.cur.shape[0]
            return (None if light else np.zeros((nb, 0), np.int32)), np.zeros(0, np.int32), np.zeros(0), {}
        self._empty_sweep = False
        self.hip.set_active_rows(lo, hi - lo)
        self._upload_cur_locals(trace, cfg)
        if reuse_buffers and trace.cur.dtype == np.int32 and trace.cur.flags.c_contiguous:
            choice, chosen, logml = self.hip.sweep(cfg, seed, sweep_idx, trace.cur, True, window=(lo, hi), light=light)
        else:
            choice, chosen, logml = self.hip.sweep(cfg, seed, sweep_idx, trace.cur[:, lo:hi], reuse_buffers, light=light)
        new_rows = {}
        for bi, blk in enumerate(self.lw.blocks):
            if blk.get("score"):
                continue
            rows, vals = self.hip.get_new_rows(bi, len(blk["nodes"]))
            if len(rows):
                new_rows[bi] = (rows, vals)
        if self.lw.locals:
            for bi in self.lw.locals:
                trace.pending_locals[bi] = self.hip.get_locals(bi, hi - lo)
        return choice, chosen, logml, new_rows

    # -- a flat observed class: own blocks (csrc/own_block.hip) -----------------------------------------------------
    def _own_blocks(self, trace):
        """[(block, first row of trace.own, one past its last)] of the own blocks: the CHOICES of a block as rows of
        Trace.own.  In a block without a product leaf these are its device leaves too; with one, the device holds one leaf
        for the pair (_own_device_blocks, which _push_own / pull_own go by)"""
        out = []
        for li, (_, b, _) in enumerate(trace.own_leaves()):
            if out and out[-1][0] == b:
                out[-1][2] = li + 1
            else:
                out.append([b, li, li + 1])
        return out

    def _own_device_blocks(self, trace):
        """[(block, [rows of trace.own per device leaf of the block, in node order])] of the own blocks: one row, or (index's
        row, choice's row) of a product leaf"""
        out = []
        for b, _, rows in trace.own_device_leaves():
            if out and out[-1][0] == b:
                out[-1][1].append(rows)
            else:
                out.append((b, [rows]))
        return out

    def _push_own(self, trace):
        """the trace's own choices -> device, unless the device holds them already (they live there between sweeps); the two
        choices of a product leaf go as the joint option index * |B| + choice"""
        key = (id(trace), trace._own_version, id(self.hip))
        if getattr(trace, "_own_dev", None) is self or getattr(self, "_own_key", None) == key:
            return
        for b, leaves in self._own_device_blocks(trace):
            self.hip.set_own(b, np.stack([trace._own[r[0]] if len(r) == 1 else trace.own_joint(trace._own, *r) for r in leaves]))
        self._own_key = key

    def pull_own(self, trace):
        """device -> trace._own (Trace.own calls it when the device is ahead)"""
        for b, leaves in self._own_device_blocks(trace):
            vals = self.hip.get_own(b, len(leaves), trace._own.shape[1])
            for v, r in zip(vals, leaves):
                if len(r) == 1:
                    trace._own[r[0]] = v
                else:
                    trace._own[r[0]], trace._own[r[1]] = trace.own_split(v, r[1])
        self._own_key = (id(trace), trace._own_version, id(self.hip))

    def sweep_own(self, trace, config, seed, sweep_idx, lo=0, hi=None, want_outputs=True):
        """One batched sweep of a FLAT observed class over its rows [lo, hi) (default: all): pclean_sweep_own.  The option
        priors are re-uploaded whenever their parameter moved (upload_trace), the own choices are updated in place on the
        device (Trace.own pulls them on access) and the Dirichlet counts follow from a device histogram.  Returns (chosen
        particle, logml) of the window's rows, or (None, None) without want_outputs."""
        import weakref
        if not getattr(self.lw, "flat", False):
            raise _lib.PCleanHipError("Engine.sweep_own: the observed class is not flat (it has reference-slot blocks)")
        cfg = config.as_c() if isinstance(config, InferenceConfig) else config
        if not cfg.use_dd_proposals:
            raise NotImplementedError("use_dd_proposals=False (prior proposals) is not served for a flat observed class")
        if getattr(self.lw, "own_star", None) and getattr(self, "_dev_comm", False):
            raise NotImplementedError("several ranks (init_device_comm): a star of own choices is served on one rank alone")
        hi = trace._own.shape[1] if hi is None else hi
        if hi <= lo:
            return (np.zeros(0, np.int32), np.zeros(0)) if want_outputs else (None, None)
        self.upload_trace(trace)
        self._push_own(trace)
        self.hip.set_active_rows(lo, hi - lo)
        chosen, logml = self.hip.sweep_own(cfg, seed, sweep_idx, hi - lo, want_outputs)
        trace._own_dev = self
        self._own_ahead = weakref.ref(trace)  # (close / reload pull the values first)
        st = self.hip.get_own_stats()
        if st.impossible_rows:
            raise ValueError(f"row {st.first_impossible_row + self.row_offset}: none of the options of an own choice is possible "
                             f"given the row's observations ({st.impossible_rows} such rows in [{lo}, {hi})); the reference "
                             "fails on such a row too")
        trace.refresh_own_counts()
        return chosen, logml

    def own_marginals(self, trace, top=1, lo=0, hi=None):
        """Exact conditionals of the own choices of a FLAT observed class over its rows [lo, hi) (default: all), given the
        parameters as they stand: pclean_own_marginals once per leaf.  Returns {own choice: (options int32 [top][n], their
        probabilities float64 [top][n], probability of the row's current value float64 [n])}, the options ordered by
        probability (ties: the smaller option index), -1 / 0.0 where fewer options are possible.  The option priors are
        re-uploaded whenever their parameter moved (upload_trace) and the own choices are pushed unless the device holds
        them; nothing is drawn, written or pulled, and no count changes.  A choice indexed by a sibling choice and that
        index (one product leaf): the top options are those of the PAIR — entry t of both is the t-th most probable pair,
        decoded per choice — and every probability is the pair's JOINT probability, not a per-column marginal; the probability
        of the current value is that of the current pair.  The choices of a STAR (own_star=True) each have an entry of their
        own: the index's is its exact marginal u_a / U; a dependent's is CONDITIONAL on the index's first value a* — the top b
        with P(b | a*, obs) and that probability of the row's current b — neither a per-column marginal nor the joint."""
        if not getattr(self.lw, "flat", False):
            raise _lib.PCleanHipError("Engine.own_marginals: the observed class is not flat (it has reference-slot blocks)")
        hi = trace._own.shape[1] if hi is None else hi
        n = max(hi - lo, 0)
        if n == 0:
            return {a: (np.full((top, 0), -1, np.int32), np.zeros((top, 0)), np.zeros(0)) for a, _, _ in trace.own_leaves()}
        self.upload_trace(trace)
        self._push_own(trace)
        self.hip.set_active_rows(lo, n)
        names, out = trace.own_leaves(), {}
        for b, nd, rows in trace.own_device_leaves():
            opt, prob, cur = self.hip.own_marginals(b, nd, top, n)
            if len(rows) == 1:
                out[names[rows[0]][0]] = (opt, prob, cur)
                continue
            # a product leaf: the joint top options, decoded into an entry per choice; both carry the JOINT probability
            oa, ob = trace.own_split(opt, rows[1])
            out[names[rows[0]][0]], out[names[rows[1]][0]] = (oa, prob, cur), (ob, prob.copy(), cur.copy())
        return out

    # -- device-resident commit (csrc/commit.hip) ------------------------------------------------------------------
    def _slack_min(self, cname, t):
        """spare rows a table needs before the next device commit: a few times what the last commits added to its
        high-water mark (rows re-created from the free list need no room).  Dead candidates cost every enumeration —
        a one-row table padded to hundreds of rows would make its reference slots hundreds of times dearer — so the
        margin stays proportional to the table"""
        dc = self._dc
        if os.environ.get("PCLEAN_DC_NOPAD"):
            return 0
        return max(8, 4 * dc["created"].get(cname, 0) + 8)

    def _capacity(self, cname, t):
        if os.environ.get("PCLEAN_DC_NOPAD"):  # diagnostic: no spare rows (every growth is a refused commit)
            return t.n
        slack = max(16, t.n // 16, 2 * self._slack_min(cname, t))
        return -(-(t.n + slack) // 16) * 16

    def enable_device_commit(self, trace, comm=None):
        """Switch the engine to the device-resident commit of observed-class sweeps (pclean_commit_*): latent tables
        are uploaded with spare capacity, their allocation state and the observed rows' referents live in HBM and
        sweep_commit_device() commits a sweep without any per-row read-back.  Returns False (and changes nothing) when
        the plan / the run is one the device commit does not take: several ranks (the new-row records of the other
        ranks are exchanged through the host), or a plan shape pclean_commit_enable refuses."""
        if getattr(self, "_dc", None) is not None:
            return True
        if getattr(self, "_dc_refused", False):
            return False
        self._dc_dist = False
        if comm is not None and (comm.world > 1 or (getattr(self, "_dev_comm", False) and os.environ.get("PCLEAN_FORCE_DIST"))):
            # several ranks: every rank's moved rows and new-row records are all-gathered on the device and the same commit
            # kernel runs everywhere (pclean_commit_device_dist) — needs the library's own RCCL communicator
            if not getattr(self, "_dev_comm", False) or os.environ.get("PCLEAN_DIST_HOST_COMMIT"):
                self._dc_refused = True
                return False
            self._dc_dist = True
        if self.row_offset:
            self._dc_refused = True
            return False
        lw = self.lw
        self.upload_trace(trace)  # (the library checks the blocks' tables exist)
        ok, why = self.hip.commit_enable(len(lw.blocks))
        if not ok:
            self._dc_refused, self._dc_why = True, why
            return False
        by_id = {tid: c for c, tid in lw.table_id.items()}
        self._dc = dict(tables=[by_id[t] for t in self.hip.commit_tables()], cap={}, alloc={}, created={}, cur_version=None,
                        commits=0, fallbacks=0)
        for cname in self._dc["tables"]:  # re-upload with capacity
            self._uploaded_shape.pop(cname, None)
        self.upload_trace(trace)
        return True

    def prepare(self, trace, comm=None):
        """One-time set-up before the first run_inference iteration: the device-resident commit (tables uploaded with their
        spare capacity from the start, so that no table changes shape later) and every compact table / per-value cache the
        sweeps of all classes will ask for (pclean_prepare).  Optional: results do not depend on it."""
        from . import inference as inf
        if getattr(self.lw, "flat", False):  # (no latent table, no reference slot: nothing to prepare or to commit)
            self.upload_trace(trace)
            self._prepared = True
            return
        if inf.DEVICE_COMMIT:
            self.enable_device_commit(trace, comm)
        self.upload_trace(trace)
        ev = 0
        for pl in self.lw.latent_plans.values():
            ev |= 1 << int(pl["block_id"])
        self.hip.prepare(ev)
        self._prepared = True

    def _sync_cur(self, trace):
        dc = self._dc
        if dc["cur_version"] != (id(trace), trace._cur_version):
            self.hip.set_cur(trace._cur)
            dc["cur_version"] = (id(trace), trace._cur_version)

    def sweep_commit_device(self, trace, config, seed, sweep_idx, lo=0, hi=None, comm=None, window=None):
        """One batched sweep of the observed rows [lo, hi) against the device-resident tables AND its commit on the
        device: ONE stream synchronisation, a summary comes back.  Returns the number of rows whose referent changed,
        or None when the device refused the commit (nothing was modified; the sweep's outputs are on the host as after
        a plain sweep(..., light=True): the caller commits on the host).  The host arrays of `trace` are left alone:
        the trace is marked as behind the device and pulls the state when something reads it (Trace._sync)."""
        dc = self._dc
        cfg = config.as_c() if isinstance(config, InferenceConfig) else config
        self._refuse_prior_product(cfg, "Engine.sweep_commit_device", [i for blk in self.lw.blocks for i in blk["node_info"]])
        hi = trace._cur.shape[1] if hi is None else hi
        if trace._dev is None:  # the host arrays are current: the device gets whatever moved since the last upload
            self.upload_trace(trace)
            self._sync_cur(trace)
        elif trace._dev is not self:
            raise _lib.PCleanHipError("the trace is ahead on another engine")
        dist = getattr(self, "_dc_dist", False)
        local_empty = hi <= lo  # (several ranks: a rank may own no row of a small window; it still takes part in the exchange)
        self._empty_sweep = local_empty
        self.hip.set_sweep_mode(True)
        try:
            if not local_empty:
                self.hip.set_active_rows(lo, hi - lo)
                self._upload_cur_locals(trace, cfg)
                self.hip.sweep_device_cur(cfg, seed, sweep_idx, len(self.lw.blocks))
            if dist:
                world = comm.world if comm is not None else 1
                b0, b1 = window if window is not None else (lo, hi)
                summ = self.hip.commit_device_dist(len(self.lw.blocks), sweep_idx, local_empty, -(-(b1 - b0) // world))
            else:
                summ = self.hip.commit_device(len(self.lw.blocks), sweep_idx)
        finally:
            self.hip.set_sweep_mode(False)
        dc["commits"] += 1
        by_id = {tid: c for c, tid in self.lw.table_id.items()}
        if summ.fallback:
            dc["fallbacks"] += 1
            dc["last_fallback"] = int(summ.fallback)
            if not local_empty:
                self.hip.sweep_fetch()
            # (several ranks: the delta reference counts in the device buffers are already summed over the ranks)
            self._stats_reduced_on_device = bool(summ.stats_reduced)
            return None  # (a table about to outgrow its capacity gets more room at the next upload: upload_trace)
        if os.environ.get("PCLEAN_DEBUG_COMMIT"):
            print("[pclean] device commit: changed", summ.n_changed, "records", list(summ.n_records[:len(self.lw.blocks)]),
                  "distinct", list(summ.n_distinct[:len(self.lw.blocks)]),
                  {by_id[summ.slot[i].table_id]: (summ.slot[i].n_hw, summ.slot[i].n_free, summ.slot[i].created, summ.slot[i].deleted,
                                                  summ.slot[i].cols_changed) for i in range(summ.n_slots)}, flush=True)
        for si in range(summ.n_slots):
            sl = summ.slot[si]
            c = by_id[sl.table_id]
            grown = max(0, int(sl.n_hw) - dc["alloc"].get(c, (int(sl.n_hw), 0))[0])  # rows the high-water mark moved
            dc["created"][c] = max(grown, dc["created"].get(c, 0) // 2)
            dc["alloc"][c] = (int(sl.n_hw), int(sl.n_free))
        for bi in lw_locals(self.lw):  # own enumerated choices of the chosen particles: host-owned (parameter moves read them)
            loc = self.hip.get_locals(bi, hi - lo) if not local_empty else np.zeros((0, 2), dtype=np.int32)
            if dist and comm is not None and comm.world > 1:  # every rank learns all of them (rank order = row order)
                b0 = window[0] if window is not None else lo
                loc = comm.allgather_varlen_i32(np.ascontiguousarray(loc, dtype=np.int32)).reshape(-1, 2)
                trace._locals[bi][b0:b0 + len(loc)] = loc
            else:
                trace._locals[bi][lo:hi] = loc
        trace._dev = self
        import weakref
        self._ahead = weakref.ref(trace)  # (close / reload pull it first: the committed sweeps exist nowhere else)
        return int(summ.n_changed)

    def fetched_new_rows(self, trace, lo, hi):
        """new-row records of the last sweep once its outputs are on the host (a refused device commit: pclean_sweep_fetch
        ran) — what sweep(..., light=True) returns as new_rows; own enumerated choices go to trace.pending_locals"""
        new_rows = {}
        if getattr(self, "_empty_sweep", False):  # (several ranks: this rank swept no row of the window)
            for bi in lw_locals(self.lw):
                trace.pending_locals[bi] = np.zeros((0, 2), dtype=np.int32)
            return new_rows
        for bi, blk in enumerate(self.lw.blocks):
            if blk.get("score"):
                continue
            rows, vals = self.hip.get_new_rows(bi, len(blk["nodes"]))
            if len(rows):
                new_rows[bi] = (rows, vals)
        for bi in lw_locals(self.lw):
            trace.pending_locals[bi] = self.hip.get_locals(bi, hi - lo)
        return new_rows

    def pull(self, trace):
        """Device-resident state -> host arrays of `trace` (called through Trace._sync when something reads a trace that
        device commits left behind): latent tables with their allocation state, the observed rows' referents, the
        Dirichlet counts of own choices (recomputed from the tables), the origins of created rows."""
        lw, dc = self.lw, self._dc
        if dc is None or not self.hip.h:
            raise _lib.PCleanHipError("the trace is behind a device-resident commit whose context is gone (Engine.close / "
                                      "reload without a pull): its committed sweeps are lost")
        for cname in dc["tables"]:
            t = trace._tables[cname]
            state, cols, counts, live, free, origin = self.hip.commit_pull_table(lw.table_id[cname])
            n = int(state[0])
            if t.cols.shape[1] < n:
                grow = max(n, 2 * t.cols.shape[1]) - t.cols.shape[1]
                t.cols = np.concatenate([t.cols, np.zeros((t.n_cols, grow), np.int32)], axis=1)
                t.counts = np.concatenate([t.counts, np.zeros(grow, np.int64)])
                t.live = np.concatenate([t.live, np.zeros(grow, bool)])
            t.cols[:, :n] = cols[:, :n]
            t.counts[:n] = counts[:n]
            t.counts[n:] = 0
            t.live[:n] = live[:n]
            t.live[n:] = False
            t.n = n
            t.free = [int(r) for r in free]
            t.cols_dirty = False
            for r in np.flatnonzero(origin[:, 0]):
                mark = int(origin[r, 0])
                if mark > 0:
                    trace._row_origin[(cname, int(r))] = (int(origin[r, 1]), int(origin[r, 2]), int(origin[r, 3]), mark - 1)
                else:
                    trace._row_origin.pop((cname, int(r)), None)
            cap = dc["cap"].get(cname, n)
            pk = np.zeros(max(cap, n), dtype=np.int64)
            pk[:n] = counts[:n]
            self._last_upload[("table", cname)] = (pk if cap > n else pk[:n].copy(), (t.strength, t.discount))
            dc["alloc"][cname] = (n, len(t.free))
        if trace._cur.flags.c_contiguous and trace._cur.dtype == np.int32:
            self.hip.get_cur(trace._cur.shape[0], trace._cur.shape[1], out=trace._cur)  # in place (the array may be page-locked)
        else:
            trace._cur[...] = self.hip.get_cur(*trace._cur.shape)
        dc["cur_version"] = (id(trace), trace._cur_version)
        for (cname, pname), state in trace._params.items():  # own-choice sufficient statistics (check_consistency's identity)
            for a in lw.model.classes[cname].attrs:
                if a.kind == "choice" and isinstance(a.dist, ChooseProportionally) and a.dist.param == pname:
                    state.counts = trace.recount(cname, a.name)

    def make_device_current(self, trace):
        """The latent tables and the observed rows' referents of `trace` as the device holds them are its current state
        afterwards: nothing to do while device commits are ahead of the host arrays (no pull), else whatever moved since
        the last upload goes up (upload_trace / set_cur) — what a kernel reading the device-resident state needs
        (tally.CellTally)."""
        if trace._dev is self:
            return
        if trace._dev is not None:
            raise _lib.PCleanHipError("the trace is ahead on another engine")
        self.upload_trace(trace)
        if self._dc is not None:
            self._sync_cur(trace)
        else:
            self.hip.set_cur(trace._cur)

    def sweep_moved(self):
        """{block: (rows relative to the swept window, new referent)} of the last sweep, rows ascending."""
        if getattr(self, "_empty_sweep", False):
            return {bi: (np.zeros(0, np.int32), np.zeros(0, np.int32))
                    for bi, blk in enumerate(self.lw.blocks) if not blk.get("score")}
        return {bi: self.hip.get_moved(bi) for bi, blk in enumerate(self.lw.blocks) if not blk.get("score")}

    def latent_dummy_served(self, cname):
        """Attributes of latent class cname whose chosen ProposalDummyValues a latent sweep with dummy_correction=True
        weighs (pclean_set_latent_dummy_correction): the class's own choices (leaf roots of its plan) with
          * a StringPrior, keyed or not, whose evidence terms are all plain AddTypos terms (no JuliaNode context, not
            tabulated), or
          * a TimePrior whose evidence terms are all MaybeSwap terms (the error probability looked up per evidence row),
        one or two such terms, no Gaussian term on the node; a keyed choice carries the equality term of its directly
        observed key besides.  Everything else — reference slots among it — is swept as with the flag off.
        KEYED choices (every TimePrior is one) are served only while `latent_dummy_keyed` is on: serving them takes the
        per-row dummy options (latent_dummy_options) and an `excl` that goes by the row's key, which inference.latent_sweep
        and run_inference supply — they turn the switch on — and a caller of the bare sweep_latent written before keyed
        choices were served does not: with the switch off (the default) such a caller gets the answers and the sweeps it
        always got."""
        lw = self.lw
        keyed_on = bool(getattr(self, "latent_dummy_keyed", False))
        pl = lw.latent_plans.get(cname)
        if pl is None:
            return []
        out = []
        for r, root in enumerate(pl["roots"]):
            node = pl["nodes"][root]
            if node[0] != _lib.NODE_LEAF:
                continue
            attr = pl["root_attr"][r]
            if isinstance(attr, tuple):  # a product leaf: neither choice has a dummy
                continue
            d = lw.model.classes[cname].attr(attr).dist
            if not isinstance(d, (StringPrior, TimePrior)):
                continue
            terms = pl["terms"][node[2]:node[2] + node[3]]
            if getattr(d, "keyed_by", None):
                if not keyed_on:
                    continue
                key_terms = [t for t in terms if t[3] == _lib.DENS_EQUAL and t[1] == 1 and t[5] < 0]
                if len(key_terms) != 1:
                    continue
                terms = [t for t in terms if t is not key_terms[0]]
            if not 1 <= len(terms) <= 2 or (pl["block_id"], root) in getattr(lw, "gauss", {}):
                continue
            if isinstance(d, TimePrior):
                if all(t[3] == _lib.DENS_MAYBE_SWAP and t[5] >= 0 and t[7] == 1 and t[1] == 0 and t[2] in lw.same_pairs
                       for t in terms):
                    out.append(attr)
                continue
            typo_pairs = {pid for pid, _, _ in lw.pair_id.values()}  # (AddTypos tables: built on the device from the strings)
            if all(t[3] == _lib.DENS_ADD_TYPOS and t[5] < 0 and t[1] == 0 and t[2] in typo_pairs for t in terms):
                out.append(attr)
        return out

    def latent_dummy_options(self, trace, cname, rows):
        """pclean_set_latent_dummy_options for latent rows `rows` of class cname: per root of the class's plan the index of
        the dummy option of the row's key in the root's option table — the served keyed choices (latent_dummy_served); -1
        everywhere else and for a key without options.  None when the class serves no keyed choice."""
        lw = self.lw
        pl = lw.latent_plans[cname]
        served = self.latent_dummy_served(cname)
        t = trace.tables[cname]
        out = None
        for r, attr in enumerate(pl["root_attr"]):
            d = lw.model.classes[cname].attr(attr).dist if attr in served else None
            if d is None or not getattr(d, "keyed_by", None):
                continue
            if out is None:
                out = np.full((len(pl["roots"]), len(rows)), -1, dtype=np.int32)
            vals, keys = lw.option_values[(cname, attr)], lw.option_keycol[(cname, attr)]
            dummy = lw.latent_dom[(cname, attr)].get(d.dummy_value())
            rowkey = t.cols[lw.colidx[cname][d.keyed_by], rows]
            lut = np.full(max(int(keys.max()), int(rowkey.max()) if len(rowkey) else 0) + 1, -1, dtype=np.int32)
            at = np.flatnonzero(vals == dummy)
            lut[keys[at]] = at
            out[r] = lut[rowkey]
        return out

    def sweep_latent(self, trace, cname, config, seed, sweep_idx, live, ev_off, ev_rows, ev_ctx, excl, ev_begin=None,
                     dummy_correction=False):
        """Rejuvenation of the latent rows `live` of class cname against their evidence sets
        (pclean_sweep_latent).  Returns (chosen particle, sampled node values) per latent row.  ev_begin (with ev_rows
        None): the rows' evidence starts at that position of the evidence build_evidence_device left on the device.
        dummy_correction: the particles of the served choices (latent_dummy_served) that chose, or stand for, the
        ProposalDummyValue are weighed as block_proposal.jl:49-60 does (excl then names the drawn strings that rows
        hold: inference.latent_current_choices); latent_weights() returns the corrections afterwards."""
        pl = self.lw.latent_plans[cname]
        cfg = config.as_c() if isinstance(config, InferenceConfig) else config
        self._refuse_prior_product(cfg, "Engine.sweep_latent", pl["node_info"])
        self.hip.set_active_rows(0, -1)
        if dummy_correction or getattr(self, "_latent_dummy_on", False):  # (a reload makes a fresh context: set per call)
            self.hip.set_latent_dummy_correction(dummy_correction)
            self._latent_dummy_on = bool(dummy_correction)
        if dummy_correction:  # (keyed choices: which option is the dummy of each row's key)
            dk = self.latent_dummy_options(trace, cname, np.asarray(live))
            if dk is not None:
                self.hip.set_latent_dummy_options(dk)
        if ev_begin is not None:
            return self.hip.sweep_latent_resident(cfg, seed, sweep_idx, pl["block_id"], pl["roots"], live, ev_off, ev_begin,
                                                  excl, len(pl["nodes"]))
        return self.hip.sweep_latent(cfg, seed, sweep_idx, pl["block_id"], pl["roots"], live, ev_off, ev_rows, ev_ctx,
                                     excl, len(pl["nodes"]))

    def latent_weights(self):
        """log-weight corrections [rows][particles] of the last sweep_latent(..., dummy_correction=True) (parity checks)"""
        return self.hip.get_latent_weights()

    def build_evidence_device(self, trace, cname):
        """inference.build_evidence on the device (pclean_build_evidence): returns (live, ev_off, None, None) with the ordered
        evidence rows and their per-row ctx values left in HBM for sweep_latent(..., ev_rows=None, ev_begin=...), or None
        when this class / state takes the host path (no device-resident referents, MaybeSwap / Gaussian evidence contexts,
        a walk longer than the library's, references to dead rows).  Same arrays as the host path, element for element
        (tests/test_gpu_edges.py::test_device_evidence_equals_host)."""
        lw = self.lw
        dc = getattr(self, "_dc", None)
        if dc is None or os.environ.get("PCLEAN_HOST_EVIDENCE"):
            return None
        pl = lw.latent_plans[cname]
        if cname in lw.latent_ev_prob or cname in getattr(lw, "latent_ev_locals", {}):
            return None
        bi = pl["src_block"]
        steps, cn = [], lw.blocks[bi]["root_class"]
        for step in [p for p in pl["path"].split(".") if p]:
            j = lw.colidx[cn][step]
            steps.append((lw.table_id[cn], j))
            cn = lw.layout[cn][j].target
        sources = []
        for ob, col in pl.get("ctx_sources", []):
            sources.append((ob, lw.table_id[lw.blocks[ob]["root_class"]], col))
        if len(steps) > _lib.EV_MAX_STEPS or len(sources) > _lib.MAX_CTX or cn != cname:
            return None
        t = trace.tables[cname]  # (a trace that device commits left behind pulls here)
        self.upload_trace(trace)
        self._sync_cur(trace)
        off = self.hip.build_evidence(bi, steps, t.n, sources)
        counts = np.diff(off)
        if off[0] != 0 or int(off[-1]) != trace.cur.shape[1] or counts[~t.live[:t.n]].any():
            return None  # rows without a referent / referring to dead rows: the host path filters them
        live = np.nonzero(t.live[:t.n])[0].astype(np.int32)
        ev_off = np.zeros(len(live) + 1, dtype=np.int32)
        np.cumsum(counts[live], out=ev_off[1:])
        # (dead rows hold no evidence: the live rows' groups are contiguous in the resident order, live row j's at ev_off[j])
        return live, ev_off, None, None

    def init_device_comm(self, comm):
        """Bind the library's own RCCL communicator to the ranks of `comm` (parallel.Comm over torch.distributed):
        rank 0's rendezvous id travels through torch's object broadcast.  Afterwards sweep_stats_reduced sums the
        delta reference counts on the device with ONE all-reduce over xGMI.  Returns False (and the torch path stays
        in use) when RCCL cannot be bound."""
        self._dev_comm = False
        self._comm = None
        if comm.dist is None:
            return False
        self._comm = comm  # reload() binds the fresh context to the same ranks
        try:
            box = [self.hip.comm_unique_id() if comm.rank == 0 else None]
            comm.dist.broadcast_object_list(box, src=0)
            self.hip.comm_init(comm.world, comm.rank, box[0])
            self._dev_comm = True
        except Exception as e:  # noqa: BLE001 — any failure: keep the torch.distributed exchange
            import sys
            print(f"[pclean] device-side RCCL exchange unavailable ({e}); using torch.distributed", file=sys.stderr)
        return self._dev_comm

    def sweep_stats_reduced(self, trace):
        """Delta reference counts of the last sweep summed over ALL ranks, per block root table — one fused RCCL
        all-reduce of the device-resident buffers (pclean_allreduce_stats_fused); None without init_device_comm."""
        if not getattr(self, "_dev_comm", False):
            return None
        blocks = [bi for bi, blk in enumerate(self.lw.blocks) if not blk.get("score")]
        if getattr(self, "_stats_reduced_on_device", False):  # a refused pclean_commit_device_dist already summed them in place
            self._stats_reduced_on_device = False
            return {bi: self.hip.get_stats(self.lw.table_id[self.lw.blocks[bi]["root_class"]],
                                           trace.tables[self.lw.blocks[bi]["root_class"]].n) for bi in blocks}
        tids = [self.lw.table_id[self.lw.blocks[bi]["root_class"]] for bi in blocks]
        ns = [trace.tables[self.lw.blocks[bi]["root_class"]].n for bi in blocks]
        # a rank that swept nothing contributes zeros (its device buffers hold stale counts)
        return dict(zip(blocks, self.hip.allreduce_stats_fused(tids, ns, getattr(self, "_empty_sweep", False))))

    def sweep_stats(self, trace):
        """Delta reference counts of the last sweep per block root table (the all-reduce payload)."""
        if getattr(self, "_empty_sweep", False):
            return {bi: np.zeros(trace.tables[blk["root_class"]].n, dtype=np.int64)
                    for bi, blk in enumerate(self.lw.blocks) if not blk.get("score")}
        return {bi: self.hip.get_stats(self.lw.table_id[blk["root_class"]], trace.tables[blk["root_class"]].n)
                for bi, blk in enumerate(self.lw.blocks) if not blk.get("score")}
