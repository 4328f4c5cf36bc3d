"""Relational model definition mirroring PClean's `@model` / `@query` DSL, and its
lowering to the static enumeration plan consumed by libpclean_hip.so.

Reference mapping (files under /root/reference/src):
  Model / ClassDef        dsl/syntax.jl:106-161 (`@model`, `@class`), dsl/builder.jl:37-258
  ClassDef.param          `@learned x::ProportionsParameter`   (builder.jl:182-202)
  ClassDef.choice         `x ~ Dist(args...)`                  (builder.jl:234-258)
  ClassDef.fk             `x ~ OtherClass`  (builder.jl:123-175: the target's nodes are
                          inlined, i.e. a row stores a flattened copy of its referents)
  ClassDef.julia          `x = expr`                            (builder.jl:205-231)
  ClassDef.block()        `begin ... end`                       (builder.jl:13-20)
  Query                   dsl/query.jl:1-43
The reference JIT-compiles one Julia function per (class, block, observed set)
(inference/proposal_compiler.jl); here the same enumeration structure is emitted
once as flat arrays (nodes / terms / children / colmap, include/pclean_hip.h).
"""
import math
from contextlib import contextmanager

import numpy as np

from . import _lib
from .encode import Domain, StringPool


# ---------------------------------------------------------------------------
# distributions (src/distributions/*.jl) — declarative descriptors
class StringPrior:
    """string_prior.jl: StringPrior(min_length, max_length, proposal_atoms).  With `keyed_by`
    the atoms are a dict keyed by the value of another attribute of the same class
    (`possibilities[countykey]`, experiments/rents/run.jl:13)."""

    def __init__(self, min_len, max_len, atoms, keyed_by=None):
        self.min_len, self.max_len, self.keyed_by = int(min_len), int(max_len), keyed_by
        self.atoms = {k: list(v) for k, v in atoms.items()} if keyed_by else list(atoms)

    def dummy_value(self):  # string_prior.jl:24-26
        return "*" * ((self.min_len + self.max_len) // 2)


class ChooseUniformly:
    """choose_uniformly.jl: ChooseUniformly(options)."""

    def __init__(self, options):
        self.options = list(options)


class ChooseProportionally:
    """choose_proportionally.jl: ChooseProportionally(options, probs::ProportionsParameter).  With `index` the
    parameter is an IndexedProportionsParameter read at the value of attribute `index` of the same class
    (`probs[key]`, dsl/builder.jl:195-201): one probability vector per value of that attribute."""

    def __init__(self, options, param, index=None):
        self.options, self.param, self.index = list(options), param, index


class AddTypos:
    """add_typos.jl: AddTypos(word[, max_typos]); `ref` names the clean value."""

    def __init__(self, ref, max_typos=None):
        self.ref, self.max_typos = ref, max_typos


class ExpandOnShortVersion:
    """expand_on_short_version.jl: ExpandOnShortVersion(val, options); `ref` names the short (clean) value, the
    observation is one of the `options` that `val` is a case-insensitive subsequence of."""

    def __init__(self, ref, options):
        self.ref, self.options = ref, list(options)


class FormatName:
    """format_name.jl:29-55, the one-name method: FormatName(name) is the name itself or its initial + "."; and
    format_name.jl:14-26, the three-name method, written with keywords: FormatName(first=.., middle=.., last=..) is
    "first middle last" or "first last" (`refs` holds the three references, `ref` the first).  Several POSITIONAL
    references stay refused, as they always were: which of them is the first, the middle and the last name is said by name."""

    def __init__(self, ref=None, *more, first=None, middle=None, last=None):
        if more:
            raise NotImplementedError("FormatName(first, middle, last): first / middle / last form: not lowered from positional "
                                      "references; name them: FormatName(first=..., middle=..., last=...)")
        named = (first, middle, last)
        if ref is not None and all(x is None for x in named):
            self.ref, self.refs = ref, None
        elif ref is None and all(isinstance(x, str) for x in named):
            self.ref, self.refs = first, named
        else:
            raise ValueError("FormatName takes one name, or first=, middle= and last=")


TABULATED = (ExpandOnShortVersion, FormatName)
# the two densities of the three-name FormatName (format_name.jl:18, 22), added left to right as the reference adds them
NAME3_LOG_THREE = math.log(0.9) + math.log(0.9) + math.log(0.9)
NAME3_LOG_TWO = math.log(0.1)
OWN_MAX_OPTIONS = 64 * 4096  # options of one own option list (csrc/own_block.hip: OWN_MAX_OPTIONS)
OWN_STAR_MAX_ARMS = 4  # dependents of one index in a star (csrc/own_star_check.h)
OWN_STAR_MAX_K = 4096  # values of a star's index or of one of its dependents
OWN_STAR_LDS_MAX = 160 * 1024 - 512  # bytes of cached values of a star (csrc/own_block.hip: OWN_PRODUCT_LDS_MAX)
OWN_GAUSS_MAX_OPTIONS = 4096  # options of an own leaf that carries Gaussian terms (csrc/own_block.hip: OWN_GAUSS_MAX_OPTIONS)


class TimePrior:
    """time_prior.jl: TimePrior(proposal_atoms); atoms keyed by another attribute of the class
    (`times_for_flight["$flight_id-field"]`, experiments/flights/run.jl:17-20)."""
    keyed = True

    def __init__(self, atoms, keyed_by):
        self.atoms = {k: list(v) for k, v in atoms.items()}
        self.keyed_by = keyed_by

    def dummy_value(self):  # time_prior.jl:17-19
        return "**:** p.m."


class MaybeSwap:
    """maybe_swap.jl: MaybeSwap(val, options, prob). `val` references the clean value, `options`
    are keyed by the value of `key` (same dict as the TimePrior atoms), `prob` names a ProbLookup."""

    def __init__(self, val, options, key, prob):
        self.val, self.options, self.key, self.prob = val, {k: list(v) for k, v in options.items()}, key, prob


class IndexedProbParameter:
    """`@learned x::Dict{String, ProbParameter{a, b}}` (maybe_swap.jl:36-52)."""

    def __init__(self, a, b):
        self.a, self.b = float(a), float(b)


class ProbLookup:
    """Deterministic node choosing an error probability: fn(*args) returns a float constant or the
    key of the indexed ProbParameter (experiments/flights/run.jl:28)."""

    def __init__(self, param, fn):
        self.param, self.fn = param, fn


class Unmodeled:
    """unmodeled.jl: logdensity 0, no proposal; must be observed."""


class NumberCodePrior:
    """number_code_prior.jl:10-14: logdensity -log(code) of an observed integer code, no proposal; must be observed.
    The values are the observed strings, each a decimal integer >= 1 (so that no density is positive)."""


def number_code(s):
    """the integer a NumberCodePrior value stands for, None when the string is no decimal integer >= 1"""
    if not isinstance(s, str) or not s.isascii() or not s.isdigit():
        return None
    v = int(s)
    return v if v >= 1 else None


class Transformation:
    """transformed_gaussian.jl:5-9 — forward, backward, |g'|."""

    def __init__(self, forward, backward, deriv):
        self.forward, self.backward, self.deriv = forward, backward, deriv


class TransformedGaussian:
    """transformed_gaussian.jl: TransformedGaussian(mean, std, t); `mean` names an IndexedLookup
    julia attribute, `unit` an own ChooseUniformly attribute over Transformations."""

    def __init__(self, mean, std, unit):
        self.mean, self.std, self.unit = mean, float(std), unit


class AddNoise:
    """add_noise.jl:1-7: AddNoise(mean, std), logpdf(Normal(mean, std), x); `mean` names an IndexedLookup julia
    attribute, as TransformedGaussian's does.  No Transformation and no unit choice."""

    def __init__(self, mean, std):
        self.mean, self.std = mean, float(std)


class IndexedMeanParameter:
    """`@learned x::Dict{String, MeanParameter{mean, std}}` (add_noise.jl:15-45, distributions.jl:45-55)."""

    def __init__(self, mean, std):
        self.mean, self.std = float(mean), float(std)


class IndexedLookup:
    """Deterministic node `param[f(args...)]` (experiments/rents/run.jl:23): the parameter indexed by
    the tuple of its discrete arguments."""

    def __init__(self, param):
        self.param = param


class ProportionsParameter:
    """choose_proportionally.jl:31-74 (Dirichlet prior, default concentration 1.0)."""

    def __init__(self, concentration=1.0):
        self.concentration = float(concentration)


class IndexedProportionsParameter:
    """`@learned x::Dict{K, ProportionsParameter{c}}` (dsl/syntax.jl:139-144, distributions.jl:45-61): one Dirichlet
    vector per key, all with the same concentration."""

    def __init__(self, concentration=1.0):
        self.concentration = float(concentration)


# ---------------------------------------------------------------------------
class Attr:
    def __init__(self, kind, name, **kw):
        self.kind, self.name = kind, name
        self.__dict__.update(kw)


class ClassDef:
    def __init__(self, model, name):
        self.model, self.name = model, name
        self.attrs = []        # in declaration order
        self.blocks = []       # list of lists of attr names; [] => whole class is one block
        self._open = None
        self.py_strength, self.py_discount = 1.0, 0.0  # builder.jl:39

    def _add(self, attr):
        if any(a.name == attr.name for a in self.attrs):
            raise ValueError(f"{self.name}.{attr.name} declared twice")
        self.attrs.append(attr)
        if attr.kind != "param":
            if self._open is not None:
                self._open.append(attr.name)
            elif self.blocks and self._implicit:
                self.blocks[-1].append(attr.name)
            else:
                self.blocks.append([attr.name])
                self._implicit = True
        return attr

    _implicit = False

    def param(self, name, prior):
        return self._add(Attr("param", name, prior=prior))

    def choice(self, name, dist):
        return self._add(Attr("choice", name, dist=dist))

    def fk(self, name, target):
        if target not in self.model.classes:
            raise ValueError(f"class {target} must be defined before it is referenced")
        return self._add(Attr("fk", name, target=target))

    def julia(self, name, fn, args):
        return self._add(Attr("julia", name, fn=fn, args=list(args)))

    @contextmanager
    def block(self):
        self._open = []
        self._implicit = False
        self.blocks.append(self._open)
        try:
            yield self
        finally:
            self._open = None

    def attr(self, name):
        for a in self.attrs:
            if a.name == name:
                return a
        raise KeyError(f"{self.name}.{name}")


class Model:
    def __init__(self):
        self.classes = {}
        self.class_order = []

    def add_class(self, name):
        c = ClassDef(self, name)
        self.classes[name] = c
        self.class_order.append(name)
        return c

    def resolve(self, cls, path):
        """Follow a dotted reference from class `cls`; returns (class name, attr)."""
        parts = path.split(".")
        c = self.classes[cls]
        for p in parts[:-1]:
            a = c.attr(p)
            if a.kind != "fk":
                raise ValueError(f"{path}: {p} is not a reference slot")
            c = self.classes[a.target]
        return c.name, c.attr(parts[-1])


class Query:
    """`@query Model.Class [ column clean_expr dirty_expr ]` (dsl/query.jl:15-38).
    bindings: column -> (clean reference, dirty attribute name)."""

    def __init__(self, model, cls, bindings):
        self.model, self.cls = model, cls
        self.cleanmap, self.obsmap = {}, {}
        for col, b in bindings.items():
            clean, dirty = (b, b) if isinstance(b, str) else b
            self.cleanmap[col] = clean
            self.obsmap[col] = dirty


# ---------------------------------------------------------------------------
# lowering
class Column:
    """One flattened column of a latent table."""

    def __init__(self, name, kind, cls, attr, target=None):
        self.name, self.kind, self.cls, self.attr, self.target = name, kind, cls, attr, target


class MappedDomain:
    """Values of a latent domain seen through a single-argument JuliaNode: entry v is the pool string f(value v)
    (repeats allowed) — what a pair table needs of its latent side (ids, lengths)."""

    def __init__(self, pool, strings):
        self.pool = pool
        self.ids = [pool.add(s) for s in strings]

    def __len__(self):
        return len(self.ids)

    def string(self, j):
        return self.pool.strings[self.ids[j]]

    def id_array(self):
        return np.array(self.ids, dtype=np.int32)


class LoweredModel:
    """Domains, flattened table layouts, option tables and per-block plans."""

    def __init__(self, model, query, dirty_columns, pool=None, extra_latent=None, own_star=False):
        """own_star: a flat observed class may hold several dependents on one index in one own block; they are lowered as a
        star (_lower_own_block: a head node and one arm per dependent, enumerated collapsed).  Off, every plan and refusal is
        what it was.
        extra_latent {(class, attribute): [strings]}: values a latent attribute holds although they are neither
        proposal atoms nor the dummy — strings drawn by random(StringPrior / TimePrior) for a chosen
        ProposalDummyValue (block_proposal.jl:58-60).  They are appended to the attribute's domain (ids of the
        atoms and the dummy do not move) and are never options of a proposal."""
        self.model, self.query = model, query
        self.own_star_enabled = bool(own_star)
        self._dirty_columns = dirty_columns
        self.extra_latent = {k: list(v) for k, v in (extra_latent or {}).items()}
        self.pool = pool or StringPool()
        self.latent_dom = {}   # (class, attr) -> Domain of latent values
        self.obs_dom = {}      # dirty attr name -> Domain of observed values
        self.layout = {}       # class -> [Column]
        self.colidx = {}       # class -> {dotted name: index}
        self.table_id = {}     # class -> candidate table id
        self.option_id = {}    # (class, attr) -> option table id
        self.pair_id = {}      # (dirty attr) -> pair table id
        self.fn_tables = {}    # fn id -> ndarray
        self.blocks = []       # dicts: nodes, terms, children, colmap, ctx_src_block, ctx_src_col, root_class
        self.obs_cols = []     # dirty attr name per observed column id
        self.obs_index = {}
        self._next_table = 0
        self._next_pair = 0
        self.cross_terms = []
        self.eq_pairs = {}
        self.same_pairs = {}   # pair id -> (observed domain, latent domain): 0 iff same string
        self.class_pairs = {}  # pair id -> (class rule, observed domain, latent domain, options or None): tabulated terms
        self._class_key = {}
        self.name3_terms = {}  # block id (observed-class block or latent plan) -> {term index: spec}: see _lower_name3
        self.prob_spec = None
        self.gauss = {}        # (block id, node id) -> dict spec (resolved by the engine): the node's first Gaussian term
        self.gauss_more = {}   # (block id, node id) -> [dict spec, ...]: its further terms, in declaration order
        self.gauss_specs = []  # the block's Gaussian observations in declaration order (gauss_spec is gauss_specs[0])
        self.locals = {}       # block index -> [own ChooseUniformly attrs enumerated with the Gaussian]
        self.latent_ev_locals = {}  # latent class -> block index whose locals feed the evidence ctx
        self.latent_ev_prob = {}    # latent class -> scoring block whose error-prob index feeds the evidence ctx
        self.latent_plans = {}
        self._build_domains(dirty_columns)
        self._resolve_indexed()
        self._build_layouts()
        self._build_blocks()
        self._build_latent_plans()

    # -- domains ------------------------------------------------------------
    def _build_domains(self, dirty_columns):
        m = self.model
        for cname in m.class_order:
            for a in m.classes[cname].attrs:
                if a.kind != "choice":
                    continue
                d = a.dist
                if (isinstance(d, StringPrior) and d.keyed_by) or isinstance(d, TimePrior):
                    dom = Domain(self.pool)
                    for k, atoms in d.atoms.items():
                        for s_ in atoms:
                            dom.add(s_)
                    dom.add(d.dummy_value())
                elif isinstance(d, StringPrior):
                    dom = Domain(self.pool, d.atoms)
                    dom.add(d.dummy_value())
                elif isinstance(d, ChooseProportionally):
                    dom = Domain(self.pool, d.options)
                elif isinstance(d, ChooseUniformly) and all(isinstance(o, str) for o in d.options):
                    dom = Domain(self.pool, d.options)
                else:
                    continue
                for s_ in self.extra_latent.get((cname, a.name), ()):
                    dom.add_extra(s_)  # ids after the dummy's: never an option (MaybeSwap: "val in options")
                self.latent_dom[(cname, a.name)] = dom
        ocls = m.classes[self.query.cls]
        self.direct_obs = {}   # obs name -> (path or own attr name) observed without noise (clean == dirty)
        self.numeric_obs = {}  # own TransformedGaussian / AddNoise attr -> numeric column index
        self.num_cols = []
        self.num_derived = []  # (source numeric column, Transformation, "backward" | "logabsderiv"): see _lower_gaussian
        for col, dirty in self.query.obsmap.items():
            own = None
            if "." not in dirty:
                own = ocls.attr(dirty)
            if own is not None and own.kind == "choice" and isinstance(own.dist, (AddTypos, MaybeSwap) + TABULATED):
                vals = [v for v in dirty_columns[col] if v is not None]
                if isinstance(own.dist, ExpandOnShortVersion):
                    # logdensity would be -log(0) for a value no option list can have produced
                    # (expand_on_short_version.jl:38): with this check every "is a short version" pair has a count >= 1
                    stray = sorted(set(vals) - set(own.dist.options))
                    if stray:
                        raise ValueError(f"{dirty}: observed value {stray[0]!r} is not among the options of "
                                         "ExpandOnShortVersion")
                self.obs_dom[dirty] = Domain(self.pool, list(dict.fromkeys(vals)))
            elif own is not None and own.kind == "choice" and isinstance(own.dist, (TransformedGaussian, AddNoise)):
                self.numeric_obs[dirty] = len(self.num_cols)
                self.num_cols.append(col)
                continue
            else:
                # direct observation of a latent value or of an own discrete choice: the observed
                # domain IS the latent domain (proposal_compiler.jl:277-293 compares values)
                if own is not None:
                    key = (self.query.cls, dirty)
                else:
                    head, rest = dirty.split(".", 1)
                    cn, la = m.resolve(ocls.attr(head).target, rest)
                    key = (cn, la.name)
                if key not in self.latent_dom:  # e.g. Unmodeled: its values are whatever is observed
                    vals = [v for v in dirty_columns[col] if v is not None]
                    if isinstance(getattr(m.classes[key[0]].attr(key[1]), "dist", None), NumberCodePrior):
                        for v in vals:
                            if number_code(v) is None:
                                raise ValueError(f"{col}: value {v!r} is not a decimal integer >= 1 (NumberCodePrior of "
                                                 f"{key[0]}.{key[1]})")
                    self.latent_dom[key] = Domain(self.pool, list(dict.fromkeys(vals)))
                self.obs_dom[dirty] = self.latent_dom[key]
                self.direct_obs[dirty] = key
            self.obs_index[dirty] = len(self.obs_cols)
            self.obs_cols.append(dirty)
        for cname in m.class_order:  # (number_code_prior.jl:1: "for _observed_ number codes")
            for a in m.classes[cname].attrs:
                if a.kind == "choice" and isinstance(a.dist, NumberCodePrior):
                    if cname == self.query.cls:
                        raise NotImplementedError(f"{cname}.{a.name}: NumberCodePrior among the observed class's own choices "
                                                  "is not lowered")
                    if (cname, a.name) not in self.direct_obs.values():
                        raise ValueError(f"{cname}.{a.name}: a NumberCodePrior value must be observed directly")
        self.query_columns = {dirty: col for col, dirty in self.query.obsmap.items()}
        self._never_missing = {dirty for col, dirty in self.query.obsmap.items()
                               if all(v is not None for v in dirty_columns[col])}

    def _resolve_indexed(self):
        """ChooseProportionally(options, param, index=attr): how each indexed choice is lowered.  self.indexed maps
        (class, dependent attribute) -> ("keyed", index attribute): the index is observed directly (e.g. Unmodeled) and the
        choice is lowered as keyed StringPrior atoms are — options (value, key) for every key of the index's domain, the
        equality term on the observed key; or -> ("product", index attribute): the index is a sibling ChooseProportionally /
        ChooseUniformly choice declared before it in the same block, and the two become ONE leaf over the |A| x |B| joint
        options (proposal_compiler.jl:55-129 enumerates them jointly).  Everything else is refused by name."""
        m = self.model
        self.indexed = {}
        self.product_index = {}  # (class, index attribute) -> its dependent: the two are enumerated as one product leaf
        self.star_index = {}     # (observed class, index attribute) -> [its dependents, two and more]: a star (own_star=True)
        for cname in m.class_order:
            cls = m.classes[cname]
            seen = {}
            for a in cls.attrs:
                if a.kind != "choice" or not isinstance(a.dist, ChooseProportionally):
                    continue
                prior = cls.attr(a.dist.param).prior
                ix = a.dist.index
                who = f"{cname}.{a.name}"
                if ix is None:
                    if isinstance(prior, IndexedProportionsParameter):
                        raise ValueError(f"{who}: the IndexedProportionsParameter {a.dist.param} needs index=...")
                    continue
                if not isinstance(prior, IndexedProportionsParameter):
                    raise ValueError(f"{who}: index={ix!r} needs an IndexedProportionsParameter, {a.dist.param} is none")
                if "." in ix:
                    raise NotImplementedError(f"{who}: an index reached through a reference ({ix}) is not lowered")
                ia = cls.attr(ix)
                if ia.kind == "julia":
                    raise NotImplementedError(f"{who}: a JuliaNode index ({ix}) is not lowered")
                if ia.kind != "choice":
                    raise NotImplementedError(f"{who}: the index {ix} is a reference slot, not a value")
                if cname == self.query.cls:
                    self._resolve_own_indexed(cname, cls, a, ia, seen)
                    continue
                if isinstance(ia.dist, ChooseProportionally) and ia.dist.index is not None:
                    raise NotImplementedError(f"{who}: the index {ix} is itself indexed")
                if ix in seen:
                    raise NotImplementedError(f"{who}: {ix} already indexes {seen[ix]}; two dependents on one index are not "
                                              "lowered")
                seen[ix] = a.name
                blk_of = {n: k for k, names in enumerate(cls.blocks) for n in names}
                if blk_of[ix] != blk_of[a.name]:
                    raise NotImplementedError(f"{who}: the index {ix} is declared in another block")
                if [x.name for x in cls.attrs].index(ix) > [x.name for x in cls.attrs].index(a.name):
                    raise NotImplementedError(f"{who}: the index {ix} must be declared before the choice")
                if isinstance(ia.dist, (ChooseProportionally, ChooseUniformly)):
                    # the product leaf stands at the dependent's place: nothing declared between the two may read the index
                    names = [x.name for x in cls.attrs]
                    for mid in cls.attrs[names.index(ix) + 1:names.index(a.name)]:
                        reads = list(getattr(mid, "args", ())) if mid.kind == "julia" else [
                            getattr(getattr(mid, "dist", None), f, None) for f in ("keyed_by", "index", "ref", "mean", "unit", "val", "key")]
                        if ix in reads:
                            raise NotImplementedError(f"{who}: {mid.name}, declared between the index {ix} and the choice, reads "
                                                      "the index; declare it after the choice")
                    na, nb = len(ia.dist.options), len(a.dist.options)
                    if na * nb > 2 ** 31 - 1:
                        raise NotImplementedError(f"{who}: the product with {ix} has {na} x {nb} options, more than 2^31 - 1")
                    if (cname, ix) not in self.latent_dom:
                        raise NotImplementedError(f"{who}: the options of the index {ix} are not strings")
                    self.indexed[(cname, a.name)] = ("product", ix)
                    self.product_index[(cname, ix)] = a.name
                    continue
                if (cname, ix) not in self.direct_obs.values():
                    raise NotImplementedError(f"{who}: the index {ix} is neither a sibling ChooseProportionally / "
                                              "ChooseUniformly choice nor observed directly")
                # a row whose key is not observed would enumerate the options of every key while its key leaf is drawn on its
                # own: the new row could hold a (key, value) pair never scored under theta[key] and count it for that key
                for obsname, k in self.direct_obs.items():
                    if k == (cname, ix) and obsname not in self._never_missing:
                        raise NotImplementedError(f"{who}: the index {ix} is observed through {obsname}, which has missing "
                                                  "values; the keyed form needs the key of every row")
                self.indexed[(cname, a.name)] = ("keyed", ix)
        self._resolve_own_stars()

    def _resolve_own_indexed(self, cname, cls, a, ia, seen):
        """An indexed own choice of the OBSERVED class: served in a flat class when its index is a sibling own
        ChooseProportionally choice over strings with a plain ProportionsParameter, declared before it in the same block —
        the two become one product leaf at the dependent's place (_lower_own_block).  Everything else is refused by name."""
        ix, who = a.dist.index, f"{cname}.{a.name}"
        if isinstance(ia.dist, ChooseUniformly):
            raise NotImplementedError(f"{who}: an indexed choice among the observed class's own choices is not lowered when "
                                      f"its index ({ix}) is a ChooseUniformly choice; an own index is a ChooseProportionally "
                                      "choice with a plain ProportionsParameter")
        fks = [x.name for x in cls.attrs if x.kind == "fk"]
        if fks:
            raise NotImplementedError(f"{who}: an indexed own choice in a class with a reference-slot block ({', '.join(fks)}) "
                                      "is not lowered; own blocks are served for flat classes alone")
        if not isinstance(ia.dist, ChooseProportionally):
            if (cname, ix) in self.direct_obs.values():
                raise NotImplementedError(f"{who}: the index {ix} is observed directly and is not a choice (the keyed form); "
                                          "among the observed class's own choices the index is a sibling ChooseProportionally "
                                          "choice")
            raise NotImplementedError(f"{who}: the index {ix} is a {type(ia.dist).__name__}, not a sibling ChooseProportionally "
                                      "choice")
        if ia.dist.index is not None:
            raise NotImplementedError(f"{who}: the index {ix} is itself indexed")
        star = self.own_star_enabled
        if ix in seen and not star:
            raise NotImplementedError(f"{who}: {ix} already indexes {seen[ix]}; two dependents on one index are not lowered")
        seen[ix] = a.name
        names = [x.name for x in cls.attrs]
        blk_of = {n: k for k, ns in enumerate(cls.blocks) for n in ns}
        if blk_of[ix] != blk_of[a.name]:
            raise NotImplementedError(f"{who}: the index {ix} is declared in another block")
        if names.index(ix) > names.index(a.name):
            raise NotImplementedError(f"{who}: the index {ix} must be declared before the choice")
        for mid in cls.attrs[names.index(ix) + 1:names.index(a.name)]:
            if star and mid.kind == "choice" and isinstance(mid.dist, ChooseProportionally) and mid.dist.index == ix:
                continue  # (an earlier dependent of the same index: an arm of the same star)
            reads = list(getattr(mid, "args", ())) if mid.kind == "julia" else [
                getattr(getattr(mid, "dist", None), f, None) for f in ("keyed_by", "index", "ref", "mean", "unit", "val", "key")]
            if ix in reads:
                raise NotImplementedError(f"{who}: {mid.name}, declared between the index {ix} and the choice, reads the index; "
                                          "declare it after the choice")
        if (cname, ix) not in self.latent_dom:
            raise NotImplementedError(f"{who}: the options of the index {ix} are not strings")
        na, nb = len(ia.dist.options), len(a.dist.options)
        if na * nb > OWN_MAX_OPTIONS:
            raise NotImplementedError(f"{who}: the product with {ix} has {na} x {nb} = {na * nb} options, more than the "
                                      f"{OWN_MAX_OPTIONS} an own option list holds (OWN_MAX_OPTIONS)")
        self.indexed[(cname, a.name)] = ("product", ix)
        if star:
            self.star_index.setdefault((cname, ix), []).append(a.name)
        self.product_index[(cname, ix)] = a.name

    def _resolve_own_stars(self):
        """own_star=True: an index of the observed class with two and more dependents becomes a star — the dependents are
        marked ("star", index) and leave product_index; an index with ONE dependent stays the product leaf."""
        for (cname, ix), deps in list(self.star_index.items()):
            if len(deps) < 2:
                del self.star_index[(cname, ix)]
                continue
            who = f"{cname}.{ix}"
            if len(deps) > OWN_STAR_MAX_ARMS:
                raise NotImplementedError(f"{who}: {len(deps)} dependents on one index ({', '.join(deps)}); a star holds at most "
                                          f"{OWN_STAR_MAX_ARMS} (OWN_STAR_MAX_ARMS)")
            cls = self.model.classes[cname]
            sizes = {n: len(cls.attr(n).dist.options) for n in [ix] + deps}
            for n, k in sizes.items():
                if k > OWN_STAR_MAX_K:
                    raise NotImplementedError(f"{cname}.{n}: {k} options; the index and the dependents of a star hold at most "
                                              f"{OWN_STAR_MAX_K} each")
            for d in deps:
                if (cname, d) not in self.latent_dom:
                    raise NotImplementedError(f"{cname}.{d}: the options of a star's dependent are not strings")
                self.indexed[(cname, d)] = ("star", ix)
            del self.product_index[(cname, ix)]

    def keyed_index(self, cname, aname):
        """attribute whose (directly observed) value selects the options of choice aname: StringPrior / TimePrior atoms
        `keyed_by` it, or the key of an IndexedProportionsParameter; None for an ordinary choice"""
        d = self.model.classes[cname].attr(aname).dist if cname in self.model.classes else None
        if (isinstance(d, StringPrior) and d.keyed_by) or isinstance(d, TimePrior):
            return d.keyed_by
        return self.indexed.get((cname, aname), (None, None))[1]

    def gauss_backward(self, rows, unit_idx, g=0):
        """unit.backward(x) of the g-th Gaussian observation of `rows` under the Transformation options unit_idx (one per
        row): x * c for the linear ones, the derived column for the others (transformed_gaussian.jl:16, 27-34); AddNoise:
        x * 1.0 (its one option, 0)."""
        spec = self.gauss_specs[g]
        rows = np.asarray(rows)
        unit_idx = np.asarray(unit_idx)
        x = self.xnum[spec["x_col"], rows] * np.asarray(spec["t_scale"])[unit_idx]
        for ui, col in enumerate(spec.get("t_x_col", ())):
            if col >= 0:
                sel = unit_idx == ui
                x[sel] = self.xnum[col, rows[sel]]
        return x

    def relower(self, extra_latent):
        """Grow latent domains by the strings of extra_latent {(class, attribute): [strings]} and rebuild every
        derived table IN PLACE (pair / fn / equality tables, plans): value ids held by a trace stay valid, callers
        keep their reference.  The engine has to reload its static data afterwards (Engine.reload)."""
        merged = {k: list(v) for k, v in self.extra_latent.items()}
        for k, v in extra_latent.items():
            have = merged.setdefault(k, [])
            have.extend(x for x in dict.fromkeys(v) if x not in have)
        dirty = self._dirty_columns
        self.__init__(self.model, self.query, dirty, None, merged, own_star=self.own_star_enabled)
        self.encode_observations(dirty)

    def encode_observations(self, dirty_columns):
        """[n_cols][n_rows] int32 observed-domain indices, -1 = missing."""
        n_rows = len(next(iter(dirty_columns.values())))
        self.xnum = np.array([[np.nan if v is None else float(v) for v in dirty_columns[c]] for c in self.num_cols],
                             dtype=np.float64).reshape(len(self.num_cols), n_rows)
        derived = getattr(self, "num_derived", [])
        if derived:  # backward(x) / log|deriv(backward(x))| of the non-linear Transformations, row by row (_lower_gaussian)
            rows = []
            for src, unit, what in derived:
                col = np.full(n_rows, np.nan)
                for i, x in enumerate(self.xnum[src]):
                    if x == x:
                        bx = float(unit.backward(float(x)))
                        col[i] = bx if what == "backward" else float(np.log(abs(float(unit.deriv(bx)))))
                rows.append(col)
            self.xnum = np.vstack([self.xnum, np.array(rows, dtype=np.float64).reshape(len(rows), n_rows)])
        obs = np.full((len(self.obs_cols), n_rows), -1, dtype=np.int32)
        for j, dirty in enumerate(self.obs_cols):
            dom = self.obs_dom[dirty]
            col = dirty_columns[self.query_columns[dirty]]
            obs[j] = [(-1 if v is None else dom.get(v)) for v in col]
        self.obs_host = obs  # host copy for the sufficient statistics of observation-level parameters
        return obs

    # -- layouts ------------------------------------------------------------
    def _build_layouts(self):
        m = self.model
        for cname in m.class_order:
            if cname == self.query.cls:
                continue
            cols = []
            for a in m.classes[cname].attrs:
                if a.kind == "fk":
                    cols.append(Column(a.name, "fk", cname, a.name, a.target))
                    for c in self.layout[a.target]:
                        cols.append(Column(a.name + "." + c.name, c.kind, c.cls, c.attr, c.target))
                elif a.kind == "choice":
                    cols.append(Column(a.name, "val", cname, a.name))
            self.layout[cname] = cols
            self.colidx[cname] = {c.name: i for i, c in enumerate(cols)}
            self.table_id[cname] = self._next_table
            self._next_table += 1
        self.option_values = {}
        self.option_keycol = {}
        self.option_ncol = {}
        self.option_cols = {}  # (class, attr) of a product leaf -> [2][options] value columns (index's value, own value)
        for (cname, aname), dom in self.latent_dom.items():
            self.option_id[(cname, aname)] = self._next_table
            self._next_table += 1
            # option k of discrete_proposal(dist, ...) is latent-domain value k (atoms are unique,
            # string_prior.jl:15; the dummy value, if any, is last)
            self.option_values[(cname, aname)] = np.arange(dom.n_base(), dtype=np.int32)  # (drawn strings are no options)
            if cname in self.model.classes:
                a = self.model.classes[cname].attr(aname)
                d = getattr(a, "dist", None)
                if (isinstance(d, StringPrior) and d.keyed_by) or isinstance(d, TimePrior):
                    # options = for every key: its atoms, then one dummy option; column 1 = key index
                    kdom = self.latent_dom[(cname, d.keyed_by)]
                    vals, keys = [], []
                    dummy = dom.get(d.dummy_value())
                    for k, atoms in d.atoms.items():
                        ki = kdom.get(k)
                        for s_ in atoms:
                            vals.append(dom.get(s_))
                            keys.append(ki)
                        vals.append(dummy)
                        keys.append(ki)
                    self.option_values[(cname, aname)] = np.array(vals, dtype=np.int32)
                    self.option_keycol[(cname, aname)] = np.array(keys, dtype=np.int32)
                    # column 2: number of atoms of the option's key group (MaybeSwap's length(options))
                    nk = {kdom.get(k): len(atoms) for k, atoms in d.atoms.items()}
                    self.option_ncol[(cname, aname)] = np.array([nk[k] for k in keys], dtype=np.int32)
                elif self.indexed.get((cname, aname), ("", ""))[0] in ("product", "star"):
                    # option a * |B| + b; two value columns: the index's value, the choice's value
                    na, nb = len(self.latent_dom[(cname, self.indexed[(cname, aname)][1])]), len(d.options)
                    self.option_cols[(cname, aname)] = np.stack([np.repeat(np.arange(na, dtype=np.int32), nb),
                                                                 np.tile(np.arange(nb, dtype=np.int32), na)])
                    self.option_values[(cname, aname)] = self.option_cols[(cname, aname)][1]
                elif (cname, aname) in self.indexed:
                    # options = for every key of the index's domain, in domain order: every option; column 1 = key index
                    nk, nb = len(self.latent_dom[(cname, self.indexed[(cname, aname)][1])]), len(d.options)
                    self.option_values[(cname, aname)] = np.tile(np.arange(nb, dtype=np.int32), nk)
                    self.option_keycol[(cname, aname)] = np.repeat(np.arange(nk, dtype=np.int32), nb)

    def option_column(self, cname, aname, cc=0):
        """latent value per option of leaf (cname, aname) for column cc of a new row's colmap entry (a product leaf has two)"""
        cols = self.option_cols.get((cname, aname))
        return self.option_values[(cname, aname)] if cols is None else cols[cc]

    # -- plans --------------------------------------------------------------
    def _obs_terms_of_block(self, ocls, names):
        """Observation choices of a block as (dirty attr, kind, payload)."""
        out = []
        for n in names:
            a = ocls.attr(n)
            if a.kind == "choice" and isinstance(a.dist, (AddTypos,) + TABULATED):
                out.append(a)
        return out

    def _eq_pair_for(self, dom_key):
        """0/1 identity table over a shared domain (observed value must equal the latent value)."""
        key = ("eq", dom_key)
        if key not in self.eq_pairs:
            self.eq_pairs[key] = (self._next_pair, len(self.latent_dom[dom_key]))
            self._next_pair += 1
        return self.eq_pairs[key][0]

    def _pair_for(self, dirty, lat_dom_key, lat_dom):
        key = (dirty, lat_dom_key)
        if key not in self.pair_id:
            self.pair_id[key] = (self._next_pair, self.obs_dom[dirty], lat_dom)
            self._next_pair += 1
        return self.pair_id[key][0]

    def _class_pair_for(self, dirty, lat_dom_key, dist, rule=None):
        """class table of a tabulated observation (ExpandOnShortVersion / FormatName) over obs domain x latent domain;
        `rule` given: one of the two byte tables of a three-name FormatName (CLASS_NAME_PREFIX / CLASS_NAME_SUFFIX)"""
        key = (dirty, lat_dom_key) if rule is None else (dirty, lat_dom_key, rule)
        if key not in self._class_key:
            if rule is not None:
                options = None
            else:
                rule, options = ((_lib.CLASS_SHORT_VERSION, list(dist.options)) if isinstance(dist, ExpandOnShortVersion)
                                 else (_lib.CLASS_FORMAT_NAME, None))
            if options is not None:
                self.pool.add_all(options)  # (the device counts over the option strings: they live in the pool)
            self.class_pairs[self._next_pair] = (rule, self.obs_dom[dirty], self.latent_dom[lat_dom_key], options)
            self._class_key[key] = self._next_pair
            self._next_pair += 1
        return self._class_key[key]

    def _build_blocks(self):
        m = self.model
        ocls = m.classes[self.query.cls]
        root_of_block = []
        fk_block = {}
        self.score_blocks = {}
        # A block of the observed class with several reference slots (PCleanClass.blocks, model.jl:100-106) is lowered
        # into one ENGINE block per slot, proposed in declaration order with no resampling in between (block_group:
        # run_smc! resamples between the class's blocks only, row_inference.jl:152-155).  An observation belongs to the
        # last slot it mentions; a JuliaNode across two slots of one block reads the earlier slot's value as context.
        # Independent slots are enumerated independently by the reference as well (process_plan!,
        # proposal_compiler.jl:363-388); slots tied by a JuliaNode are proposed here one after the other, each given
        # the earlier ones, instead of jointly.
        eblocks, self.block_group = [], []
        for ub, names in enumerate(ocls.blocks):
            fks = [n for n in names if ocls.attr(n).kind == "fk"]
            if len(fks) <= 1:
                eblocks.append(list(names))
                self.block_group.append(ub)
                continue
            order = {f: i for i, f in enumerate(fks)}
            groups = [[f] for f in fks]

            def heads(a):
                if a.kind == "julia":
                    return [x.split(".", 1)[0] for x in a.args]
                ref = getattr(a.dist, "ref", None) if a.kind == "choice" else None
                if ref is None:
                    return []
                if "." in ref:
                    return [ref.split(".", 1)[0]]
                return heads(ocls.attr(ref))
            for n in names:
                a = ocls.attr(n)
                if a.kind == "fk":
                    continue
                hs = [order[h] for h in heads(a) if h in order]
                groups[max(hs) if hs else len(fks) - 1].append(n)
            for g in groups:
                eblocks.append(g)
                self.block_group.append(ub)
        self.engine_blocks = eblocks
        for bi, names in enumerate(eblocks):
            fks = [n for n in names if ocls.attr(n).kind == "fk"]
            root_of_block.append(fks[0] if fks else None)
            if fks:
                fk_block[fks[0]] = bi
        # A block without a reference slot that holds a choice other than a MaybeSwap observation is an OWN block: its own
        # discrete choices are enumerated from their observations (_lower_own_block).  Served for FLAT classes alone — every
        # block an own block: a class that mixes the two kinds would need the own values to follow the ancestor permutation
        # of the particles inside the sweep.
        self.own_leaf = {}   # own choice of the observed class -> (block, node) of its leaf
        self.own_product = {}  # own choice indexed by a sibling own choice -> that index: the two share ONE product leaf
        self.own_star = {}   # (block, head node) of a star -> [its arm nodes] (own_star=True: _lower_own_star)
        self.own_gauss = {}  # (block, node) of a Gaussian leaf -> dict(table, factors, sizes, cols, specs): _lower_own_gauss
        own_blocks = [bi for bi, names in enumerate(eblocks) if root_of_block[bi] is None and any(
            ocls.attr(n).kind == "choice" and not isinstance(ocls.attr(n).dist, MaybeSwap) for n in names)]
        self.flat = bool(own_blocks) and len(own_blocks) == len(eblocks)
        if own_blocks and not self.flat:
            first = next(n for n in eblocks[own_blocks[0]] if ocls.attr(n).kind == "choice")
            others = [n for k, n in enumerate(root_of_block) if n is not None]
            raise NotImplementedError(
                f"{self.query.cls}.{first}: a choice in a block without a reference slot, in a class that also has "
                + (f"reference-slot blocks ({', '.join(others)})" if others else "a MaybeSwap scoring block")
                + "; own blocks are served for flat classes alone (every block without a reference slot), mixed classes are "
                  "not lowered")
        for bi, names in enumerate(eblocks):
            if bi in own_blocks:
                self.blocks.append(self._lower_own_block(bi, ocls, names))
                continue
            if root_of_block[bi] is None:
                self._lower_score_block(bi, ocls, names, fk_block)
                self.blocks.append(dict(score=True, nodes=[], terms=[], children=[], colmap=[], node_info=[],
                                        root_class=None, root_fk=None, ctx_src_block=[], ctx_src_col=[]))
                continue
            root_fk = ocls.attr(root_of_block[bi])
            blk = dict(nodes=[], terms=[], children=[], colmap=[], ctx_src_block=[], ctx_src_col=[],
                       root_class=root_fk.target, root_fk=root_fk.name, node_info=[])
            # collect observation terms of this block: (dirty attr, path below root, ctx spec)
            terms = []
            for a in self._obs_terms_of_block(ocls, names):
                ref = a.dist.ref
                if isinstance(a.dist, FormatName) and a.dist.refs is not None:
                    terms.append(self._lower_name3(a, root_fk))
                    continue
                if isinstance(a.dist, TABULATED):
                    # a term DENS_TABULATED exactly where an AddTypos term of the same `ref` would go
                    if "." not in ref:
                        if ocls.attr(ref).kind == "choice":
                            raise NotImplementedError(f"{a.name}: {type(a.dist).__name__} of the own choice {ref} in a block with "
                                                      f"the reference slot {root_fk.name} (joint enumeration) is not lowered")
                        raise NotImplementedError(f"{a.name}: {type(a.dist).__name__} of a JuliaNode value is not lowered")
                    head, rest = ref.split(".", 1)
                    if head != root_fk.name:
                        raise NotImplementedError(f"{a.name}: reference outside the block's root slot")
                    cname, la = m.resolve(root_fk.target, rest)
                    if (cname, la.name) not in self.latent_dom:
                        raise NotImplementedError(f"{a.name}: {type(a.dist).__name__} of a value without a string domain")
                    pid = self._class_pair_for(a.name, (cname, la.name), a.dist)
                    terms.append(dict(obs=a.name, path=rest, pair=pid, max_typos=None, ctx=None, dens=_lib.DENS_TABULATED))
                    continue
                if "." in ref:
                    head, rest = ref.split(".", 1)
                    if head != root_fk.name:
                        raise NotImplementedError(f"{a.name}: reference outside the block's root slot")
                    cname, la = m.resolve(root_fk.target, rest)
                    pid = self._pair_for(a.name, (cname, la.name), self.latent_dom[(cname, la.name)])
                    terms.append(dict(obs=a.name, path=rest, pair=pid, max_typos=a.dist.max_typos, ctx=None))
                else:
                    j = ocls.attr(ref)
                    if j.kind != "julia":
                        raise NotImplementedError(f"{a.name}: AddTypos of a non-reference: the own choice {ref} stands in a block "
                                                  f"with the reference slot {root_fk.name}, where the reference enumerates the two "
                                                  "jointly; own choices are enumerated in blocks without a reference slot alone")
                    local = [x for x in j.args if x.split(".", 1)[0] == root_fk.name]
                    other = [x for x in j.args if x.split(".", 1)[0] != root_fk.name]
                    if len(local) != 1 or len(other) > 1:
                        raise NotImplementedError(f"{j.name}: a JuliaNode under an AddTypos observation combines ONE value of "
                                                  "its block's slot with at most one value of an earlier slot; functions of "
                                                  "several values of one slot, or of three and more slots, are not lowered")
                    lc, la = m.resolve(root_fk.target, local[0].split(".", 1)[1])
                    ldom = self.latent_dom[(lc, la.name)]
                    if other:
                        ohead, orest = other[0].split(".", 1)
                        sb = fk_block[ohead]
                        if sb >= bi:
                            raise NotImplementedError("ctx must come from an earlier block")
                        ocn, oa = m.resolve(ocls.attr(ohead).target, orest)
                        odom = self.latent_dom[(ocn, oa.name)]
                        src = (sb, self.colidx[ocls.attr(ohead).target][orest])
                        have = list(zip(blk["ctx_src_block"], blk["ctx_src_col"]))
                        if src in have:  # two JuliaNodes reading the same earlier value share its ctx slot
                            slot = have.index(src)
                        else:
                            slot = len(have)
                            if slot >= _lib.MAX_CTX:
                                raise NotImplementedError(f"a block reads more than {_lib.MAX_CTX} earlier values through JuliaNodes "
                                                          "(PCLEAN_MAX_CTX)")
                            blk["ctx_src_block"].append(sb)
                            blk["ctx_src_col"].append(src[1])
                        order = [j.args.index(other[0]), j.args.index(local[0])]
                        jdom = Domain(self.pool)
                        fn = np.zeros((len(odom), len(ldom)), dtype=np.int32)
                        for x in range(len(odom)):
                            for y in range(len(ldom)):
                                argv = [None, None]
                                argv[order[0]] = odom.string(x)
                                argv[order[1]] = ldom.string(y)
                                fn[x, y] = jdom.add(j.fn(*argv))
                        fid = len(self.fn_tables)
                        self.fn_tables[fid] = fn
                        pid = self._pair_for(a.name, ("julia", j.name), jdom)
                        terms.append(dict(obs=a.name, path=local[0].split(".", 1)[1], pair=pid,
                                          max_typos=a.dist.max_typos, ctx=(slot, fid)))
                        # the same observation also constrains the OTHER argument's class (external
                        # likelihood of e.g. County.state through Record.stateavg_obs)
                        self.cross_terms.append(dict(obs=a.name, pair=pid, max_typos=a.dist.max_typos, fn=fid,
                                                     ctx_block=sb, ctx_path=orest, local_block=bi,
                                                     local_path=local[0].split(".", 1)[1]))
                    else:
                        # f(one value of this slot): a pair table whose latent string of value v is f(v) — the
                        # distances and word lengths AddTypos needs (add_typos.jl:56-63), nothing else changes
                        mdom = MappedDomain(self.pool, [j.fn(ldom.string(y)) for y in range(len(ldom))])
                        pid = self._pair_for(a.name, ("julia", j.name), mdom)
                        terms.append(dict(obs=a.name, path=local[0].split(".", 1)[1], pair=pid,
                                          max_typos=a.dist.max_typos, ctx=None))
            # direct (noise-free) observations of values below the root slot: equality constraints
            for obsname, key in self.direct_obs.items():
                if "." in obsname and obsname.split(".", 1)[0] == root_fk.name:
                    terms.append(dict(obs=obsname, path=obsname.split(".", 1)[1], pair=self._eq_pair_for(key),
                                      max_typos=None, ctx=None, dens=_lib.DENS_EQUAL))
            self._emit_fk_node(blk, root_fk.target, "", terms, parent=-1, parent_fk_col=-1)
            if blk.get("name3"):
                self.name3_terms[bi] = blk["name3"]
            self.blocks.append(blk)
            self._lower_gaussian(bi, blk, ocls, names, root_fk)

    def _lower_name3(self, a, root_fk):
        """`a ~ FormatName(first, middle, last)` (format_name.jl:14-26) -> one term DENS_NAME3 that reads three values of the
        candidate: on the slot's node three columns of the flattened candidate table; in the new-row branch the reference
        enumerates the unobserved names JOINTLY (proposal_compiler.jl:55-129), which the forest of separable leaves has no
        place for — so at most one of the three may be an enumerated choice, whose leaf carries the term and reads the
        other two from the row's own direct observations (never missing, so that the evidence rows of one latent row
        agree on them); with all three observed the first name's leaf carries it."""
        m = self.model
        who = f"{a.name}: FormatName({', '.join(a.dist.refs)})"
        rests, keys = [], []
        for ref in a.dist.refs:
            if "." not in ref:
                raise NotImplementedError(f"{who}: {ref} is a JuliaNode value or an own attribute, not a value of the block's "
                                          "reference slot; not lowered")
            head, rest = ref.split(".", 1)
            if head != root_fk.name:
                raise NotImplementedError(f"{who}: {ref} is a reference outside the block's root slot {root_fk.name}")
            cname, la = m.resolve(root_fk.target, rest)
            if la.kind != "choice":
                raise NotImplementedError(f"{who}: {ref} is a JuliaNode value or a reference slot, not a choice; not lowered")
            if (cname, la.name) not in self.latent_dom:
                raise NotImplementedError(f"{who}: {ref} is a value without a string domain")
            rests.append(rest)
            keys.append((cname, la.name))
        if len({k[0] for k in keys}) != 1 or len({r.rpartition(".")[0] for r in rests}) != 1:
            raise NotImplementedError(f"{who}: the three names must be attributes of one class reached through one path")
        if len(set(keys)) != 3:
            raise NotImplementedError(f"{who}: the three names must be three different attributes")
        obsnames = [root_fk.name + "." + r for r in rests]
        open_ = [i for i, o in enumerate(obsnames) if o not in self.direct_obs]
        if len(open_) > 1:
            raise NotImplementedError(f"{who}: {' and '.join(a.dist.refs[i] for i in open_)} are {'both' if len(open_) == 2 else 'all'} enumerated choices of a new "
                                      f"{keys[0][0]} row; the reference would enumerate the product of their options, which "
                                      "the separable leaves of a new row cannot hold — at most one of the three names may be "
                                      "unobserved")
        for i, o in enumerate(obsnames):
            if i not in open_ and o not in self._never_missing:
                raise NotImplementedError(f"{who}: the directly observed name {a.dist.refs[i]} is missing in some rows; then "
                                          "the reference would enumerate the product of it and the other names")
        carrier = keys[open_[0] if open_ else 0][1]
        if (keys[0][0], carrier) in self.product_index or self.indexed.get((keys[0][0], carrier), ("", ""))[0] == "product":
            raise NotImplementedError(f"{who}: {carrier} is enumerated jointly with another choice (a product leaf); the "
                                      "reference would enumerate the product with the names")
        prefix = self._class_pair_for(a.name, keys[0], a.dist, _lib.CLASS_NAME_PREFIX)
        suffix = self._class_pair_for(a.name, keys[2], a.dist, _lib.CLASS_NAME_SUFFIX)
        return dict(obs=a.name, path=rests[0], pair=prefix, max_typos=None, ctx=None, dens=_lib.DENS_NAME3,
                    name3=dict(paths=tuple(rests), suffix=suffix, doms=tuple(keys), carrier=carrier, obsnames=tuple(obsnames)))

    @staticmethod
    def _below(t, head):
        """term t as the sub-tree of reference slot `head` sees it (paths relative to it), None when it lives elsewhere"""
        if "." not in t["path"] or t["path"].split(".", 1)[0] != head:
            return None
        t = dict(t, path=t["path"].split(".", 1)[1])
        if t.get("name3"):  # (the three names share their path: _lower_name3)
            t["name3"] = dict(t["name3"], paths=tuple(p.split(".", 1)[1] for p in t["name3"]["paths"]))
        return t

    def name3_call(self, spec):
        """arguments of set_term_name3 behind (block, term) for the spec `_emit_term` recorded"""
        odom = self.obs_dom[spec["obs"]]
        f, mid, last = (self.latent_dom[k] for k in spec["doms"])
        return ([k for k, _ in spec["src"]], [c for _, c in spec["src"]], spec["suffix"], odom.id_array(), f.id_array(),
                mid.id_array(), last.id_array(), NAME3_LOG_THREE, NAME3_LOG_TWO)

    def _emit_term(self, blk, t, cand_col, n3src=None):
        if t.get("name3"):
            blk.setdefault("name3", {})[len(blk["terms"])] = dict(t["name3"], obs=t["obs"], src=list(n3src))
        blk["terms"].append((self.obs_index[t["obs"]], cand_col, t["pair"], t.get("dens", _lib.DENS_ADD_TYPOS),
                             -1 if t["max_typos"] is None else int(t["max_typos"]),
                             -1 if t["ctx"] is None else t["ctx"][0], -1 if t["ctx"] is None else t["ctx"][1], 0))

    def _emit_fk_node(self, blk, cname, prefix, terms, parent, parent_fk_col):
        """Node enumerating rows of latent class `cname`; `terms` are the observation
        terms whose clean value lives in this sub-tree (paths relative to it)."""
        m = self.model
        nid = len(blk["nodes"])
        blk["nodes"].append(None)
        blk["node_info"].append(dict(kind="fk", cls=cname, attr=None, path=prefix[:-1]))
        tb = len(blk["terms"])
        for t in terms:
            n3 = t.get("name3")
            self._emit_term(blk, t, self.colidx[cname][t["path"]],
                            n3 and [(_lib.NAME3_CAND, self.colidx[cname][p]) for p in n3["paths"]])
        nt = len(blk["terms"]) - tb
        # children: own attributes of the class, in declaration order
        kids = []
        colsrc = {}
        for a in m.classes[cname].attrs:
            if a.kind == "fk":
                sub = [x for x in (self._below(t, a.name) for t in terms) if x is not None]
                cid = self._emit_fk_node(blk, a.target, prefix + a.name + ".", sub, nid, self.colidx[cname][a.name])
                kids.append(cid)
                colsrc[a.name] = (-1, -1)
                for c in self.layout[a.target]:
                    colsrc[a.name + "." + c.name] = (cid, self.colidx[a.target][c.name])
            elif a.kind == "choice":
                if (cname, a.name) in self.product_index:
                    continue  # enumerated jointly with its dependent: column 0 of that leaf
                prod = self.indexed.get((cname, a.name), ("", ""))
                prod = prod[1] if prod[0] == "product" else None
                # (a product leaf: the terms of the index read value column 0, those of the choice column 1, declaration order)
                def here(t):  # (a name3 term sits on the leaf of its carrier, whichever of its names that is)
                    if t.get("name3"):
                        return "." not in t["path"] and t["name3"]["carrier"] == a.name
                    return t["path"] == a.name or (prod is not None and t["path"] == prod)
                sub = [t for t in terms if here(t)]
                cid = len(blk["nodes"])
                ltb = len(blk["terms"])
                for t in sub:
                    if t.get("name3"):  # the option's value for this name, the row's own observations for the other two
                        src = [(_lib.NAME3_CAND, 0) if p == a.name else (_lib.NAME3_OBS, self.obs_index[o])
                               for p, o in zip(t["name3"]["paths"], t["name3"]["obsnames"])]
                        self._emit_term(blk, t, 0, src)
                        continue
                    self._emit_term(blk, t, 1 if prod is not None and t["path"] == a.name else 0)
                n_leaf_terms = len(sub)
                keyed_by = self.keyed_index(cname, a.name) if prod is None else None
                if keyed_by:
                    # atoms belong to the key they were listed under: the option's key must equal the
                    # (directly observed) key of this row
                    kt = [t for t in terms if t["path"] == keyed_by and t.get("dens") == _lib.DENS_EQUAL]
                    if len(kt) != 1:
                        raise NotImplementedError("keyed atoms need their key attribute observed directly")
                    self._emit_term(blk, kt[0], 1)
                    n_leaf_terms += 1
                # (the per-observed-value cache has no slot for the missing observation a tabulated term scores)
                cacheable = int(n_leaf_terms == 1 and len(sub) == 1 and sub[0]["ctx"] is None
                                and sub[0].get("dens") not in (_lib.DENS_TABULATED, _lib.DENS_NAME3) and prod is None)
                # the ProposalDummyValue of the proposal (string_prior.jl:16-26, time_prior.jl:15-19): which latent
                # value is the placeholder and what random(dist) samples when the dummy is chosen
                dval, dspec = 0, 0
                if isinstance(a.dist, (StringPrior, TimePrior)):
                    dval = self.latent_dom[(cname, a.name)].get(a.dist.dummy_value()) + 1
                    if isinstance(a.dist, TimePrior):
                        dspec = _lib.DUMMY_TIME_PRIOR
                    else:
                        if not (0 <= int(a.dist.min_len) <= 255 and 0 <= int(a.dist.max_len) <= 255):
                            raise NotImplementedError(f"{cname}.{a.name}: StringPrior lengths beyond 255 do not fit the "
                                                      "dummy specification (device draws use DUMMY_MAX_LEN = 255)")
                        dspec = _lib.DUMMY_STRING_PRIOR | (int(a.dist.min_len) << 8) | (int(a.dist.max_len) << 16)
                blk["nodes"].append((_lib.NODE_LEAF, self.option_id[(cname, a.name)], ltb, n_leaf_terms, 0, 0, nid, -1,
                                     cacheable, 0, dval, dspec))
                blk["node_info"].append(dict(kind="leaf", cls=cname, attr=a.name, path=prefix + a.name))
                kids.append(cid)
                colsrc[a.name] = (cid, 0)
                if prod is not None:
                    blk["node_info"][-1]["product"] = (prod, a.name)
                    colsrc[prod], colsrc[a.name] = (cid, 0), (cid, 1)
        cb = len(blk["children"])
        blk["children"].extend(kids)
        cmb = len(blk["colmap"]) // 2
        for c in self.layout[cname]:
            blk["colmap"].extend(colsrc[c.name])
        blk["nodes"][nid] = (_lib.NODE_FK, self.table_id[cname], tb, nt, cb, len(kids), parent, parent_fk_col, 0, cmb,
                             0, 0)
        return nid

    def _lower_own_block(self, bi, ocls, names):
        """Block of a flat observed class: every own choice (`ChooseProportionally` with a plain ProportionsParameter,
        `ChooseUniformly` over strings) becomes one NODE_LEAF on its option table, carrying the block's observations of it in
        declaration order (AddTypos, ExpandOnShortVersion, one-name FormatName) and, last, the equality term of a direct
        observation in the query — the order a new row's leaf gives them (_emit_fk_node).  The reference enumerates such a
        block like any other (proposal_compiler.jl:55-129); the choices of one block are separable (no observation reads two
        of them), so each is enumerated on its own.  The exception is a choice indexed by a sibling choice
        (_resolve_own_indexed): the two become ONE leaf at the dependent's place over the grid a * |B| + b of the two-column
        option table (option_cols), the index's terms on value column 0, then the choice's on column 1; own_leaf maps both
        choices to that leaf and own_product names the pair.  Everything else is refused by name."""
        cls = self.query.cls
        blk = dict(own=True, nodes=[], terms=[], children=[], colmap=[], node_info=[], root_class=None, root_fk=None,
                   ctx_src_block=[], ctx_src_col=[])
        block_of = {n: k for k, ns in enumerate(self.engine_blocks) for n in ns}
        choices, observations = [], []
        # Gaussian observations of the block that the query binds (an unbound one scores nothing) and the unit choices they name
        gauss_obs = [ocls.attr(n) for n in names if ocls.attr(n).kind == "choice"
                     and isinstance(ocls.attr(n).dist, (TransformedGaussian, AddNoise)) and n in self.numeric_obs]
        gauss_units = list(dict.fromkeys(g.dist.unit for g in gauss_obs if isinstance(g.dist, TransformedGaussian)))
        for n in names:
            a = ocls.attr(n)
            if a.kind != "choice":
                continue  # (a JuliaNode is refused where an observation reads it)
            d, who = a.dist, f"{cls}.{n}"
            if isinstance(d, (AddTypos,) + TABULATED):
                observations.append(a)
            elif isinstance(d, (TransformedGaussian, AddNoise)):
                continue  # (a term of the block's Gaussian leaf: _lower_own_gauss)
            elif n in gauss_units and isinstance(d, ChooseUniformly) and (cls, n) not in self.latent_dom:
                choices.append(a)  # (a unit: a factor of the Gaussian leaf)
            elif isinstance(d, (StringPrior, TimePrior, NumberCodePrior)):
                raise NotImplementedError(f"{who}: a {type(d).__name__} own choice is not lowered (its proposal holds a dummy value "
                                          "or none at all); own choices are ChooseProportionally or ChooseUniformly")
            elif isinstance(d, ChooseProportionally):
                if d.index is not None and self.indexed.get((cls, n), ("", ""))[0] not in ("product", "star"):  # (_resolve_indexed refuses it first)
                    raise NotImplementedError(f"{who}: an indexed choice among the observed class's own choices is not lowered")
                choices.append(a)
            elif isinstance(d, ChooseUniformly):
                if (cls, n) not in self.latent_dom:
                    raise NotImplementedError(f"{who}: an own ChooseUniformly choice whose options are not strings is not lowered")
                choices.append(a)
            else:
                raise NotImplementedError(f"{who}: a {type(d).__name__} choice in a block without a reference slot is not lowered")
        by_choice = {c.name: [] for c in choices}
        for a in observations:
            who = f"{cls}.{a.name}"
            if isinstance(a.dist, FormatName) and a.dist.refs is not None:
                raise NotImplementedError(f"{who}: FormatName({', '.join(a.dist.refs)}) reads several own choices; the reference "
                                          "would enumerate their product, which separable leaves cannot hold")
            ref = a.dist.ref
            if "." in ref:
                raise NotImplementedError(f"{who}: {type(a.dist).__name__}({ref}) reads a value behind a reference slot from a "
                                          "block without one")
            r = ocls.attr(ref)
            if r.kind == "julia":
                raise NotImplementedError(f"{who}: {type(a.dist).__name__} of the JuliaNode {ref} of an own choice is not lowered")
            if ref in gauss_units:
                raise NotImplementedError(f"{who}: {type(a.dist).__name__} of the unit choice {ref} (its options are "
                                          "Transformations, not strings) is not lowered")
            if ref not in by_choice:
                if block_of.get(ref) != bi:
                    raise NotImplementedError(f"{who}: its choice {ref} is declared in another block; an observation is scored in "
                                              "the block of its choice")
                raise NotImplementedError(f"{who}: {ref} is not an enumerated own choice")
            if a.name in self.obs_index:  # (an observation the query does not bind scores nothing)
                by_choice[ref].append(a)

        def emit_terms(c, cand_col):
            """the observations of own choice c in declaration order, then the equality term of its direct observation"""
            key = (cls, c.name)
            dom = self.latent_dom[key]
            for a in by_choice[c.name]:
                if isinstance(a.dist, TABULATED):
                    t = dict(obs=a.name, pair=self._class_pair_for(a.name, key, a.dist), max_typos=None, ctx=None,
                             dens=_lib.DENS_TABULATED)
                else:
                    t = dict(obs=a.name, pair=self._pair_for(a.name, key, dom), max_typos=a.dist.max_typos, ctx=None)
                self._emit_term(blk, t, cand_col)
            if c.name in self.direct_obs:
                col = self._dirty_columns[self.query_columns[c.name]]
                stray = sorted({v for v in col if v is not None and dom.get(v) < 0})
                if stray:
                    raise ValueError(f"{cls}.{c.name}: observed value {stray[0]!r} is not among the options of the choice")
                self._emit_term(blk, dict(obs=c.name, pair=self._eq_pair_for(key), max_typos=None, ctx=None,
                                          dens=_lib.DENS_EQUAL), cand_col)

        factors, looks = self._own_gauss_factors(bi, ocls, names, choices, gauss_obs, gauss_units) if gauss_obs else ([], [])
        for c in choices:
            key = (cls, c.name)
            if c.name in factors:
                if c.name == factors[-1]:  # the Gaussian leaf stands at the place of the factor declared last
                    self._lower_own_gauss(bi, blk, ocls, factors, gauss_obs, looks, emit_terms)
                continue
            if key in self.product_index:
                continue  # enumerated jointly with its dependent: value column 0 of that leaf
            if self.indexed.get(key, ("", ""))[0] == "star":
                continue  # an arm of its index's star: lowered right after the head
            if key in self.star_index:
                self._lower_own_star(bi, blk, ocls, c, emit_terms)
                continue
            tb = len(blk["terms"])
            index = self.indexed.get(key, ("", ""))
            index = index[1] if index[0] == "product" else None
            if index is not None:
                # ONE leaf over the grid a * |B| + b (option_cols, key-major): the index's terms read value column 0, the
                # choice's column 1
                emit_terms(ocls.attr(index), 0)
                emit_terms(c, 1)
                if len(blk["terms"]) - tb > _lib.MAX_TERMS:
                    raise NotImplementedError(f"{cls}.{c.name}: the product leaf with {index} carries more than "
                                              f"{_lib.MAX_TERMS} terms (PCLEAN_MAX_TERMS)")
                self.own_leaf[index] = (bi, len(blk["nodes"]))
                self.own_product[c.name] = index
            else:
                emit_terms(c, 0)
            self.own_leaf[c.name] = (bi, len(blk["nodes"]))
            blk["nodes"].append((_lib.NODE_LEAF, self.option_id[key], tb, len(blk["terms"]) - tb, 0, 0, -1, -1, 0, 0, 0, 0))
            blk["node_info"].append(dict(kind="leaf", cls=cls, attr=c.name, path=c.name))
            if index is not None:
                blk["node_info"][-1]["product"] = (index, c.name)
        if not choices:
            raise NotImplementedError(f"{cls}: a block without a reference slot and without an own choice "
                                      f"({', '.join(names)}) is not lowered")
        return blk

    def _lower_own_star(self, bi, blk, ocls, c, emit_terms):
        """The star of index c: 1 + D consecutive NODE_LEAF nodes at the index's place.  The HEAD on the index's own option
        table with the index's terms (value column 0); then arm j on dependent j's two-column table a * K_j + b (option_cols,
        key-major) with the dependent's terms on value column 1 — the arm's prior is log theta_j[a][b] alone (engine.py,
        option_prior), log p(a) belongs to the head.  own_leaf maps every choice to its own node and
        own_star[(block, head node)] lists the arm nodes; Trace.own keeps one row per choice holding its own option index."""
        cls = self.query.cls
        deps = self.star_index[(cls, c.name)]
        head = len(blk["nodes"])
        t0 = len(blk["terms"])
        per_node = []
        for n, col in [(c.name, 0)] + [(d, 1) for d in deps]:
            tb = len(blk["terms"])
            emit_terms(ocls.attr(n), col)
            per_node.append(len(blk["terms"]) - tb)
            self.own_leaf[n] = (bi, len(blk["nodes"]))
            blk["nodes"].append((_lib.NODE_LEAF, self.option_id[(cls, n)], tb, per_node[-1], 0, 0, -1, -1, 0, 0, 0, 0))
            blk["node_info"].append(dict(kind="leaf", cls=cls, attr=n, path=n, star=(c.name, tuple(deps))))
        if len(blk["terms"]) - t0 > _lib.MAX_TERMS:
            raise NotImplementedError(f"{cls}.{c.name}: the star with {', '.join(deps)} carries more than {_lib.MAX_TERMS} terms "
                                      "(PCLEAN_MAX_TERMS)")
        ka = len(c.dist.options)
        ks = [len(ocls.attr(d).dist.options) for d in deps]
        lds = 8 * (per_node[0] * ka + sum(t * k for t, k in zip(per_node[1:], ks)) + ka + (ka + 63) // 64)
        if lds > OWN_STAR_LDS_MAX:
            raise NotImplementedError(f"{cls}.{c.name}: the star with {', '.join(deps)} caches {lds} bytes of term values, more "
                                      f"than the {OWN_STAR_LDS_MAX} of a workgroup's LDS (no second kernel variant)")
        self.own_star[(bi, head)] = [head + 1 + j for j in range(len(deps))]

    def _own_gauss_factors(self, bi, ocls, names, choices, gauss_obs, gauss_units):
        """(factors, lookups) of the Gaussian observations of own block bi.  The factors are the choices of the block that
        some Gaussian term reads — a mean index argument or the unit — in declaration order: at most one string choice
        (ChooseProportionally with a plain ProportionsParameter, ChooseUniformly over strings) and at most one unit.
        Everything else is refused by name."""
        cls = self.query.cls

        def get(n):
            try:
                return ocls.attr(n)
            except (KeyError, TypeError):
                return None
        if len(gauss_obs) > _lib.MAX_GAUSS:
            raise NotImplementedError(f"{cls}.{gauss_obs[_lib.MAX_GAUSS].name}: more than {_lib.MAX_GAUSS} Gaussian observations "
                                      "in one block (PCLEAN_MAX_GAUSS)")
        by_name = {c.name: c for c in choices}
        looks, seen, strings = [], {}, []
        for g in gauss_obs:
            who = f"{cls}.{g.name}"
            look = get(g.dist.mean)
            if (look is None or look.kind != "julia" or not isinstance(look.fn, IndexedLookup)
                    or not isinstance(getattr(get(look.fn.param), "prior", None), IndexedMeanParameter)):
                raise NotImplementedError(f"{who}: the mean {g.dist.mean} of a Gaussian observation in an own block must be an "
                                          "IndexedLookup of an IndexedMeanParameter")
            if look.fn.param in seen:
                raise NotImplementedError(f"{who}: only one Gaussian observation per block may read the mean parameter "
                                          f"{look.fn.param} ({seen[look.fn.param]} already does)")
            seen[look.fn.param] = g.name
            looks.append(look)
            for arg in look.args:
                if "." in arg:
                    raise NotImplementedError(f"{who}: the mean index {arg} lies behind a reference; in an own block a mean is "
                                              "indexed by an own string choice of the same block")
                r = get(arg)
                if r is not None and r.kind == "julia":
                    raise NotImplementedError(f"{who}: the mean index {arg} is a JuliaNode; in an own block a mean is indexed by "
                                              "an own string choice of the same block")
                if arg in gauss_units or arg not in by_name:
                    what = ("a unit choice" if arg in gauss_units else
                            "observed directly and not a choice" if (cls, arg) in self.direct_obs.values() else
                            "declared in another block" if {n: k for k, ns in enumerate(self.engine_blocks) for n in ns}.get(arg, bi) != bi
                            else "no enumerated own choice")
                    raise NotImplementedError(f"{who}: the mean index {arg} is {what}; in an own block a mean is indexed by an own "
                                              "string choice of the same block")
                if arg not in strings:
                    strings.append(arg)
        if len(strings) > 1:
            raise NotImplementedError(f"{cls}: the Gaussian observations of a block read two string factors "
                                      f"({', '.join(strings)}); at most one string factor and one unit are enumerated jointly")
        if len(gauss_units) > 1:
            raise NotImplementedError(f"{cls}: the Gaussian observations of a block read more than two factors (the units "
                                      f"{', '.join(gauss_units)}); at most one string factor and one unit are enumerated jointly")
        for u in gauss_units:
            ua = get(u)
            if ua is None or u not in by_name or not isinstance(ua.dist, ChooseUniformly) or not all(
                    isinstance(o, Transformation) for o in ua.dist.options):
                raise NotImplementedError(f"{cls}.{u}: the unit of a Gaussian observation in an own block must be a ChooseUniformly "
                                          "choice over Transformations declared in the same block")
            if len(ua.dist.options) > 4:
                raise NotImplementedError(f"{cls}.{u}: more than 4 units to choose from (pclean_gauss::t_scale[4])")
            if u in self.direct_obs:
                raise NotImplementedError(f"{cls}.{u}: a directly observed unit choice is not lowered")
        for f in strings:
            d = by_name[f].dist
            if (isinstance(d, ChooseProportionally) and d.index is not None) or (cls, f) in self.product_index or (cls, f) in self.star_index:
                raise NotImplementedError(f"{cls}.{f}: a factor of a Gaussian observation that is itself indexed, or that indexes "
                                          "a sibling choice, is not lowered (no product leaf inside a Gaussian leaf)")
        factors = [c.name for c in choices if c.name in strings or c.name in gauss_units]
        if not factors:
            raise NotImplementedError(f"{cls}.{gauss_obs[0].name}: a Gaussian observation that reads no own choice of its block "
                                      "(a constant mean and no unit) is not lowered")
        k = int(np.prod([len(by_name[f].dist.options) for f in factors], dtype=np.int64))
        if k > OWN_GAUSS_MAX_OPTIONS:
            raise NotImplementedError(f"{cls}: the Gaussian leaf over {' x '.join(factors)} has {k} options, more than the "
                                      f"{OWN_GAUSS_MAX_OPTIONS} it may hold (OWN_GAUSS_MAX_OPTIONS)")
        # The cleaned column of a numeric observation is the query's JuliaNode on the observation (and its unit), e.g.
        # round(unit.backward(rent)), as on the rents path.  A column whose clean side is the observation itself or the mean
        # lookup would be reported as something else than the program says (the raw number; the mean parameter's value).
        for g in gauss_obs:
            col = next(c for c, d in self.query.obsmap.items() if d == g.name)
            clean = get(self.query.cleanmap[col]) if "." not in self.query.cleanmap[col] else None
            if clean is None or clean.kind != "julia" or isinstance(clean.fn, IndexedLookup) or g.name not in clean.args:
                raise NotImplementedError(
                    f"{cls}.{g.name}: a Gaussian observation in a block without a reference slot is lowered only when the query "
                    f"reports its column ({col}) through a JuliaNode of the observation (and its unit), e.g. "
                    f"round(unit.backward({g.name})); {self.query.cleanmap[col]} is none")
        return factors, looks

    def _lower_own_gauss(self, bi, blk, ocls, factors, gauss_obs, looks, emit_terms):
        """The Gaussian leaf of own block bi: ONE NODE_LEAF over the factors' full grid a * |B| + b (key-major, as the product
        leaf's; one factor: its options), on an option table of its own with one value column per factor.  Its terms: the
        string terms of the factors in factor order (emit_terms: declaration order, the equality term of a direct observation
        last), then — attached by the engine after pclean_load_own_block — the Gaussian terms in declaration order
        (self.own_gauss[(block, node)]["specs"], also appended to self.gauss_specs: term g reads mean table g).  own_leaf maps
        every factor to the leaf; two factors are a pair of own_product, so Trace.own keeps one row per choice and the joint
        value is encoded as the product leaf's is."""
        cls = self.query.cls
        tb, nid = len(blk["terms"]), len(blk["nodes"])
        sizes = [len(ocls.attr(f).dist.options) for f in factors]
        for col, f in enumerate(factors):
            if (cls, f) in self.latent_dom:
                emit_terms(ocls.attr(f), col)
        if len(blk["terms"]) - tb > _lib.MAX_TERMS:
            raise NotImplementedError(f"{cls}.{factors[-1]}: the Gaussian leaf carries more than {_lib.MAX_TERMS} string terms "
                                      "(PCLEAN_MAX_TERMS)")
        tid = self._next_table
        self._next_table += 1
        if len(factors) == 2:
            cols = np.stack([np.repeat(np.arange(sizes[0], dtype=np.int32), sizes[1]),
                             np.tile(np.arange(sizes[1], dtype=np.int32), sizes[0])])
            self.own_product[factors[1]] = factors[0]
        else:
            cols = np.arange(sizes[0], dtype=np.int32)[None, :]
        specs = []
        for g, look in zip(gauss_obs, looks):
            spec, dims, transform = self._gaussian_term(len(self.gauss_specs), g, look, ocls, None, factors)
            spec = dict(spec, kinds=[("local", d[1]) for d in dims], n_locals=len(factors), transform=transform, leaf=(bi, nid),
                        term=len(specs))
            self.gauss_specs.append(spec)
            specs.append(spec)
        self.gauss_spec = self.gauss_specs[0]
        for f in factors:
            self.own_leaf[f] = (bi, nid)
        self.own_gauss[(bi, nid)] = dict(table=tid, factors=list(factors), sizes=sizes, cols=cols, specs=specs)
        blk["nodes"].append((_lib.NODE_LEAF, tid, tb, len(blk["terms"]) - tb, 0, 0, -1, -1, 0, 0, 0, 0))
        blk["node_info"].append(dict(kind="leaf", cls=cls, attr=factors[-1], path=factors[-1], gauss=tuple(factors)))

    def own_block_arrays(self, bi):
        """Arguments of pclean_load_own_block behind the block id: (nodes, terms)."""
        return self.block_arrays(bi)[:2]

    def score_block_args(self, bi):
        """Arguments of pclean_load_score_block for scoring block bi."""
        sb = self.score_blocks[bi]
        t, pr = sb["terms"], sb["prob"]
        return (bi, [x["obs"] for x in t], [x["pair"] for x in t], [c for x in t for c in x["val"]],
                [c for x in t for c in x["key"]], [x["nopt_fn"] for x in t], [x["other"] for x in t], pr["fn"],
                list(pr["a"]), list(pr["b"]))

    def load_blocks_into(self, target):
        """Upload every block plan (observed-class blocks, scoring blocks, latent-class plans) into an
        object exposing load_block / load_score_block (the HIP context or the oracle world)."""
        for bi, blk in enumerate(self.blocks):
            if blk.get("own"):
                if not hasattr(target, "load_own_block"):
                    raise NotImplementedError("a flat observed class (own blocks): this target does not know own blocks")
                target.load_own_block(bi, *self.own_block_arrays(bi))
            elif blk.get("score"):
                target.load_score_block(*self.score_block_args(bi))
            else:
                target.load_block(bi, *self.block_arrays(bi))
        for cname, pl in self.latent_plans.items():
            target.load_block(pl["block_id"], *self.latent_block_arrays(cname))
        for bid, specs in self.name3_terms.items():  # (after the blocks: pclean_load_block forgets them)
            if not hasattr(target, "set_term_name3"):
                raise NotImplementedError("FormatName(first, middle, last): this target does not know name3 terms")
            for ti, spec in specs.items():
                target.set_term_name3(bid, ti, *self.name3_call(spec))
        if len(set(self.block_group)) < len(self.block_group):  # a model block with several reference slots
            for bi, g in enumerate(self.block_group):
                target.set_block_group(bi, g)

    def same_pair_table(self, pid):
        odom, vdom = self.same_pairs[pid]
        return (odom.id_array()[:, None] != vdom.id_array()[None, :]).astype(np.uint8)

    def _lower_score_block(self, bi, ocls, names, fk_block):
        """Block without a reference slot: MaybeSwap observations of values chosen in earlier blocks
        (experiments/flights/run.jl:29-34)."""
        m = self.model
        terms = []
        prob_spec = None
        for n in names:
            a = ocls.attr(n)
            if a.kind != "choice":
                continue
            if not isinstance(a.dist, MaybeSwap):
                raise NotImplementedError("a block without a reference slot may only hold MaybeSwap observations")
            vh, vrest = a.dist.val.split(".", 1)
            kh, krest = a.dist.key.split(".", 1)
            vcls, vattr = m.resolve(ocls.attr(vh).target, vrest)
            kcls, kattr = m.resolve(ocls.attr(kh).target, krest)
            vdom, kdom = self.latent_dom[(vcls, vattr.name)], self.latent_dom[(kcls, kattr.name)]
            # 0/1 "same string" table between the observed values and the latent domain
            odom = self.obs_dom[n]
            pid = self._next_pair
            self._next_pair += 1
            self.same_pairs[pid] = (odom, vdom)
            nopt = np.ones((len(kdom), 1), dtype=np.int32)
            for k, opts in a.dist.options.items():
                if kdom.get(k) >= 0:
                    nopt[kdom.get(k), 0] = len(opts)
            fid = len(self.fn_tables)
            self.fn_tables[fid] = nopt
            terms.append(dict(obs=self.obs_index[n], pair=pid, val=(fk_block[vh], self.colidx[ocls.attr(vh).target][vrest]),
                              key=(fk_block[kh], self.colidx[ocls.attr(kh).target][krest]), nopt_fn=fid,
                              other=vdom.get(vattr.dist.dummy_value()), attr=n, val_ref=a.dist.val))
            pl = ocls.attr(a.dist.prob)
            if pl.kind != "julia" or not isinstance(pl.fn, ProbLookup):
                raise NotImplementedError("MaybeSwap prob must be a ProbLookup")
            if prob_spec is None:
                (ah, arest), (bh, brest) = [x.split(".", 1) for x in pl.args]
                acls, aattr = m.resolve(ocls.attr(ah).target, arest)
                bcls, battr = m.resolve(ocls.attr(bh).target, brest)
                adom, bdom = self.latent_dom[(acls, aattr.name)], self.latent_dom[(bcls, battr.name)]
                keys, consts = [], []
                pf = np.zeros((len(adom), len(bdom)), dtype=np.int32)
                for x in range(len(adom)):
                    for y in range(len(bdom)):
                        r = pl.fn.fn(adom.string(x), bdom.string(y))
                        if isinstance(r, float):
                            if r not in consts:
                                consts.append(r)
                            pf[x, y] = consts.index(r)
                        else:
                            if r not in keys:
                                keys.append(r)
                            pf[x, y] = -1 - keys.index(r)
                # prob table layout: constants first, then one entry per parameter key
                pf = np.where(pf < 0, len(consts) + (-1 - pf), pf).astype(np.int32)
                pfid = len(self.fn_tables)
                self.fn_tables[pfid] = pf
                prob_spec = dict(fn=pfid, a=(fk_block[ah], self.colidx[ocls.attr(ah).target][arest]),
                                 b=(fk_block[bh], self.colidx[ocls.attr(bh).target][brest]), consts=consts, keys=keys,
                                 param=(self.query.cls, pl.fn.param))
        self.score_blocks[bi] = dict(terms=terms, prob=prob_spec)
        self.prob_spec = prob_spec

    def _lower_gaussian(self, bi, blk, ocls, names, root_fk):
        """`x ~ TransformedGaussian(param[f(root values, own choices)], std, unit)` with own
        ChooseUniformly choices (experiments/rents/run.jl:19-25), or `x ~ AddNoise(param[..], std)`
        (add_noise.jl:7: no Transformation, no unit choice) -> pclean_gauss specs.  A block may hold up to
        PCLEAN_MAX_GAUSS such observations: each reads its own IndexedMeanParameter, all share the block's own
        choices, which are enumerated once (proposal_compiler.jl:55-129 adds every observed choice's logdensity
        inside the enumeration of the block's own choices)."""
        m = self.model
        ga = [ocls.attr(n) for n in names
              if ocls.attr(n).kind == "choice" and isinstance(ocls.attr(n).dist, (TransformedGaussian, AddNoise))]
        if not ga:
            return
        if len(ga) > _lib.MAX_GAUSS:
            raise NotImplementedError(f"{ga[_lib.MAX_GAUSS].name}: more than {_lib.MAX_GAUSS} Gaussian observations in one "
                                      "block (PCLEAN_MAX_GAUSS)")
        looks, seen = [], {}
        for g in ga:
            look = ocls.attr(g.dist.mean)
            if look.kind != "julia" or not isinstance(look.fn, IndexedLookup):
                raise NotImplementedError(f"{type(g.dist).__name__} mean must be an IndexedLookup")
            if look.fn.param in seen:
                # (each term resamples its own parameter from its own rows: a shared one would need joint statistics)
                raise NotImplementedError(f"{g.name}: only one Gaussian observation per block may read the mean parameter "
                                          f"{look.fn.param} ({seen[look.fn.param]} already does)")
            seen[look.fn.param] = g.name
            looks.append(look)
        # own enumerated choices, shared by the terms: index arguments that are own attrs, plus the units, in the order
        # the terms name them (a choice that only some terms index is still enumerated once)
        locs = []
        for g, look in zip(ga, looks):
            for arg in look.args:
                if "." not in arg:
                    if not isinstance(ocls.attr(arg).dist, ChooseUniformly):
                        raise NotImplementedError("own index arguments must be ChooseUniformly choices")
                    if arg not in locs:
                        locs.append(arg)
            if not isinstance(g.dist, AddNoise) and g.dist.unit not in locs:
                locs.append(g.dist.unit)
        if len(locs) > 2:
            raise NotImplementedError("at most two enumerated own choices")
        if int(np.prod([len(ocls.attr(l).dist.options) for l in locs])) > 16:
            raise NotImplementedError("at most 16 combinations of the enumerated own choices (gauss_combo_scores: sc[16])")
        if locs:  # (an AddNoise whose mean is indexed by candidate-side values alone enumerates nothing: one combination)
            self.locals[bi] = locs
        self.gauss_block = bi
        self.num_derived = []
        self.gauss_specs = []
        open_leaf = None
        for gi, (g, look) in enumerate(zip(ga, looks)):
            spec, dims, transform = self._gaussian_term(gi, g, look, ocls, root_fk, locs)
            self.gauss_specs.append(spec)
            # (a) block root: candidate-side index values come from the candidate's columns
            rc = root_fk.target
            self._add_gauss(bi, 0, dict(spec, kinds=[("cand", self.colidx[rc][d[1]]) if d[0] == "cand" else ("local", d[1])
                                                    for d in dims], n_locals=len(locs), transform=transform))
            # (b) new-row branch: the leaf of the one candidate-side value that is not always observed
            #     carries the term; the others are read from their direct observations
            open_dims = [d for d in dims if d[0] == "cand" and not self._always_observed(root_fk.name + "." + d[1])]
            if len(open_dims) != 1:
                raise NotImplementedError(f"{g.name}: exactly one candidate-side index value may be unobserved")
            if open_leaf is not None and open_dims[0][1] != open_leaf:
                raise NotImplementedError(f"{g.name}: the Gaussian observations of a block must leave the same candidate-side "
                                          f"index value unobserved ({open_leaf}, not {open_dims[0][1]})")
            open_leaf = open_dims[0][1]
            for nid, info in enumerate(blk["node_info"]):
                if info["kind"] == "leaf" and info["path"] == open_dims[0][1]:
                    kinds = []
                    for d in dims:
                        if d[0] == "local":
                            kinds.append(("local", d[1]))
                        elif d is open_dims[0]:
                            kinds.append(("cand", 0))
                        else:
                            kinds.append(("obs", self.obs_index[root_fk.name + "." + d[1]]))
                    self._add_gauss(bi, nid, dict(spec, kinds=kinds, n_locals=len(locs), transform=transform))
                    node = list(blk["nodes"][nid])
                    node[8] = 0  # not cacheable any more
                    blk["nodes"][nid] = tuple(node)
                    if gi == 0:
                        self.gauss_open = (bi, open_dims[0])
        self.gauss_spec = self.gauss_specs[0]

    def _add_gauss(self, bid, nid, term):
        """the node's first term goes to self.gauss, further ones (declaration order) to self.gauss_more"""
        if (bid, nid) not in self.gauss:
            self.gauss[(bid, nid)] = term
        else:
            self.gauss_more.setdefault((bid, nid), []).append(term)

    def _gaussian_term(self, gi, g, look, ocls, root_fk, locs):
        """(spec, index dimensions, transform source) of the block's gi-th Gaussian observation `g`; its mean table id is gi"""
        m = self.model
        add_noise = isinstance(g.dist, AddNoise)
        if add_noise:
            # one fixed identity option: backward(x) = x * 1.0, log|deriv| = 0.0; no choice picks it (transform
            # source "none": the kernels and the oracle take option 0), so the score is logpdf(Normal(mean, std), x)
            units = [Transformation(lambda x: x, lambda x: x, lambda x: 1.0)]
        else:
            units = ocls.attr(g.dist.unit).dist.options
        if len(units) > 4:
            raise NotImplementedError("at most four Transformations to choose from (pclean_gauss::t_scale[4])")
        # A LINEAR unit (backward(x) = c x, |deriv| constant: the rents program's) is evaluated by the kernels as x * c and a
        # constant log|deriv|.  Any other Transformation (transformed_gaussian.jl:5-9 takes arbitrary functions, 15-16
        # evaluates them per observation): x is DATA, so backward(x) and log|deriv(backward(x))| of every row are two
        # more numeric columns, evaluated once on the host (encode_observations) and read by the kernels per row.
        t_linear = []
        for u in units:
            probes = (0.5, 2.0, -3.0, 1267.0)
            try:
                b1 = float(u.backward(1.0))
                d1 = float(u.deriv(b1))
                lin = abs(float(u.backward(0.0))) <= 1e-12 and all(
                    abs(float(u.backward(x)) - x * b1) <= 1e-9 * max(1.0, abs(x * b1)) and
                    abs(float(u.deriv(u.backward(x))) - d1) <= 1e-9 * max(1.0, abs(d1)) for x in probes)
            except (ValueError, ZeroDivisionError, OverflowError, FloatingPointError):
                lin = False  # (a probe outside the function's domain: log of a negative number ...)
            t_linear.append(bool(lin))
        dims = []  # (kind, payload, n_values)
        for arg in look.args:
            if "." in arg:
                head, rest = arg.split(".", 1)
                cn, la = m.resolve(root_fk.target, rest)
                dims.append(("cand", rest, len(self.latent_dom[(cn, la.name)]), (cn, la.name)))
            else:
                dims.append(("local", locs.index(arg), len(ocls.attr(arg).dist.options), None))
        strides, acc = [], 1
        for d in reversed(dims):
            strides.append(acc)
            acc *= d[2]
        strides = strides[::-1]
        spec = dict(x_col=self.numeric_obs[g.name], param=(self.query.cls, look.fn.param), n_mean=acc, dims=dims,
                    strides=strides, locals=locs, local_n=[len(ocls.attr(l).dist.options) for l in locs],
                    local_obs=[self.obs_index.get(l, -1) if l in self.direct_obs else -1 for l in locs],
                    t_local=None if add_noise else locs.index(g.dist.unit), sigma=g.dist.std, gauss_attr=g.name,
                    t_scale=[float(u.backward(1.0)) if lin else 1.0 for u, lin in zip(units, t_linear)],
                    t_lad=[float(np.log(abs(u.deriv(u.backward(1.0))))) if lin else 0.0 for u, lin in zip(units, t_linear)],
                    units=units, t_linear=t_linear, t_x_col=[-1] * len(units), t_lad_col=[-1] * len(units), mean_table=gi)
        # derived numeric columns of the non-linear units: appended behind the observed ones, term by term
        # (encode_observations)
        for ui, lin in enumerate(t_linear):
            if not lin:
                spec["t_x_col"][ui] = len(self.num_cols) + len(self.num_derived)
                self.num_derived.append((spec["x_col"], units[ui], "backward"))
                spec["t_lad_col"][ui] = len(self.num_cols) + len(self.num_derived)
                self.num_derived.append((spec["x_col"], units[ui], "logabsderiv"))
        return spec, dims, ("none", -1) if add_noise else ("local", spec["t_local"])

    def _always_observed(self, obsname):
        return obsname in self.direct_obs and obsname in self._never_missing

    # -- latent-class plans ------------------------------------------------------
    def _build_latent_plans(self):
        """For every latent class T: the sub-plans of its own attributes, scored against all
        observed rows that (transitively) refer to a row of T — the ExternalLikelihoodNodes that
        builder.jl:264-340 adds to T, restated as the children of T's node in the observed plan
        with evidence sets instead of a single row."""
        next_block = len(self.blocks)
        for bi, blk in enumerate(self.blocks):
            if blk.get("score"):
                continue
            for nid, info in enumerate(blk["node_info"]):
                if info["kind"] != "fk" or info["cls"] in self.latent_plans:
                    continue
                cname = info["cls"]
                # per-evidence-row context values of the plan's JuliaNode terms: slot s of the observed block keeps its
                # number (the evidence row's value of that earlier slot); every cross-block JuliaNode whose CONTEXT
                # argument lives in this class adds a slot holding the evidence row's LOCAL argument (_copy_subtree)
                plan = dict(block_id=next_block, src_block=bi, src_node=nid, cls=cname, path=info["path"], nodes=[],
                            terms=[], children=[], colmap=[], node_info=[], roots=[], root_attr=[],
                            ctx_sources=list(zip(blk["ctx_src_block"], blk["ctx_src_col"])))
                node = blk["nodes"][nid]
                for k in range(node[4], node[4] + node[5]):
                    child = blk["children"][k]
                    plan["roots"].append(self._copy_subtree(blk, child, plan, -1, bi))
                    ci = blk["node_info"][child]
                    # attribute of T this root re-proposes
                    # (a product leaf writes two attributes: the pair)
                    plan["root_attr"].append(ci.get("product", ci["attr"]) if ci["kind"] == "leaf" else ci["path"].split(".")[-1])
                self.latent_plans[cname] = plan
                next_block += 1

    def _copy_subtree(self, blk, nid, plan, parent, bi):
        node, info = blk["nodes"][nid], blk["node_info"][nid]
        new_id = len(plan["nodes"])
        plan["nodes"].append(None)
        plan["node_info"].append(dict(info))
        tb = len(plan["terms"])
        for ti, t in enumerate(blk["terms"][node[2]:node[2] + node[3]], start=node[2]):
            t = list(t)
            if t[5] >= 0:
                t[7] = 1  # ctx now comes from the evidence row (fn[ctx][candidate])
            if ti in blk.get("name3", {}):  # (its sources go with it: the option's value, the evidence rows' observations)
                self.name3_terms.setdefault(plan["block_id"], {})[len(plan["terms"])] = blk["name3"][ti]
            plan["terms"].append(tuple(t))
        # cross-block julia observations whose other argument lives in this sub-tree
        for ct in self.cross_terms:
            if ct["ctx_block"] != bi:
                continue
            q, p = ct["ctx_path"], info["path"]
            if info["kind"] == "leaf" and p == q:
                col = 0
            elif info["kind"] == "fk" and q.startswith(p + "."):
                col = self.colidx[info["cls"]][q[len(p) + 1:]]
            else:
                continue
            lb = ct["local_block"]
            src = (lb, self.colidx[self.blocks[lb]["root_class"]][ct["local_path"]])
            if src not in plan["ctx_sources"]:
                if len(plan["ctx_sources"]) >= _lib.MAX_CTX:
                    raise NotImplementedError(f"latent class {plan['cls']}: more than {_lib.MAX_CTX} per-evidence-row context "
                                              "values (PCLEAN_MAX_CTX)")
                plan["ctx_sources"].append(src)
            plan["terms"].append((self.obs_index[ct["obs"]], col, ct["pair"], _lib.DENS_ADD_TYPOS,
                                  -1 if ct["max_typos"] is None else int(ct["max_typos"]), plan["ctx_sources"].index(src),
                                  ct["fn"], 2))
        # MaybeSwap observations (scoring blocks) of this value: external likelihood of the referring rows,
        # each with its own error probability (evidence ctx slot 0 = index into the prob table)
        for sbi, sb in getattr(self, "score_blocks", {}).items():
            for t in sb["terms"]:
                if info["kind"] == "leaf" and t["val"][0] == bi and t["val_ref"].split(".", 1)[1] == info["path"]:
                    plan["terms"].append((t["obs"], 0, t["pair"], _lib.DENS_MAYBE_SWAP, 2, 0, t["other"], 1))
                    self.latent_ev_prob[plan["cls"]] = sbi
        nt = len(plan["terms"]) - tb
        if (bi, nid) in self.gauss and info["kind"] == "leaf":
            # latent sweep of the class owning this value: external likelihood of the referring rows'
            # Gaussian observations, their own choices held at their current values (evidence ctx: the slots of the
            # block's own choices, the same for every term of the node)
            for src in [self.gauss[(bi, nid)]] + self.gauss_more.get((bi, nid), []):
                kinds = [("evctx", k[1]) if k[0] == "local" else k for k in src["kinds"]]
                self._add_gauss(plan["block_id"], new_id, dict(src, kinds=kinds, n_locals=0,
                                                               transform=("none", -1) if src["t_local"] is None
                                                               else ("evctx", src["t_local"])))
                if src["locals"]:
                    self.latent_ev_locals[plan["cls"]] = bi
        kids = []
        if node[0] == _lib.NODE_FK:
            remap = {}
            for k in range(node[4], node[4] + node[5]):
                c = blk["children"][k]
                remap[c] = self._copy_subtree(blk, c, plan, new_id, bi)
                kids.append(remap[c])
            cb = len(plan["children"])
            plan["children"].extend(kids)
            cmb = len(plan["colmap"]) // 2
            ncols = len(self.layout[info["cls"]])
            for j in range(ncols):
                cn, cc = blk["colmap"][2 * (node[9] + j)], blk["colmap"][2 * (node[9] + j) + 1]
                plan["colmap"].extend((remap[cn] if cn >= 0 else -1, cc))
            plan["nodes"][new_id] = (node[0], node[1], tb, nt, cb, len(kids), parent, node[7], 0, cmb, 0, 0)
        else:
            plan["nodes"][new_id] = (node[0], node[1], tb, nt, 0, 0, parent, -1, 0, 0, 0, 0)
        return new_id

    def latent_block_arrays(self, cname):
        pl = self.latent_plans[cname]
        nodes = np.array(pl["nodes"], dtype=_lib.NODE_DTYPE)
        terms = np.array(pl["terms"], dtype=_lib.TERM_DTYPE) if pl["terms"] else np.zeros(0, dtype=_lib.TERM_DTYPE)
        # latent-mode ctx terms read the evidence row's ctx slots (ctx_sources; MaybeSwap / Gaussian evidence: slots 0, 1)
        n_ctx = max(2 if (pl["cls"] in self.latent_ev_locals) else 1, len(pl.get("ctx_sources", [])))
        return (nodes, terms, np.array(pl["children"], dtype=np.int32), np.array(pl["colmap"], dtype=np.int32),
                np.zeros(n_ctx, dtype=np.int32), np.zeros(n_ctx, dtype=np.int32))

    # -- arrays for the C ABI -------------------------------------------------
    def block_arrays(self, bi):
        blk = self.blocks[bi]
        nodes = np.array(blk["nodes"], dtype=_lib.NODE_DTYPE)
        terms = np.array(blk["terms"], dtype=_lib.TERM_DTYPE) if blk["terms"] else np.zeros(0, dtype=_lib.TERM_DTYPE)
        return (nodes, terms, np.array(blk["children"], dtype=np.int32), np.array(blk["colmap"], dtype=np.int32),
                np.array(blk["ctx_src_block"], dtype=np.int32), np.array(blk["ctx_src_col"], dtype=np.int32))
