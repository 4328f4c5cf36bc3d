"""The three-name FormatName (format_name.jl:14-26) without a GPU: the restatement of tests/name3_program.py against a
literal character-by-character check, the lowering (what it accepts, what it refuses and with which words), the two new
walks of pclean_amd/csrc/class_rules.h compiled for the host against the restatement, and the test data itself: every
outcome of the term occurs among the pairs the GPU tests score."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import name3_program as n3
from pclean_amd import _lib
from pclean_amd.model import (ChooseUniformly, FormatName, LoweredModel, Model, Query, StringPrior, Unmodeled,
                              NAME3_LOG_THREE, NAME3_LOG_TWO)

HERE = os.path.dirname(os.path.abspath(__file__))


# ---- 1. the restatement ----------------------------------------------------------------------------------------------------
def _literal(observed, first, middle, last):
    """format_name.jl:14-26 once more, character by character: no str.lower() of a whole string, no f-string"""
    if observed is None:
        return 0.0

    def same(a, b):
        if len(a) != len(b):
            return False
        for x, y in zip(a, b):
            if x.lower() != y.lower():
                return False
        return True
    three = list(first) + [" "] + list(middle) + [" "] + list(last)
    two = list(first) + [" "] + list(last)
    if same(list(observed), three):
        return math.log(0.9) + math.log(0.9) + math.log(0.9)
    if same(list(observed), two):
        return math.log(0.1)
    return -1000.0


HAND = [
    ("Jo Ann Smith", "jo", "ann", "SMITH", n3.LOG_THREE),       # a three-name match
    ("jo smith", "Jo", "Ann", "Smith", n3.LOG_TWO),             # a two-name match
    ("a  b", "a", "", "b", n3.LOG_THREE),                       # an empty middle: two spaces
    ("a b", "a", "", "b", n3.LOG_TWO),                          # ... against one space: the two-name form
    ("al al al al", "al", "al", "al al", n3.LOG_THREE),         # both splittings of "al al al al"
    ("al al al al", "al al", "al", "al", n3.LOG_THREE),
    ("al al al al", "al", "al al", "al", n3.LOG_THREE),
    ("al al al al", "al al", "", "al al", n3.LOG_TWO),
    ("al al al al", "al", "", "al al", n3.NEITHER),
    ("ÉMILE ü zoë", "émile", "Ü", "ZOË", n3.LOG_THREE),         # mixed case beyond ASCII
    ("Émile Zoë", "émile", "ü", "zoë", n3.LOG_TWO),
    (None, "a", "b", "c", 0.0),                                 # a missing observation
    ("al", "al", "", "", n3.NEITHER),                           # a first name equal to the whole observation
    ("al ", "al", "", "", n3.LOG_TWO),                          # ... "al" + " " + "" is the two-name string
    ("al  ", "al", "", "", n3.LOG_THREE),
    ("jo ann smith", "jo", "an", "smith", n3.NEITHER),
    ("jo annsmith", "jo", "ann", "smith", n3.NEITHER),
]


@pytest.mark.parametrize("case", HAND, ids=[repr(c[:4]) for c in HAND])
def test_restatement_equals_the_literal_check(case):
    o, f, m, l, want = case
    assert n3.name3_logdensity(o, f, m, l) == want
    assert _literal(o, f, m, l) == want


def test_restatement_equals_the_literal_check_on_the_program():
    dirty, who, ppl = n3.data()
    n = 0
    for i, o in enumerate(dirty["Full"]):
        for j in (who[i], (who[i] + 1) % len(ppl), i % len(ppl)):
            assert n3.name3_logdensity(o, *ppl[j]) == _literal(o, *ppl[j])
            n += 1
    assert n == 3300
    assert (NAME3_LOG_THREE, NAME3_LOG_TWO) == (n3.LOG_THREE, n3.LOG_TWO)  # the lowering passes the same bits


# ---- 2. lowering -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", n3.VARIANTS)
def test_lowering_accepts_the_three_variants(variant):
    S = n3.setup(variant)
    lw = S["lw"]
    arrays = lw.block_arrays(0)
    nodes, terms = arrays[0], arrays[1]
    k = terms["dens_kind"]
    assert int((k == _lib.DENS_NAME3).sum()) == 2  # one on the slot, one on the carrier's leaf
    assert sorted(r for r, *_ in lw.class_pairs.values()) == [_lib.CLASS_NAME_PREFIX, _lib.CLASS_NAME_SUFFIX]
    root = lw.name3_terms[0][0]
    ci = lw.colidx["Person"]
    assert root["src"] == [(_lib.NAME3_CAND, ci["first"]), (_lib.NAME3_CAND, ci["middle"]), (_lib.NAME3_CAND, ci["last"])]
    carrier = "first" if variant == "observed" else variant
    (ti, leaf), = [(t, s) for t, s in lw.name3_terms[0].items() if t != 0]
    owner = [i for i, nd in enumerate(nodes) if nd["term_begin"] <= ti < nd["term_begin"] + nd["n_terms"]]
    assert [lw.blocks[0]["node_info"][i]["attr"] for i in owner] == [carrier]
    assert nodes[owner[0]]["cacheable"] == 0
    for name, (kind, col) in zip(("first", "middle", "last"), leaf["src"]):
        if name == carrier:
            assert (kind, col) == (_lib.NAME3_CAND, 0)
        else:
            assert (kind, col) == (_lib.NAME3_OBS, lw.obs_index["p." + name])
    # the latent plan of Person holds the carrier's copy
    pl = lw.latent_plans["Person"]
    (pt, pspec), = lw.name3_terms[pl["block_id"]].items()
    assert pspec["src"] == leaf["src"] and pl["terms"][pt][3] == _lib.DENS_NAME3
    # relower rebuilds the same plan
    before = [a.copy() for a in arrays[:2]]
    lw.relower({})
    after = lw.block_arrays(0)
    assert all(np.array_equal(x, y) for x, y in zip(before, after[:2])) and 0 in lw.name3_terms


def _lower(person, refs, bindings, rows=None, extra=None):
    m = Model()
    extra and extra(m)
    p = m.add_class("Person")
    for name, dist in person:
        p.choice(name, dist)
    o = m.add_class("Obs")
    if extra:
        o.fk("q", "Other")
    o.fk("p", "Person")
    if any(r == "nick" for r in refs):
        o.julia("nick", lambda s: s[:1], ["p.first"])
    o.choice("full", FormatName(first=refs[0], middle=refs[1], last=refs[2]))
    rows = rows or {"Full": ["a b c", "a c"], "First": ["a", "a"], "Middle": ["b", "b"], "Last": ["c", "c"], "Other": ["x", "y"]}
    b = dict(bindings, Full=("p.first", "full"))
    return LoweredModel(m, Query(m, "Obs", b), {c: rows[c] for c in b})


U3 = [("first", Unmodeled()), ("middle", Unmodeled()), ("last", Unmodeled())]
ALL = {"First": "p.first", "Middle": "p.middle", "Last": "p.last"}
REFS = ("p.first", "p.middle", "p.last")


def test_lowering_refusals():
    two_open = [("first", Unmodeled()), ("middle", ChooseUniformly(["", "b"])), ("last", StringPrior(1, 9, ["c"]))]
    with pytest.raises(NotImplementedError, match=r"full: FormatName\(p.first, p.middle, p.last\): p.middle and p.last are both "
                                                  r"enumerated choices .* would enumerate the product"):
        _lower(two_open, REFS, {"First": "p.first"})
    three_open = [("first", ChooseUniformly(["a"])), ("middle", ChooseUniformly(["", "b"])), ("last", StringPrior(1, 9, ["c"]))]
    with pytest.raises(NotImplementedError, match=r"p.first and p.middle and p.last are all enumerated .* enumerate the product"):
        _lower(three_open, REFS, {})
    with pytest.raises(NotImplementedError, match=r"FormatName\(p.first, p.middle, q.last\): q.last is a reference outside the "
                                                  r"block's root slot p"):
        def other(m):
            m.add_class("Other").choice("last", Unmodeled())
        _lower(U3, ("p.first", "p.middle", "q.last"), dict(ALL, Other="q.last"), extra=other)
    with pytest.raises(NotImplementedError, match=r"FormatName\(nick, p.middle, p.last\): nick is a JuliaNode value"):
        _lower(U3, ("nick", "p.middle", "p.last"), ALL)
    with pytest.raises(NotImplementedError, match=r"the directly observed name p.middle is missing in some rows; then the "
                                                  r"reference would enumerate the product"):
        _lower(U3, REFS, ALL, rows={"Full": ["a b c", "a c"], "First": ["a", "a"], "Middle": ["b", None], "Last": ["c", "c"]})
    with pytest.raises(NotImplementedError, match=r"must be three different attributes"):
        _lower(U3, ("p.first", "p.first", "p.last"), ALL)
    with pytest.raises(ValueError, match="one name, or first=, middle= and last="):
        FormatName(first="p.first", last="p.last")
    with pytest.raises(ValueError, match="one name, or first=, middle= and last="):
        FormatName("p.name", first="p.first", middle="p.middle", last="p.last")
    # several positional references stay refused, with a message that says how to write the three-name form
    with pytest.raises(NotImplementedError, match=r"first / middle / last form: not lowered from positional references; name them"):
        FormatName("p.first", "p.middle", "p.last")
    d = FormatName(first="p.first", middle="p.middle", last="p.last")
    assert d.refs == ("p.first", "p.middle", "p.last") and d.ref == "p.first" and FormatName("p.name").refs is None


def test_the_one_name_method_is_lowered_as_before():
    import tabulated_program as tp
    lw = tp.setup()["lw"]
    assert not lw.name3_terms and sorted(r for r, *_ in lw.class_pairs.values()) == [tp.SHORT, tp.FORMAT]


def test_load_blocks_into_sets_every_name3_term_after_its_block():
    lw = n3.setup("middle")["lw"]
    calls = []

    class Target:
        def load_block(self, bid, *a):
            calls.append(("block", bid))

        def set_term_name3(self, bid, ti, kinds, cols, suffix, oi, fi, mi, li, l3, l2):
            calls.append(("name3", bid, ti))
            assert (l3, l2) == (n3.LOG_THREE, n3.LOG_TWO) and len(kinds) == 3 and len(cols) == 3
            rule, odom, ldom, _ = lw.class_pairs[suffix]
            assert rule == _lib.CLASS_NAME_SUFFIX and len(oi) == len(odom) and len(li) == len(ldom)
    lw.load_blocks_into(Target())
    pb = lw.latent_plans["Person"]["block_id"]
    assert calls[:2] == [("block", 0), ("block", pb)]
    assert sorted(calls[2:]) == sorted([("name3", 0, 0)] + [("name3", b, t) for b in (0, pb) for t in lw.name3_terms[b] if (b, t) != (0, 0)])

    class Old:
        def load_block(self, *a):
            pass
    with pytest.raises(NotImplementedError, match="does not know name3 terms"):
        lw.load_blocks_into(Old())


# ---- 3. the two walks of class_rules.h, compiled for the host ----------------------------------------------------------------
@pytest.fixture(scope="module")
def host():
    src = os.path.join(HERE, "name3_host", "name3_host.cpp")
    lib = os.path.join(HERE, "name3_host", "libname3_host.so")
    deps = [src, os.path.join(HERE, "..", "pclean_amd", "csrc", "class_rules.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", lib, src])
    L = C.CDLL(lib)
    for f in (L.n3h_prefix, L.n3h_suffix):
        f.restype = C.c_int
        f.argtypes = [C.POINTER(C.c_uint16), C.c_int, C.POINTER(C.c_uint16), C.c_int, C.c_uint16, C.c_int]
    return L


def _folded(s):
    a = np.array([ord(ch.lower()) if len(ch.lower()) == 1 else ord(ch) for ch in s] + [0], dtype=np.uint16)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint16)), len(s)


def test_host_walks_equal_the_restatement_on_the_programs_domains(host):
    S = n3.setup("observed")
    lw = S["lw"]
    odom = lw.obs_dom["full"]
    ostr = [odom.string(u) for u in range(len(odom))] + ["", " ", "al", "al ", " al", "al  al"]
    n_set = [0, 0]
    for which, (fn, walk) in enumerate(((n3.is_prefix, host.n3h_prefix), (n3.is_suffix, host.n3h_suffix))):
        for attr in ("first", "middle", "last"):
            ldom = lw.latent_dom[("Person", attr)]
            lat = [_folded(ldom.string(v)) + (ldom.string(v),) for v in range(len(ldom))]
            for o in ostr:
                _, op, ol = fo = _folded(o)
                for _, vp, vl, v in lat:
                    want = fn(o, v)
                    n_set[which] += want
                    for piece in (1, 3, 64):
                        assert walk(op, ol, vp, vl, ord(" "), piece) == want, (which, o, v, piece)
    assert min(n_set) > 200
    # no separator in the pool: nothing matches
    _, op, ol = _folded("al al")
    _, vp, vl = _folded("al")
    assert host.n3h_prefix(op, ol, vp, vl, 0xFFFF, 64) == 0 and host.n3h_suffix(op, ol, vp, vl, 0xFFFF, 64) == 0


# ---- 4. the input is not degenerate ----------------------------------------------------------------------------------------------
def test_every_outcome_occurs_among_the_scored_pairs():
    """the pairs tests/test_gpu_name3.py scores: every row against the 257-candidate table (the smaller tables are its
    prefixes), and the few-row cases against theirs"""
    dirty, who, ppl = n3.data()
    R = n3.Restated()
    n_out = {n3.LOG_THREE: 0, n3.LOG_TWO: 0, n3.NEITHER: 0}
    both = 0
    for k, rows, _ in n3.SCORE_CASES:
        if k < 257:
            continue
        cand, counts = n3.candidates(k)
        for i in n3.case_rows(len(who), rows):
            o = dirty["Full"][i]
            if o is None:
                continue
            seen = set()
            for c, cnt in zip(cand, counts):
                if cnt:
                    v = R(o, *c)
                    n_out[v] += 1
                    seen.add(v)
            both += int(n3.LOG_THREE in seen and n3.LOG_TWO in seen)
    assert min(n_out.values()) >= 20, n_out
    assert both >= 1  # a row with two candidates that match in different ways ("al bo cy": al|bo|cy and al||bo cy)
    assert sum(o is None for o in dirty["Full"]) >= 20
