"""Tabulated likelihood terms (ExpandOnShortVersion, FormatName) on the host: the restatement's known answers, what the
lowering emits for tests/tabulated_program.py, every refusal of the lowering, and the literal interpreter's two densities
(oracle/literal.py, on strings) against known answers and against the table-shaped restatement."""
import math
import os
import sys

import numpy as np
import pytest

import tabulated_program as tp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import literal as lit  # noqa: E402
from pclean_amd import _lib
from pclean_amd.encode import StringPool
from pclean_amd.engine import class_density_rows
from pclean_amd.model import (AddTypos, ExpandOnShortVersion, FormatName, LoweredModel, Model, Query, StringPrior)


def test_short_version_known_answers():
    assert tp.is_short_version("jm", "Jim")
    assert tp.is_short_version("", "x")
    assert not tp.is_short_version("ab", "ba")
    assert tp.is_short_version("JIM", "jimmy")
    assert not tp.is_short_version("jimmy", "jim")


def test_format_name_known_answers():
    assert tp.format_name_class("j.", "Jim") == 1
    assert tp.format_name_class("JIM", "jim") == 0
    # format_name.jl:49: lowercase(observed) == lowercase("$(name[1]).") — the initial of the one-letter name "J" is "J",
    # so "J." is its initial form (class 1); the name "J." observed as "J" is neither
    assert tp.format_name_class("J.", "J") == 1
    assert tp.format_name_class("J", "J.") == 2
    assert tp.format_name_class("j.", "J.") == 0  # (equality is asked first, format_name.jl:47)
    assert tp.format_name_class("", "") == 0 and tp.format_name_class("x", "") == 2


def test_missing_observation_values():
    T = tp.density_rows(tp.SHORT, ["al", "Sam"], ["Sam", "Alan", "sal"])
    assert T[0, 3] == -1000.0 and T[1, 3] == 0.0  # in(val, options) is string membership
    assert T[0, 0] == -np.log(2.0) and T[1, 0] == -np.log(1.0) and T[0, 1] == -1000.0
    F = tp.density_rows(tp.FORMAT, ["", "a*b", "Jim"])
    assert list(F[:, 3]) == [0.0, -1000.0, -5.0]
    assert list(F[0, :3]) == [-1000.0, -1000.0, -1000.0]  # the empty name against any observation
    assert list(F[2, :3]) == [np.log(0.9999), np.log(0.0001), -1000.0]


def test_engine_density_rows_are_the_restatement():
    """what Engine._upload_static uploads (from the device's counts) equals the restatement's T, bit for bit"""
    lat = tp.NICKS + ["zzz"]
    counts = tp.short_counts(lat, tp.LONGS)
    assert counts[-1] == 0 and counts[:-1].min() >= 1
    want = tp.density_rows(tp.SHORT, lat, tp.LONGS)
    assert np.array_equal(class_density_rows(_lib.CLASS_SHORT_VERSION, lat, tp.LONGS, counts), want)
    names = tp.NAMES + ["", "a*"]
    assert np.array_equal(class_density_rows(_lib.CLASS_FORMAT_NAME, names), tp.density_rows(tp.FORMAT, names))
    assert (want <= 0).all()


def test_program_shape():
    S = tp.setup()
    d = S["dirty"]
    assert len(d["Name"]) == 64 and len(tp.NAMES) == 40 and len(tp.NICKS) == 12 and len(tp.LONGS) == 50
    for col in d.values():
        assert sum(v is None for v in col) == 8
    assert all(d[c][i] is None for c in d for i in (0, 1))
    assert any(ord(ch) > 127 and ch.isupper() for n in tp.NAMES for ch in n) and any(len(n) == 1 for n in tp.NAMES)
    assert sum(not any(tp.is_short_version(n, x) for n in tp.NICKS) for x in tp.LONGS) == 6


def test_lowering_emits_tabulated_terms():
    S = tp.setup()
    lw = S["lw"]
    nodes, terms = lw.block_arrays(0)[:2]
    info = lw.blocks[0]["node_info"]
    tab = terms["dens_kind"] == _lib.DENS_TABULATED
    root = terms[nodes[0]["term_begin"]:nodes[0]["term_begin"] + nodes[0]["n_terms"]]
    assert list(root["dens_kind"]) == [_lib.DENS_TABULATED, _lib.DENS_TABULATED, _lib.DENS_ADD_TYPOS]
    for nid, path, kinds in ((1, "name", [_lib.DENS_TABULATED, _lib.DENS_ADD_TYPOS]), (2, "nick", [_lib.DENS_TABULATED])):
        assert info[nid]["kind"] == "leaf" and info[nid]["path"] == path
        leaf = terms[nodes[nid]["term_begin"]:nodes[nid]["term_begin"] + nodes[nid]["n_terms"]]
        assert list(leaf["dens_kind"]) == kinds
        assert nodes[nid]["cacheable"] == 0
    assert (terms["max_typos"][tab] == -1).all() and (terms["ctx_slot"][tab] == -1).all()
    # the same pair id on the slot and on the new row's leaf, registered in class_pairs
    assert set(terms["pair_table"][tab]) == set(lw.class_pairs)
    rules = {lw.obs_cols[t["obs_col"]]: lw.class_pairs[t["pair_table"]][0] for t in terms[tab]}
    assert rules == {"name_obs": _lib.CLASS_FORMAT_NAME, "long_obs": _lib.CLASS_SHORT_VERSION}
    for pid, (rule, odom, ldom, options) in lw.class_pairs.items():
        assert (options == tp.LONGS) if rule == _lib.CLASS_SHORT_VERSION else options is None
        assert pid not in [p for p, _, _ in lw.pair_id.values()]
    # a nick leaf with the AddTypos observation alone would be cached per observed value; the latent plan carries the terms
    pl = lw.latent_plans["Person"]
    assert sorted(t[3] for t in pl["terms"]) == [_lib.DENS_ADD_TYPOS, _lib.DENS_TABULATED, _lib.DENS_TABULATED]
    lt = lw.latent_block_arrays("Person")[1]
    assert (lt["ctx_slot"][lt["dens_kind"] == _lib.DENS_TABULATED] == -1).all()


def test_fold_map():
    pool = StringPool()
    for s in ["Aa.", "bÉé", "İ"]:
        pool.add(s)
    f = pool.fold_symbols()
    sym = pool.symbol_of
    assert f[sym("A")] == f[sym("a")] == min(sym("A"), sym("a"))
    assert f[sym("É")] == f[sym("é")]
    assert f[sym(".")] == sym(".") and f[sym("b")] == sym("b")
    assert f[sym("İ")] == sym("İ")  # its lowercase is two characters: it stands for itself
    assert pool.symbol_of("?") == 0xFFFF
    assert all(f[s] <= s and f[f[s]] == f[s] for s in range(len(f)))


def _person_model(obs_fn):
    m = Model()
    p = m.add_class("Person")
    p.choice("name", StringPrior(1, 30, ["Jim", "Ann"]))
    o = m.add_class("Obs")
    o.fk("p", "Person")
    obs_fn(o)
    return m


def test_format_name_with_three_references_is_refused():
    with pytest.raises(NotImplementedError, match="first / middle / last form: not lowered"):
        FormatName("p.first", "p.middle", "p.last")


def test_reference_through_a_julia_node_is_refused():
    def obs(o):
        o.julia("shout", lambda name: name.upper(), ["p.name"])
        o.choice("name_obs", FormatName("shout"))
    m = _person_model(obs)
    with pytest.raises(NotImplementedError, match="FormatName of a JuliaNode value is not lowered"):
        LoweredModel(m, Query(m, "Obs", {"Name": ("p.name", "name_obs")}), {"Name": ["JIM", None]})

    def obs2(o):
        o.julia("shout", lambda name: name.upper(), ["p.name"])
        o.choice("long_obs", ExpandOnShortVersion("shout", ["JIMMY"]))
    m = _person_model(obs2)
    with pytest.raises(NotImplementedError, match="ExpandOnShortVersion of a JuliaNode value is not lowered"):
        LoweredModel(m, Query(m, "Obs", {"Long": ("p.name", "long_obs")}), {"Long": ["JIMMY"]})


def test_observed_value_outside_the_options_is_refused():
    m = _person_model(lambda o: o.choice("long_obs", ExpandOnShortVersion("p.name", ["Jimmy", "Anna"])))
    q = Query(m, "Obs", {"Long": ("p.name", "long_obs")})
    LoweredModel(m, q, {"Long": ["Jimmy", None, "Anna"]})
    with pytest.raises(ValueError, match="observed value 'Jimbo' is not among the options of ExpandOnShortVersion"):
        LoweredModel(m, q, {"Long": ["Jimmy", "Jimbo"]})


def test_existing_terms_are_unchanged():
    """an AddTypos observation next to the new ones lowers as it did: its own distance table, no class pair"""
    m = _person_model(lambda o: o.choice("name_typo", AddTypos("p.name")))
    lw = LoweredModel(m, Query(m, "Obs", {"Typo": ("p.name", "name_typo")}), {"Typo": ["Jim", "Amn"]})
    assert lw.class_pairs == {} and len(lw.pair_id) == 1
    assert lw.block_arrays(0)[0][1]["cacheable"] == 1


# ---- the literal interpreter's densities (oracle/literal.py): strings in, float64 out -------------------------------------
EQUAL, INITIAL, NEITHER = math.log(0.9999), math.log(0.0001), -1000.0


def test_literal_format_name_known_answers():
    f = lit.format_name_logpdf
    assert f("JIM", "jim") == EQUAL and f("j.", "Jim") == INITIAL and f("Tim", "Jim") == NEITHER
    # format_name.jl:49 — the initial form of the one-letter name "J" is "J."; the name "J." observed as "J" is neither
    assert f("J.", "J") == INITIAL
    assert f("J", "J.") == NEITHER
    assert f("j.", "J.") == EQUAL  # (equality is asked first, format_name.jl:47)
    # the empty name: every observation is impossible, the missing one certain (format_name.jl:35-36, 44-46)
    assert f("", "") == NEITHER and f("x", "") == NEITHER and f(".", "") == NEITHER and f(None, "") == 0.0
    # a name holding "*": impossible against a missing observation, an ordinary name against a present one
    assert f(None, "a*b") == -1000.0 and f("A*B", "a*b") == EQUAL and f("a.", "a*b") == INITIAL and f("*.", "*") == INITIAL
    assert f(None, "Jim") == -5.0
    # character-by-character folding: U+0130 lowercases to two characters and stands for itself
    assert f("\u0130x", "\u0130X") == EQUAL and f("i\u0307x", "\u0130x") == NEITHER
    assert f("\u00c9mile", "\u00e9MILE") == EQUAL and f("\u00e9.", "\u00c9mile") == INITIAL
    assert all(isinstance(f(o, n), float) for o, n in [("a", "a"), ("a.", "ab"), ("b", "a"), (None, "a"), (None, ""), ("a", "")])


def test_literal_short_version_known_answers():
    g = lit.expand_on_short_version_logpdf
    opts = ["Sam", "Samuel", "Samantha", "Alan", "sal", "Bob"]
    assert g("Bob", "zz", opts) == -1000.0 and g(None, "zz", opts) == -1000.0      # a short version of no option
    assert g("Bob", "bb", opts) == -math.log(1) and g("Alan", "bb", opts) == -1000.0  # of one
    assert g("Samuel", "sm", opts) == -math.log(3) == g("Samantha", "SM", opts)     # of several, ignoring case
    assert g("Alan", "al", opts) == -math.log(3) and g("Bob", "al", opts) == -1000.0  # (Alan, sal, Samuel)
    assert g("Sam", "Sam", opts) == -math.log(3)
    # a missing observation: string membership of the value among the options, case and all (in(val, options))
    assert g(None, "Sam", opts) == 0.0 and g(None, "sam", opts) == -1000.0 and g(None, "al", opts) == -1000.0
    assert g("Bob", "", opts) == -math.log(6) and g(None, "", opts) == -1000.0      # the empty value fits every option
    assert not lit._is_short_version("ab", "ba") and not lit._is_short_version("jimmy", "jim")
    assert all(isinstance(g(o, v, opts), float) for o, v in [("Bob", "bb"), ("Bob", "zz"), (None, "Sam"), (None, "x")])


def _some_strings(n, seed):
    """strings of the kind test_gpu_tabulated_terms._strings makes (that module is GPU-marked: restated here): lengths
    walking 0, 1, 2, 63, 64, 65, 300 over a small mixed-case alphabet, a few initial forms"""
    rng = np.random.default_rng(seed)
    alpha = "abAB.\u00c9\u00e9*"
    out = []
    for i in range(n):
        L = [0, 1, 2, 63, 64, 65, 300][i % 7]
        if i % 11 == 3:
            out.append("abAB"[int(rng.integers(0, 4))] + ".")
        else:
            out.append("".join(alpha[int(rng.integers(0, len(alpha)))] for _ in range(L)))
    return out


def test_literal_densities_equal_the_table_restatement():
    """two restatements written apart — oracle/literal.py on strings, tabulated_program on (T, class byte) — agree on
    every (observed or missing, latent) pair, exactly"""
    obs = sorted(set(_some_strings(230, 1)))
    lat = _some_strings(240, 2)
    rng = np.random.default_rng(3)
    for j in range(0, len(lat), 4):  # class 0 of both rules, short versions, initials of latent strings, options as values
        o = obs[int(rng.integers(0, len(obs)))]
        lat[j] = (o.swapcase() if j % 8 == 0 else "".join(ch for ch in o if rng.random() < 0.5)) if j % 16 else o
    lat = sorted(set(lat + [""]))
    obs = sorted(set(obs + [v[0] + "." for v in lat[1:40]] + [""]))
    assert len(obs) + len(lat) >= 300
    for L in (0, 1, 2, 63, 64, 65, 300):
        assert any(len(o) == L for o in obs) and any(len(v) == L for v in lat)
    assert any(o != o.lower() and o != o.upper() for o in obs) and any(o.endswith(".") and len(o) == 2 for o in obs)
    seen = {tp.SHORT: set(), tp.FORMAT: set()}
    for rule in (tp.SHORT, tp.FORMAT):
        options = obs if rule == tp.SHORT else None  # (the lowering requires an observed value to be an option)
        T = tp.density_rows(rule, lat, options)
        cls = tp.class_table(rule, obs, lat)
        opts = tuple(obs)
        for v, name in enumerate(lat):
            got = lit.expand_on_short_version_logpdf(None, name, opts) if rule == tp.SHORT else lit.format_name_logpdf(None, name)
            assert got == T[v, 3], (rule, None, name)
            for u, o in enumerate(obs):
                got = lit.expand_on_short_version_logpdf(o, name, opts) if rule == tp.SHORT else lit.format_name_logpdf(o, name)
                assert got == T[v, cls[u, v]], (rule, o, name)
                seen[rule].add(int(cls[u, v]))
        seen[rule].update(("missing", float(x)) for x in T[:, 3])
    assert {0, 1} <= seen[tp.SHORT] and {0, 1, 2} <= seen[tp.FORMAT]
    assert {("missing", 0.0), ("missing", -1000.0)} <= seen[tp.SHORT]
    assert {("missing", 0.0), ("missing", -1000.0), ("missing", -5.0)} <= seen[tp.FORMAT]


def test_engine_density_rows_hold_the_reference_values():
    """class_density_rows (what the engine uploads) against the literal densities on one value of every sort"""
    names = ["", "a*b", "Jim", "J"]
    T = class_density_rows(_lib.CLASS_FORMAT_NAME, names)
    for v, name in enumerate(names):
        seen = {0: name.upper(), 1: name[:1] + ".", 2: "zz"}
        assert [T[v, c] for c in range(3)] == [lit.format_name_logpdf(seen[c], name) for c in range(3)] or name == ""
        assert T[v, 3] == lit.format_name_logpdf(None, name)
    assert list(T[0]) == [-1000.0, -1000.0, -1000.0, 0.0]
    opts = ["Sam", "Samuel", "sal"]
    vals = ["Sam", "sl", "zz"]
    T = class_density_rows(_lib.CLASS_SHORT_VERSION, vals, opts, tp.short_counts(vals, opts))
    assert T[0, 0] == lit.expand_on_short_version_logpdf("Samuel", "Sam", opts) == -math.log(2)
    assert T[1, 0] == lit.expand_on_short_version_logpdf("sal", "sl", opts) == -math.log(2)
    assert T[2, 0] == -1000.0 and (T[:, 1:3] == -1000.0).all()
    assert [T[v, 3] for v in range(3)] == [lit.expand_on_short_version_logpdf(None, s, opts) for s in vals] == [0.0, -1000.0, -1000.0]
