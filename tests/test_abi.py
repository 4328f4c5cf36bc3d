"""CPU tests of the boundary: the shared object loads and exports every symbol
declared in include/pclean_hip.h; compute without a GPU fails loudly."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "pclean_hip.h")).read()
    return sorted(set(re.findall(r"\b(pclean_[a-z0-9_]+)\s*\(", src)) - {"pclean_ctx"})


def test_library_exports_every_declared_symbol():
    from pclean_amd import build
    build.build(verbose=False)
    lib = ctypes.CDLL(build.LIB)
    syms = declared_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/pclean_hip.h but not exported"


def test_launch_counters_are_declared_exported_and_named_slot_for_slot():
    """The three launch counters of the debug interface: each is declared with its slot count in the header, exported by
    the library, and bound in pclean_amd._lib with exactly one distinct name per slot."""
    from pclean_amd import _lib, build
    build.build(verbose=False)
    lib = ctypes.CDLL(build.LIB)
    src = open(os.path.join(ROOT, "include", "pclean_hip.h")).read()
    for kind in ("enum", "root", "dist"):
        m = re.search(rf"#define PCLEAN_{kind.upper()}_LAUNCH_SLOTS (\d+)", src)
        assert m, kind
        assert re.search(rf"int pclean_debug_{kind}_launches\(pclean_ctx\* ctx, int64_t\* out, int32_t reset\);", src), kind
        assert hasattr(lib, f"pclean_debug_{kind}_launches"), kind
        names = getattr(_lib.HipContext, f"{kind.upper()}_LAUNCH_SLOTS")
        assert len(names) == len(set(names)) == int(m.group(1)), kind
        assert callable(getattr(_lib.HipContext, f"{kind}_launches"))
        # a NULL context is refused, not dereferenced
        assert getattr(lib, f"pclean_debug_{kind}_launches")(None, None, 0) != 0
    # the table builders: 16 + 2 + 8 + 6 + 1 + 2 instantiations
    d = _lib.HipContext.DIST_LAUNCH_SLOTS
    assert [sum(n.startswith(p) for n in d) for p in ("osa_bitpar", "osa_tile", "dl_seg", "dl_wave", "dl_lds", "dl_pair")] == \
        [16, 2, 8, 6, 1, 2]


def test_memo_counter_is_declared_exported_and_named_slot_for_slot():
    """pclean_debug_memo_stats, the counter of the memo of option-list marginals: declared with its slot count, exported,
    bound with one distinct name per slot, and a NULL context is refused"""
    from pclean_amd import _lib, build
    build.build(verbose=False)
    lib = ctypes.CDLL(build.LIB)
    src = open(os.path.join(ROOT, "include", "pclean_hip.h")).read()
    m = re.search(r"#define PCLEAN_MEMO_STAT_SLOTS (\d+)", src)
    assert m
    assert re.search(r"int pclean_debug_memo_stats\(pclean_ctx\* ctx, int64_t\* out, int32_t reset\);", src)
    assert hasattr(lib, "pclean_debug_memo_stats")
    names = _lib.HipContext.MEMO_STAT_SLOTS
    assert len(names) == len(set(names)) == int(m.group(1)) == 5
    assert names == ("calls", "lookups", "misses", "resets", "stored")
    assert callable(_lib.HipContext.memo_stats)
    assert lib.pclean_debug_memo_stats(None, None, 0) != 0
    out = (ctypes.c_int64 * 5)()
    assert lib.pclean_debug_memo_stats(None, out, 1) != 0


def test_no_cpu_fallback():
    import torch
    from pclean_amd import HipContext, PCleanHipError
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(PCleanHipError):
        HipContext(0)


def test_struct_layouts_match_header():
    from pclean_amd import _lib
    assert ctypes.sizeof(_lib.Term) == 32 == _lib.TERM_DTYPE.itemsize
    assert ctypes.sizeof(_lib.Node) == 48 == _lib.NODE_DTYPE.itemsize
    assert ctypes.sizeof(_lib.InferConfig) == 28
