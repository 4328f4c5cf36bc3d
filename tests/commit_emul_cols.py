"""TEST INFRASTRUCTURE: tests/commit_emul.py for plans whose leaves have several value columns (product leaves).  The host
build gains one entry (tests/commit_host/commit_host_cols.cpp: the leaf's option table column-major with its stride, as
commit.hip passes it on the device); everything else is commit_emul.EmulatedDevice."""
import ctypes as C
import os
import subprocess

import numpy as np

import commit_emul

SRC = os.path.join(commit_emul.HERE, "commit_host", "commit_host_cols.cpp")
LIB = os.path.join(commit_emul.HERE, "commit_host", "libcommit_host_cols.so")
_lib = None


def lib():
    global _lib
    if _lib is None:
        newest = max(os.path.getmtime(p) for p in (SRC, commit_emul.SRC, commit_emul.CORE))
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < newest:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", LIB, SRC])
        _lib = C.CDLL(LIB)
        _lib.pcch_create.restype = C.c_void_p
    return _lib


class EmulatedDeviceCols(commit_emul.EmulatedDevice):
    """with_strides=False leaves the multi-column leaves as commit_emul passes them (no stride): the commit must refuse"""

    def __init__(self, lw, trace, slack=64, with_strides=True):
        # the base class takes its library from commit_emul.lib(): hand it this one (a superset of libcommit_host.so, the same
        # entries) for the time of the construction only — other EmulatedDevices keep the library they always had
        saved, commit_emul._lib = commit_emul._lib, lib()
        try:
            super().__init__(lw, trace, slack=slack)
        finally:
            commit_emul._lib = saved
        if not self.supported or not with_strides:
            return
        for p, bi in enumerate(self.plans):
            for i, info in enumerate(lw.blocks[bi]["node_info"]):
                cols = lw.option_cols.get((info["cls"], info["attr"])) if info["kind"] == "leaf" else None
                if cols is not None:
                    cols = np.ascontiguousarray(cols, dtype=np.int32)
                    self._keep.append(cols)
                    assert self.L.pcch_set_leaf_columns(self.h, p, i, C.c_void_p(cols.ctypes.data), cols.shape[1]) == 0
