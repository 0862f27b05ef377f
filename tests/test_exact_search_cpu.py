"""The exact-search entry points (cmr_index_search_exact and its kin) are declared, exported and bound, and reject a NULL
index without a device."""
import ctypes as C
import os
import re

import numpy as np

from comorag_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cmr_index_search_exact", "cmr_index_search_exact_pipelined", "cmr_index_round_stats", "cmr_mindex_search_exact")


def test_exact_symbols_declared_and_bound():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "comorag_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cmr_[a-z0-9_]+)\s*\(", txt))
    lib = L.lib()
    for s in NEW:
        assert s in declared, s
        assert s in L.SIGNATURES, s
        assert hasattr(lib, s), s
    assert lib.cmr_abi_version() == 2


def test_exact_search_null_index_is_invalid():
    q = np.zeros((1, 8), np.float32)
    ids = np.zeros((1, 4), np.int64)
    sc = np.zeros((1, 4), np.float32)
    ex = np.zeros(1, np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)        # noqa: E731
    assert L.lib().cmr_index_search_exact(None, p(q), 1, 4, p(ids), p(sc), p(ex)) == L.CMR_ERR_INVALID
    assert L.lib().cmr_mindex_search_exact(None, p(q), 1, 4, p(ids), p(sc), p(ex)) == L.CMR_ERR_INVALID
    a, b = C.c_float(0), C.c_float(0)
    assert L.lib().cmr_index_round_stats(None, C.byref(a), C.byref(b)) == L.CMR_ERR_INVALID
    done = C.c_void_p()
    assert L.lib().cmr_index_search_exact_pipelined(None, None, 1, 4, None, None, None, None, C.byref(done)) == L.CMR_ERR_INVALID
