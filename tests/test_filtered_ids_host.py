"""Filtered search from row-id lists (cmr_index_search_ids*, cmr_index_row_masks_dev, cmr_mindex_search_ids), host
side: the symbols are bound, every argument check comes before any device call (so it holds on a CPU-only host), the list marshaller
`pack_id_lists` against hand-written CSR, and the numpy model of the id translation (tests/filtered_ids_model.py, the GPU tests'
oracle for based and blocked indexes) against `pack_row_masks` on hand-written local rows."""
import ctypes as C
import os

import numpy as np
import pytest

from comorag_amd import _lib as L
from comorag_amd.index import pack_id_lists, pack_row_mask, pack_row_masks
from tests import filtered_ids_model as M

NEW = ("cmr_index_row_masks_dev", "cmr_index_search_ids", "cmr_index_search_ids_dev", "cmr_mindex_search_ids")


def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_every_new_symbol_is_bound():
    lib = L.lib()
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert (L.CMR_IDS_EXCLUDE, L.CMR_IDS_ALLOW) == (0, 1)
    assert lib.cmr_abi_version() == 2                                  # symbols were only added
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "..", "include", "comorag_hip.h")).read()
    assert "#define CMR_ROUTE_FILTERED_IDS (1 << 14)" in hdr
    assert "#define CMR_IDS_EXCLUDE 0" in hdr and "#define CMR_IDS_ALLOW   1" in hdr


def _host_calls():
    """(name, call(handle, q, nq, k, mode, off, ids, n_ids, out_ids, out_sc)) of the two host forms"""
    lib = L.lib()
    return [("cmr_index_search_ids", lambda h, q, nq, k, mode, off, ids, n, oi, os_: lib.cmr_index_search_ids(h, q, nq, k, mode, off, ids, n, oi, os_, None, None)),
            ("cmr_mindex_search_ids", lambda h, q, nq, k, mode, off, ids, n, oi, os_: lib.cmr_mindex_search_ids(h, q, nq, k, mode, off, ids, n, oi, os_, None, None))]


def test_argument_checks_come_before_any_device_call():
    """No handle exists on a CPU-only host, so every call below carries a NULL one — and the message says WHICH check answered: the
    checks of the list come first and need neither an index nor a device; well-formed arguments get as far as the handle."""
    lib = L.lib()
    q = np.zeros((2, 8), np.float32)
    oi = np.zeros((2, 4), np.int64)
    os_ = np.zeros((2, 4), np.float32)
    ids = np.array([3, 1, 4], np.int64)
    off = np.array([0, 1, 3], np.int64)
    for name, call in _host_calls():
        def err(*a):
            assert call(*a) == L.CMR_ERR_INVALID, name
            return lib.cmr_last_error()
        assert b"NULL index" in err(None, _p(q), 2, 4, 0, _p(off), _p(ids), 3, _p(oi), _p(os_))          # everything else is in order
        assert b"NULL index" in err(None, _p(q), 2, 4, 1, None, _p(ids), 3, _p(oi), _p(os_))            # a shared list
        assert b"NULL index" in err(None, _p(q), 2, 4, 0, None, None, 0, _p(oi), _p(os_))               # n_ids == 0 is legal
        assert b"NULL argument" in err(None, None, 2, 4, 0, _p(off), _p(ids), 3, _p(oi), _p(os_))
        assert b"NULL argument" in err(None, _p(q), 2, 4, 0, _p(off), _p(ids), 3, None, _p(os_))
        assert b"NULL argument" in err(None, _p(q), 2, 4, 0, _p(off), _p(ids), 3, _p(oi), None)
        assert b"NULL ids" in err(None, _p(q), 2, 4, 0, _p(off), None, 3, _p(oi), _p(os_))
        assert b"n_ids" in err(None, _p(q), 2, 4, 0, None, _p(ids), -1, _p(oi), _p(os_))
        for mode in (2, -1):
            assert b"mode" in err(None, _p(q), 2, 4, mode, _p(off), _p(ids), 3, _p(oi), _p(os_))
        assert b"nq" in err(None, _p(q), 0, 4, 0, None, _p(ids), 3, _p(oi), _p(os_))
        assert b"k must" in err(None, _p(q), 2, 0, 0, _p(off), _p(ids), 3, _p(oi), _p(os_))
        # bad offsets: not starting at 0, decreasing, a last entry that is not n_ids
        assert b"id_offsets[0]" in err(None, _p(q), 2, 4, 0, _p(np.array([1, 1, 3], np.int64)), _p(ids), 3, _p(oi), _p(os_))
        assert b"decrease" in err(None, _p(q), 2, 4, 0, _p(np.array([0, 4, 3], np.int64)), _p(ids), 3, _p(oi), _p(os_))
        assert b"id_offsets[nq]" in err(None, _p(q), 2, 4, 0, _p(np.array([0, 1, 2], np.int64)), _p(ids), 3, _p(oi), _p(os_))
        assert b"id_offsets[nq]" in err(None, _p(q), 2, 4, 0, _p(np.array([0, 1, 4], np.int64)), _p(ids), 3, _p(oi), _p(os_))
        # k beyond CMR_MAX_K is refused as unsupported, again before the handle is looked at
        assert call(None, _p(q), 2, L.CMR_MAX_K + 1, 0, _p(off), _p(ids), 3, _p(oi), _p(os_)) == L.CMR_ERR_UNSUPPORTED, name


def test_device_forms_check_their_arguments_without_a_device():
    lib = L.lib()
    a = np.zeros(8, np.int64)          # stands for device pointers: never dereferenced, the checks answer first
    w = np.zeros(8, np.uint32)
    f = np.zeros(8, np.float32)
    build, search = lib.cmr_index_row_masks_dev, lib.cmr_index_search_ids_dev
    assert build(None, 0, 1, None, _p(a), 3, _p(w), 1, None) == L.CMR_ERR_INVALID and b"NULL index" in lib.cmr_last_error()
    assert build(None, 0, 1, None, _p(a), 3, None, 1, None) == L.CMR_ERR_INVALID and b"NULL argument" in lib.cmr_last_error()
    assert build(None, 2, 1, None, _p(a), 3, _p(w), 1, None) == L.CMR_ERR_INVALID and b"mode" in lib.cmr_last_error()
    assert build(None, 0, 0, None, _p(a), 3, _p(w), 1, None) == L.CMR_ERR_INVALID and b"nq" in lib.cmr_last_error()
    assert build(None, 0, 1, None, None, 3, _p(w), 1, None) == L.CMR_ERR_INVALID and b"NULL ids" in lib.cmr_last_error()
    assert build(None, 0, 1, None, _p(a), -2, _p(w), 1, None) == L.CMR_ERR_INVALID and b"n_ids" in lib.cmr_last_error()
    assert search(None, _p(f), 1, 4, 0, None, _p(a), 3, _p(a), _p(f), None, None, None) == L.CMR_ERR_INVALID and b"NULL index" in lib.cmr_last_error()
    assert search(None, None, 1, 4, 0, None, _p(a), 3, _p(a), _p(f), None, None, None) == L.CMR_ERR_INVALID and b"NULL argument" in lib.cmr_last_error()
    assert search(None, _p(f), 1, 4, 0, None, _p(a), 3, None, _p(f), None, None, None) == L.CMR_ERR_INVALID
    assert search(None, _p(f), 1, 4, 3, None, _p(a), 3, _p(a), _p(f), None, None, None) == L.CMR_ERR_INVALID and b"mode" in lib.cmr_last_error()
    assert search(None, _p(f), 1, 0, 0, None, _p(a), 3, _p(a), _p(f), None, None, None) == L.CMR_ERR_INVALID and b"k must" in lib.cmr_last_error()
    assert search(None, _p(f), 1, 129, 0, None, _p(a), 3, _p(a), _p(f), None, None, None) == L.CMR_ERR_UNSUPPORTED


# ---- the list marshaller against hand-written CSR
def _same(got, off, ids):
    assert got[1].dtype == np.int64 and got[1].ndim == 1 and got[1].tolist() == ids
    if off is None:
        assert got[0] is None
    else:
        assert got[0].dtype == np.int64 and got[0].flags["C_CONTIGUOUS"] and got[0].tolist() == off


def test_a_shared_list():
    _same(pack_id_lists(exclude=[7, 3, 3, -1]), None, [7, 3, 3, -1])
    _same(pack_id_lists(allow=(5, 6)), None, [5, 6])
    _same(pack_id_lists(allow=np.array([9, 2], np.int32)), None, [9, 2])
    _same(pack_id_lists(exclude=np.array([], np.int64)), None, [])
    _same(pack_id_lists(exclude=[]), None, [])
    _same(pack_id_lists(exclude=[np.int64(4), 5]), None, [4, 5])


def test_per_query_lists_with_empty_entries():
    _same(pack_id_lists(exclude=[[1, 2], [], [5]]), [0, 2, 2, 3], [1, 2, 5])
    _same(pack_id_lists(allow=[[], []]), [0, 0, 0], [])
    _same(pack_id_lists(allow=[[]]), [0, 0], [])
    _same(pack_id_lists(allow=[np.array([4, 4]), (), [0], np.array([], np.int64)]), [0, 2, 2, 3, 3], [4, 4, 0])
    # a 2-d integer array is one row per query: the -1 padded ids of an earlier search go back in as they are
    _same(pack_id_lists(exclude=np.array([[8, 2, -1], [5, -1, -1]])), [0, 3, 6], [8, 2, -1, 5, -1, -1])
    _same(pack_id_lists(exclude=np.zeros((2, 0), np.int64)), [0, 0, 0], [])


def test_marshaller_errors():
    for bad in (dict(), dict(allow=[1], exclude=[2]), dict(allow=3), dict(allow="12"), dict(allow=[0.5]), dict(allow=[[0.5]]),
                dict(allow=[1, [2]]), dict(allow=[[1], 2]), dict(exclude=np.array([0.5])), dict(exclude=np.zeros((1, 1, 1), np.int64)),
                dict(allow=[[[1]]]), dict(allow=[True, False]), dict(allow=np.array([True])), dict(allow=[["a"]]), dict(allow=iter([1]))):
        with pytest.raises(ValueError):
            pack_id_lists(**bad)


# ---- the model of the translation against pack_row_masks on hand-written local rows
def test_model_plain_and_id_base():
    n = 40
    ids = [0, 31, 32, 39, 39, -1, 40, 1000, -7]
    assert M.local_rows(ids, n).tolist() == [0, 31, 32, 39, 39]
    assert np.array_equal(M.words_of(n, 1, "exclude", None, ids), pack_row_mask(n, exclude=[0, 31, 32, 39]))
    assert np.array_equal(M.words_of(n, 1, "allow", None, ids), pack_row_mask(n, allow=[0, 31, 32, 39]))
    base = 1_000_000
    based = [base, base + 39, base - 1, base + 40, 5, -1, base + 7]
    assert M.local_rows(based, n, base=base).tolist() == [0, 39, 7]
    off = [0, 3, 3, 7]
    want = pack_row_masks(n, exclude=[[0, 39], [], [7]])
    assert np.array_equal(M.words_of(n, 3, "exclude", off, based, base=base), want)
    want = pack_row_masks(n, allow=[[0, 39], [], [7]])
    assert np.array_equal(M.words_of(n, 3, "allow", off, based, base=base), want)
    assert want[1].tolist() == [0, 0] and pack_row_masks(n, exclude=[[]])[0].tolist() == [0xFFFFFFFF, 0xFF]          # tail bits zero


def test_model_three_blocks_with_gaps():
    """local rows 0..9 are ids 100..109, 10..29 are 500..519, 30..36 are 9000..9006; everything else is not held"""
    n, blocks = 37, ([0, 10, 30], [100, 500, 9000])
    held = {100: 0, 109: 9, 500: 10, 519: 29, 9000: 30, 9006: 36}
    gaps = [0, 99, 110, 499, 520, 8999, 9007, 10 ** 12, -1, -100]          # below the first block, between blocks, beyond the last
    for g, r in held.items():
        assert M.local_rows([g], n, blocks=blocks).tolist() == [r]
    assert M.local_rows(gaps, n, blocks=blocks).size == 0
    ids = [109, 110, 500, 9006, 9007, -1, 519, 99]
    off = [0, 4, 8]
    assert np.array_equal(M.words_of(n, 2, "exclude", off, ids, blocks=blocks), pack_row_masks(n, exclude=[[9, 10, 36], [29]]))
    assert np.array_equal(M.words_of(n, 2, "allow", off, ids, blocks=blocks), pack_row_masks(n, allow=[[9, 10, 36], [29]]))
    assert np.array_equal(M.words_of(n, 1, "allow", None, gaps, blocks=blocks), pack_row_mask(n, allow=[]))
    # a last block that starts at or beyond the rows held so far names no row
    assert M.local_rows([9000], 30, blocks=blocks).size == 0 and M.local_rows([519], 30, blocks=blocks).tolist() == [29]
