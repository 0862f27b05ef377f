"""Filtered score-bound searches (cmr_index_search_min_score_masked / _ids, cmr_index_range_count_masked / _ids,
cmr_index_range_search_masked / _ids and the three cmr_mindex_*_ids), host side: the nine symbols are bound, every
argument rule that needs no index answers before the handle is looked at (so it holds on a host without a device), the numpy helpers of
the GPU tests (tests/filtered_range_model.py) against hand-made lists, and `retrieval.neighbours_within` forwarding to the id form."""
import ctypes as C
import os

import numpy as np
import pytest

from comorag_amd import _lib as L
from tests import filtered_range_model as fm

NEW = ("cmr_index_search_min_score_masked", "cmr_index_search_min_score_ids", "cmr_index_range_count_masked", "cmr_index_range_count_ids",
       "cmr_index_range_search_masked", "cmr_index_range_search_ids", "cmr_mindex_search_min_score_ids", "cmr_mindex_range_count_ids",
       "cmr_mindex_range_search_ids")
NAN = float("nan")


def _p(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def test_every_new_symbol_is_bound_and_the_header_says_what_is_filtered():
    lib = L.lib()
    for name in NEW:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.cmr_abi_version() == 2                                  # symbols were only added
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(L.__file__)), "..", "include", "comorag_hip.h")).read()
    for name in NEW:
        assert f"int32_t {name}(" in hdr, name
    assert "Not filtered, as before" not in hdr and "DESIGN.md 4.19" in hdr


# ---- the argument rules on NULL handles.  Every call takes (handle, q, nq, out, b, filter...) below; "words" forms get (words, n_words,
# n_masks), "ids" forms (mode, off, ids, n_ids).  k = 4 and max_total = 0 where the call has them.
def _words_calls():
    lib = L.lib()
    return {
        "cmr_index_search_min_score_masked": lambda h, q, nq, out, b, w, nw, nm, k=4: lib.cmr_index_search_min_score_masked(h, q, nq, k, b, w, nw, nm, out, out),
        "cmr_index_range_count_masked": lambda h, q, nq, out, b, w, nw, nm, k=4: lib.cmr_index_range_count_masked(h, q, nq, b, w, nw, nm, out),
        "cmr_index_range_search_masked": lambda h, q, nq, out, b, w, nw, nm, k=4: lib.cmr_index_range_search_masked(h, q, nq, b, 0, w, nw, nm, out),
    }


def _ids_calls():
    lib = L.lib()
    calls = {}
    for pre in ("cmr_index_", "cmr_mindex_"):
        calls[pre + "search_min_score_ids"] = (lambda f: lambda h, q, nq, out, b, mode, off, ids, n, k=4: f(h, q, nq, k, b, mode, off, ids, n, out, out))(getattr(lib, pre + "search_min_score_ids"))
        calls[pre + "range_count_ids"] = (lambda f: lambda h, q, nq, out, b, mode, off, ids, n, k=4: f(h, q, nq, b, mode, off, ids, n, out))(getattr(lib, pre + "range_count_ids"))
        calls[pre + "range_search_ids"] = (lambda f: lambda h, q, nq, out, b, mode, off, ids, n, k=4: f(h, q, nq, b, 0, mode, off, ids, n, out))(getattr(lib, pre + "range_search_ids"))
    return calls


def test_the_nine_entry_points_are_all_covered_below():
    assert sorted(list(_words_calls()) + list(_ids_calls())) == sorted(NEW)


def test_words_forms_check_their_arguments_before_the_handle():
    lib = L.lib()
    q = np.zeros((2, 8), np.float32)
    out = np.zeros(64, np.int64)          # stands for every output (ids, scores, counts, the result pointer): never written
    w = np.zeros((2, 1), np.uint32)
    for name, call in _words_calls().items():
        def err(*a, **kw):
            assert call(*a, **kw) == L.CMR_ERR_INVALID, name
            return lib.cmr_last_error()
        assert b"NULL index" in err(None, _p(q), 2, _p(out), 0.5, _p(w), 1, 1)              # everything else is in order: shared ...
        assert b"NULL index" in err(None, _p(q), 2, _p(out), 0.5, _p(w), 1, 2)              # ... and per query
        assert b"NULL index" in err(None, _p(q), 2, _p(out), float("-inf"), _p(w), 1, 2)
        assert b"NULL argument" in err(None, None, 2, _p(out), 0.5, _p(w), 1, 1)
        assert b"NULL argument" in err(None, _p(q), 2, None, 0.5, _p(w), 1, 1)
        assert b"NULL allow words" in err(None, _p(q), 2, _p(out), 0.5, None, 1, 1)
        for nm in (0, 3, -1):
            assert b"n_masks" in err(None, _p(q), 2, _p(out), 0.5, _p(w), 1, nm)
        for nq in (0, -2):
            assert b"nq" in err(None, _p(q), nq, _p(out), 0.5, _p(w), 1, 1)
        assert b"n_words" in err(None, _p(q), 2, _p(out), 0.5, _p(w), -1, 1)
        assert b"NaN" in err(None, _p(q), 2, _p(out), NAN, _p(w), 1, 1)
    thr = _words_calls()["cmr_index_search_min_score_masked"]
    assert thr(None, _p(q), 2, _p(out), 0.5, _p(w), 1, 1, k=0) == L.CMR_ERR_INVALID and b"k must" in lib.cmr_last_error()
    assert thr(None, _p(q), 2, _p(out), 0.5, _p(w), 1, 1, k=L.CMR_MAX_K + 1) == L.CMR_ERR_UNSUPPORTED


def test_id_forms_check_their_arguments_before_the_handle():
    lib = L.lib()
    q = np.zeros((2, 8), np.float32)
    out = np.zeros(64, np.int64)
    ids = np.array([3, 1, 4], np.int64)
    off = np.array([0, 1, 3], np.int64)
    for name, call in _ids_calls().items():
        def err(*a, **kw):
            assert call(*a, **kw) == L.CMR_ERR_INVALID, name
            return lib.cmr_last_error()
        assert b"NULL index" in err(None, _p(q), 2, _p(out), 0.5, 0, _p(off), _p(ids), 3)
        assert b"NULL index" in err(None, _p(q), 2, _p(out), 0.5, 1, None, _p(ids), 3)           # a shared list
        assert b"NULL index" in err(None, _p(q), 2, _p(out), 0.5, 0, None, None, 0)              # n_ids == 0 is legal
        assert b"NULL argument" in err(None, None, 2, _p(out), 0.5, 0, _p(off), _p(ids), 3)
        assert b"NULL argument" in err(None, _p(q), 2, None, 0.5, 0, _p(off), _p(ids), 3)
        assert b"NULL ids" in err(None, _p(q), 2, _p(out), 0.5, 0, _p(off), None, 3)
        assert b"n_ids" in err(None, _p(q), 2, _p(out), 0.5, 0, None, _p(ids), -1)
        for mode in (2, -1):
            assert b"mode" in err(None, _p(q), 2, _p(out), 0.5, mode, _p(off), _p(ids), 3)
        assert b"nq" in err(None, _p(q), 0, _p(out), 0.5, 0, None, _p(ids), 3)
        assert b"NaN" in err(None, _p(q), 2, _p(out), NAN, 0, _p(off), _p(ids), 3)
        assert b"id_offsets[0]" in err(None, _p(q), 2, _p(out), 0.5, 0, _p(np.array([1, 1, 3], np.int64)), _p(ids), 3)
        assert b"decrease" in err(None, _p(q), 2, _p(out), 0.5, 0, _p(np.array([0, 4, 3], np.int64)), _p(ids), 3)
        assert b"id_offsets[nq]" in err(None, _p(q), 2, _p(out), 0.5, 0, _p(np.array([0, 1, 2], np.int64)), _p(ids), 3)
        if "search_min_score" in name:
            assert b"k must" in err(None, _p(q), 2, _p(out), 0.5, 0, _p(off), _p(ids), 3, k=0)
            assert call(None, _p(q), 2, _p(out), 0.5, 0, _p(off), _p(ids), 3, k=L.CMR_MAX_K + 1) == L.CMR_ERR_UNSUPPORTED, name


def test_a_refused_range_search_leaves_the_result_pointer_null():
    lib = L.lib()
    q = np.zeros((1, 8), np.float32)
    w = np.zeros(1, np.uint32)
    res = C.c_void_p(12345)
    assert lib.cmr_index_range_search_masked(None, _p(q), 1, 0.5, 0, _p(w), 1, 1, C.byref(res)) == L.CMR_ERR_INVALID and not res.value
    res = C.c_void_p(12345)
    assert lib.cmr_index_range_search_ids(None, _p(q), 1, 0.5, 0, 0, None, None, 0, C.byref(res)) == L.CMR_ERR_INVALID and not res.value
    res = C.c_void_p(12345)
    assert lib.cmr_mindex_range_search_ids(None, _p(q), 1, 0.5, 0, 0, None, None, 0, C.byref(res)) == L.CMR_ERR_INVALID and not res.value


# ---- the helpers against hand-made lists
def test_rows_of_and_words_of():
    assert fm.rows_of(np.array([0xFFFFFFFF, 0xFFFFFFFF], np.uint32), 40).tolist() == list(range(40))          # garbage beyond n does not count
    assert fm.rows_of(np.array([0xAAAAAAAA], np.uint32), 7).tolist() == [1, 3, 5]
    assert fm.rows_of(np.zeros(0, np.uint32), 0).tolist() == []
    assert fm.words_of(40, [0, 31, 32, 39]).tolist() == [0x80000001, 0x81]
    assert fm.rows_of(fm.words_of(40, [0, 31, 32, 39]), 40).tolist() == [0, 31, 32, 39]


def test_the_mask_family():
    n, tied = 5003, [31, 700, 2501, 5002]
    M = fm.family(n, tied)
    assert M.shape == (8, 157) and M.dtype == np.uint32
    assert fm.rows_of(M[0], n).tolist() == list(range(n)) and M[0][-1] == 0xFFFFFFFF          # 11 live bits, 21 of garbage
    assert fm.rows_of(M[1], n).size == 0
    assert fm.rows_of(M[2], n).tolist() == list(range(1, n, 2))
    assert fm.rows_of(M[3], n).tolist() == [700]
    assert fm.rows_of(M[4], n).tolist() == list(range(2040, 2060)) + list(range(4090, 4100))
    assert 2300 < fm.rows_of(M[5], n).size < 2700 and 20 < fm.rows_of(M[6], n).size < 90
    assert fm.rows_of(M[7], n).tolist() == [r for r in range(n) if r != 2501]
    P = fm.per_query(M, 10)
    assert P.shape == (10, 157) and all(np.array_equal(P[i], M[i % 7]) for i in range(10))
    S = fm.small_family(33)
    assert S.shape == (5, 2) and fm.rows_of(S[3], 33).tolist() == [32] and fm.small_family(0).shape == (5, 0)


def test_drop_against_hand_made_lists():
    lims = np.array([0, 3, 3, 7], np.int64)
    ids = np.array([5, 2, 9, 9, 2, 5, 1], np.int64)
    sc = np.array([0.9, 0.5, -0.0, 0.9, 0.9, 0.25, 0.0], np.float32)
    got = fm.drop((lims, ids, sc), np.array([2, 9, 1], np.int64))
    assert got[0].tolist() == [0, 2, 2, 5] and got[1].tolist() == [2, 9, 9, 2, 1]
    assert got[2].view(np.uint32).tolist() == np.array([0.5, -0.0, 0.9, 0.9, 0.0], np.float32).view(np.uint32).tolist()      # the -0.0 keeps its sign
    got = fm.drop((lims, ids, sc), [np.array([5]), np.array([5]), np.empty(0, np.int64)])
    assert got[0].tolist() == [0, 1, 1, 1] and got[1].tolist() == [5] and got[2].tolist() == [np.float32(0.9)]
    got = fm.drop((lims, ids, sc), np.empty(0, np.int64))
    assert got[0].tolist() == [0, 0, 0, 0] and got[1].dtype == np.int64 and got[2].dtype == np.float32 and got[1].size == 0
    with pytest.raises(AssertionError):
        fm.drop((lims, ids, sc), [np.array([5])])


def test_pad_below_against_hand_made_rows():
    ids = np.array([[4, 8, 1], [7, -1, -1]], np.int64)
    sc = np.array([[0.9, 0.5, 0.25], [0.5, -np.inf, -np.inf]], np.float32)
    i, s = fm.pad_below(ids, sc, 0.5, 5)
    assert i.tolist() == [[4, 8, -1, -1, -1], [7, -1, -1, -1, -1]]
    assert s.tolist() == [[np.float32(0.9), 0.5, -np.inf, -np.inf, -np.inf], [0.5, -np.inf, -np.inf, -np.inf, -np.inf]]
    i, s = fm.pad_below(ids, sc, float("-inf"), 3)
    assert i.tolist() == ids.tolist() and s.tolist() == sc.tolist()
    i, s = fm.pad_below(ids, sc, float("inf"), 3)
    assert (i == -1).all() and np.isneginf(s).all()
    i, s = fm.pad_below(np.empty((2, 0), np.int64), np.empty((2, 0), np.float32), 0.0, 2)
    assert i.tolist() == [[-1, -1], [-1, -1]]
    z = np.array([[0.0, -0.0]], np.float32)
    i, s = fm.pad_below(np.array([[3, 6]]), z, 0.0, 2)
    assert i.tolist() == [[3, 6]] and np.signbit(s).tolist() == [[False, True]]          # -0.0 attains a bound of +0.0 and keeps its bits


# ---- neighbours_within forwards to the id form
class _StandIn:
    """numpy stand-in for an index of 6 rows whose scores are given: records which call it got"""

    def __init__(self, S):
        self.S = np.asarray(S, np.float32)
        self.calls = []

    def _lists(self, nq, b, rows):
        lims, ids, sc = [0], [], []
        for i in range(nq):
            r = np.array([j for j in rows[i] if self.S[i, j] >= np.float32(b)], np.int64)
            r = r[np.lexsort((r, -self.S[i, r]))] if len(r) else r
            ids.append(r); sc.append(self.S[i, r]); lims.append(lims[-1] + len(r))
        return np.array(lims, np.int64), np.concatenate(ids).astype(np.int64), np.concatenate(sc).astype(np.float32)

    def range_search(self, q, b):
        self.calls.append(("range_search", None, None))
        return self._lists(len(q), b, [range(self.S.shape[1])] * len(q))

    def range_search_filtered_ids(self, q, b, *, allow=None, exclude=None):
        self.calls.append(("range_search_filtered_ids", allow, exclude))
        n = self.S.shape[1]
        rows = [[j for j in range(n) if (j in allow if allow is not None else j not in exclude)]] * len(q)
        return self._lists(len(q), b, rows)


def test_neighbours_within_forwards_the_id_lists():
    from comorag_amd.retrieval import neighbours_within
    S = [[0.9, 0.1, 0.5, 0.5, 0.7, 0.2], [0.3, 0.8, 0.5, 0.0, 0.5, 0.6]]
    Q = np.zeros((2, 4), np.float32)
    idx = _StandIn(S)
    plain = neighbours_within(idx, Q, 0.5)
    assert idx.calls == [("range_search", None, None)]
    assert [p[0].tolist() for p in plain] == [[0, 4, 2, 3], [1, 5, 2, 4]]
    ex = neighbours_within(idx, Q, 0.5, exclude_ids=[4, 2])
    assert idx.calls[-1] == ("range_search_filtered_ids", None, [4, 2])
    assert [p[0].tolist() for p in ex] == [[0, 3], [1, 5]] and ex[0][1].tolist() == [np.float32(0.9), 0.5]
    al = neighbours_within(idx, Q, 0.5, allow_ids=[2, 4, 5])
    assert idx.calls[-1] == ("range_search_filtered_ids", [2, 4, 5], None)
    assert [p[0].tolist() for p in al] == [[4, 2], [5, 2, 4]]
    assert len(idx.calls) == 3
