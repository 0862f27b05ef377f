"""No device: cmr_range_merge (the host merge of per-shard range-search lists) against a numpy lexsort on hand-made shard lists, and the
argument checks of every range entry point, which return CMR_ERR_INVALID before any device call."""
import ctypes as C

import numpy as np
import pytest

from comorag_amd import _lib as L


def _ptr_array(arrays, ctype):
    return (C.POINTER(ctype) * len(arrays))(*[a.ctypes.data_as(C.POINTER(ctype)) for a in arrays])


def _merge(shards, nq):
    """shards: per shard (lims [nq + 1], ids, scores) -> merged (lims, ids, scores)"""
    lims = [np.ascontiguousarray(s[0], np.int64) for s in shards]
    ids = [np.ascontiguousarray(s[1], np.int64) for s in shards]
    sc = [np.ascontiguousarray(s[2], np.float32) for s in shards]
    total = sum(int(l[nq]) for l in lims)
    out_lims = np.full(nq + 1, -7, np.int64)
    out_ids = np.full(max(total, 1), -7, np.int64)
    out_sc = np.full(max(total, 1), 7.0, np.float32)
    L.check(L.lib().cmr_range_merge(len(shards), nq, _ptr_array(lims, C.c_int64), _ptr_array(ids, C.c_int64), _ptr_array(sc, C.c_float),
                                    out_lims.ctypes.data, out_ids.ctypes.data, out_sc.ctypes.data))
    return out_lims, out_ids[:total], out_sc[:total]


def _reference(shards, nq):
    lims, ids, sc = [0], [], []
    for i in range(nq):
        qi = np.concatenate([s[1][s[0][i]:s[0][i + 1]] for s in shards]).astype(np.int64)
        qs = np.concatenate([s[2][s[0][i]:s[0][i + 1]] for s in shards]).astype(np.float32)
        order = np.lexsort((qi, -qs))
        ids.append(qi[order]); sc.append(qs[order]); lims.append(lims[-1] + len(order))
    return np.array(lims, np.int64), np.concatenate(ids), np.concatenate(sc)


def _shard_lists(rng, nq, rows, empty_queries=(), values=None):
    """one shard's lists over its global ids `rows`: per query a random subset with scores from a small set of values (ties across and
    inside shards), sorted in the exported order"""
    values = np.array([0.9, 0.5, 0.5, 0.25, 0.0, -0.0, -0.75], np.float32) if values is None else values
    lims, ids, sc = [0], [], []
    for i in range(nq):
        take = np.empty(0, np.int64) if i in empty_queries or len(rows) == 0 else np.sort(rng.choice(rows, size=rng.integers(0, len(rows) + 1), replace=False))
        s = rng.choice(values, size=len(take)).astype(np.float32)
        order = np.lexsort((take, -s))
        ids.append(take[order].astype(np.int64)); sc.append(s[order]); lims.append(lims[-1] + len(take))
    return np.array(lims, np.int64), np.concatenate(ids) if ids else np.empty(0, np.int64), np.concatenate(sc) if sc else np.empty(0, np.float32)


def _same(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32))


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("n_shards", [1, 2, 4])
def test_merge_equals_lexsort(n_shards, nq):
    rng = np.random.default_rng(100 * n_shards + nq)
    # interleaved id runs (what block tables give): shard s holds the ids of blocks s, s + S, ...
    blocks = np.arange(64).reshape(8, 8)
    shards = []
    for s in range(n_shards):
        rows = blocks[s::n_shards].reshape(-1) if s != 1 else np.empty(0, np.int64)      # shard 1: an empty shard
        shards.append(_shard_lists(rng, nq, rows, empty_queries=(nq - 1,) if s == 0 else ()))
    got = _merge(shards, nq)
    _same(got, _reference(shards, nq))
    assert got[0][0] == 0 and got[0][-1] == sum(s[0][-1] for s in shards)
    if n_shards >= 2:
        assert shards[1][0].tolist() == [0] * (nq + 1)
    if n_shards == 4:      # not vacuous: ties across shards, both zeros present, and a query one shard leaves empty
        last = got[2][got[0][-2]:]
        assert np.any(np.diff(got[2]) == 0) and np.signbit(got[2][got[2] == 0]).any() and not np.signbit(got[2][got[2] == 0]).all()
        assert len(last) > 0 and shards[0][0][nq] == shards[0][0][nq - 1]


def test_merge_ties_across_shards_go_by_id_and_zeros_are_one_value():
    nz = np.float32(-0.0)
    a = (np.int64([0, 3]), np.int64([10, 2, 30]), np.float32([0.5, 0.0, nz]))
    b = (np.int64([0, 4]), np.int64([5, 11, 7, 20]), np.float32([0.5, 0.5, nz, 0.0]))
    lims, ids, sc = _merge([a, b], 1)
    assert lims.tolist() == [0, 7] and ids.tolist() == [5, 10, 11, 2, 7, 20, 30]
    assert np.signbit(sc).tolist() == [False, False, False, False, True, False, True]      # every score keeps its bits
    # all queries empty everywhere: NULL lists are fine then
    z = np.zeros(3, np.int64)
    out = np.full(3, -1, np.int64)
    lp = _ptr_array([z, z], C.c_int64)
    null_i = (C.POINTER(C.c_int64) * 2)()
    null_f = (C.POINTER(C.c_float) * 2)()
    assert L.lib().cmr_range_merge(2, 2, lp, null_i, null_f, out.ctypes.data, None, None) == L.CMR_OK and out.tolist() == [0, 0, 0]


def test_argument_checks_need_no_device():
    lib = L.lib()
    q = np.zeros((2, 8), np.float32)
    cnt = np.zeros(2, np.int64)
    res = C.c_void_p(0x1234)
    fake = C.c_void_p(8)      # never dereferenced: the checks below fail before the handle is touched
    nan = float("nan")
    for prefix in ("cmr_index_", "cmr_mindex_"):
        count, search = getattr(lib, prefix + "range_count"), getattr(lib, prefix + "range_search")
        assert count(None, q.ctypes.data, 2, 0.5, cnt.ctypes.data) == L.CMR_ERR_INVALID
        assert count(fake, None, 2, 0.5, cnt.ctypes.data) == L.CMR_ERR_INVALID
        assert count(fake, q.ctypes.data, 2, 0.5, None) == L.CMR_ERR_INVALID
        assert count(fake, q.ctypes.data, 0, 0.5, cnt.ctypes.data) == L.CMR_ERR_INVALID
        assert count(fake, q.ctypes.data, 2, nan, cnt.ctypes.data) == L.CMR_ERR_INVALID
        assert b"NaN" in lib.cmr_last_error()
        for args in ((None, q.ctypes.data, 2, 0.5, 0), (fake, None, 2, 0.5, 0), (fake, q.ctypes.data, 0, 0.5, 0), (fake, q.ctypes.data, -3, 0.5, 0),
                     (fake, q.ctypes.data, 2, nan, 0)):
            res.value = 0x1234
            assert search(*args, C.byref(res)) == L.CMR_ERR_INVALID, (prefix, args)
            assert res.value is None, "*out must be NULL after a refused call"
        assert search(fake, q.ctypes.data, 2, 0.5, 0, None) == L.CMR_ERR_INVALID
    dev = lib.cmr_index_range_count_dev
    assert dev(None, fake, 2, 0.5, fake, None) == L.CMR_ERR_INVALID and dev(fake, None, 2, 0.5, fake, None) == L.CMR_ERR_INVALID
    assert dev(fake, fake, 2, 0.5, None, None) == L.CMR_ERR_INVALID and dev(fake, fake, 0, 0.5, fake, None) == L.CMR_ERR_INVALID
    assert dev(fake, fake, 2, nan, fake, None) == L.CMR_ERR_INVALID
    assert lib.cmr_range_result_view(None, None, None, None, None) == L.CMR_ERR_INVALID
    assert lib.cmr_range_result_destroy(None) == L.CMR_OK      # NULL is a no-op
    z = np.zeros(2, np.int64)
    lp, ip, fp = _ptr_array([z], C.c_int64), _ptr_array([z], C.c_int64), _ptr_array([np.zeros(1, np.float32)], C.c_float)
    out = np.zeros(2, np.int64)
    assert lib.cmr_range_merge(0, 1, lp, ip, fp, out.ctypes.data, None, None) == L.CMR_ERR_INVALID
    assert lib.cmr_range_merge(1, 0, lp, ip, fp, out.ctypes.data, None, None) == L.CMR_ERR_INVALID
    assert lib.cmr_range_merge(1, 1, None, ip, fp, out.ctypes.data, None, None) == L.CMR_ERR_INVALID
    assert lib.cmr_range_merge(1, 1, lp, ip, fp, None, None, None) == L.CMR_ERR_INVALID
    one = np.int64([0, 1])
    assert lib.cmr_range_merge(1, 1, _ptr_array([one], C.c_int64), ip, fp, out.ctypes.data, None, None) == L.CMR_ERR_INVALID      # hits but no output


def test_binding_constants_match_the_header():
    import os
    import re
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "comorag_hip.h")).read()
    assert int(re.search(r"#define CMR_ROUTE_RANGE (\d+)", txt).group(1)) == L.CMR_ROUTE_RANGE == 11
    assert int(re.search(r"#define CMR_RANGE_TILE (\d+)", txt).group(1)) == L.CMR_RANGE_TILE == 2048
    assert int(re.search(r"#define CMR_RANGE_MAX_TOTAL (\d+)ll", txt).group(1)) == L.CMR_RANGE_MAX_TOTAL == 2 ** 31 - 1
