"""Wave-private hit records of the certified int8 pre-filter on the device: the filter's waves write their hits to areas
of their own ("prefilter_wave_cap" records each, counted by "prefilter_wave_overflow"), q8_bucket_kernel sorts them into the queries'
lists.  Whatever the loop shape, the capacities and the history of the workspace, a pipelined call with "prefilter" = 1 returns, bit for
bit, what "prefilter" = 0 and the synchronous search return."""
import ctypes as C

import numpy as np
import pytest

from tests.prefilter_gpu_helpers import MAX_K, N_BIG, N_MID, N_SMALL, _data, _enqueue, _index, _same_bits

pytestmark = pytest.mark.gpu


def _pipelined(idx, Q, k, prefilter, tighten=1, cap=16384, wave_cap=0):
    idx.set_option("prefilter", prefilter)
    idx.set_option("prefilter_tighten", tighten)
    idx.set_option("prefilter_pair_cap", cap)
    idx.set_option("prefilter_wave_cap", wave_cap)
    done, _, oi, os_ = _enqueue(idx, Q, k)
    idx.sync(done)
    assert idx.query_status() is False
    assert idx.get_option("prefilter_active") == (1 if prefilter else 0)
    return oi.cpu().numpy(), os_.cpu().numpy()


def _reference(idx, Q, k):
    """the unfiltered pipeline's result, checked against the synchronous search"""
    ref = _pipelined(idx, Q, k, 0)
    kk = min(k, len(idx))
    assert _same_bits((ref[0][:, :kk], ref[1][:, :kk]), idx.search(Q, k, with_minmax=False)[:2])
    return ref


def _counters(idx):
    return {name: idx.get_option("prefilter_" + name) for name in ("candidates", "pairs", "pair_overflow", "wave_overflow")}


# ---- loop shapes: d = 768 is three 8-block chunks per panel (an odd chunk count for a wave with one panel, an even one with two),
# d = 128 one 4-block chunk; 1 / 33 / 64 queries are one and two query tiles; 70 rows leave most waves of the grid without a panel
@pytest.mark.parametrize("n", [N_SMALL, N_MID, N_BIG])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("d", [128, 768])
def test_loop_shapes(d, dtype, n):
    X, Q = _data("gauss", n, d)
    idx = _index(X, d, dtype)
    try:
        for nq in (1, 33, 64):
            for k in (1, 20, MAX_K):
                ref = _reference(idx, Q[:nq], k)
                got = _pipelined(idx, Q[:nq], k, 1)
                c = _counters(idx)
                print(f"n={n} d={d} {dtype} nq={nq} k={k}: {c}")
                assert _same_bits(got, ref), (nq, k)
                assert c["pairs"] <= n * nq and c["candidates"] <= n      # (a loose threshold, k = 1, may fill wave areas and lists alike)
    finally:
        idx.close()


# ---- a wave's area fills: the rest of its hits are kept directly
def test_wave_area_overflow():
    d, n, k = 128, N_MID, MAX_K
    X, Q = _data("gauss", n, d)
    idx = _index(X, d, "f16")
    try:
        ref = _reference(idx, Q, k)
        loose = _pipelined(idx, Q, k, 1, tighten=0)
        kept0 = idx.get_option("prefilter_candidates")
        assert _same_bits(loose, ref)
        got = _pipelined(idx, Q, k, 1, wave_cap=64)
        c = _counters(idx)
        print(f"wave_cap=64: {c}, untightened {kept0}")
        assert c["wave_overflow"] > 0
        assert _same_bits(got, ref)
        assert len(np.unique(ref[0])) <= c["candidates"] <= kept0
        got = _pipelined(idx, Q, k, 1)
        c = _counters(idx)
        print(f"default wave_cap: {c}")
        assert c["wave_overflow"] == 0
        assert _same_bits(got, ref)
        assert len(np.unique(ref[0])) <= c["candidates"] <= kept0
    finally:
        idx.close()


# ---- a query's list fills in the bucket step: the rest of its records are kept directly
def test_query_list_overflow_through_the_bucket_step():
    d, n, k = 128, N_MID, 20
    X, Q = _data("gauss", n, d)
    idx = _index(X, d, "f16")
    try:
        ref = _reference(idx, Q, k)
        got = _pipelined(idx, Q, k, 1, cap=32)
        c = _counters(idx)
        print(f"pair_cap=32: {c}")
        assert c["pair_overflow"] > 0
        assert c["pairs"] <= 64 * 32
        assert _same_bits(got, ref)
    finally:
        idx.close()


# ---- the wave counters are never cleared: after a batch with many records, a batch on 70 rows of the same index and workspaces
# (three calls each, so that every slot of the pipeline has held the large batch and then holds the small one)
def test_stale_counts():
    from comorag_amd import _lib as L
    d, nq, k = 128, 64, 20
    X, Q = _data("gauss", N_BIG, d)
    idx = _index(X, d, "bf16")
    try:
        for _ in range(3):
            _pipelined(idx, Q[:nq], MAX_K, 1)
        assert idx.get_option("prefilter_pairs") > N_SMALL * nq
        # int cmr_index_truncate(cmr_index_t*, long long) of cmr_internal.h: a C++ symbol of the library, not part of its C ABI
        truncate = getattr(L.lib(), "_Z18cmr_index_truncateP9cmr_indexx")
        truncate.argtypes, truncate.restype = [C.c_void_p, C.c_longlong], C.c_int
        L.check(truncate(idx._h, N_SMALL))
        assert len(idx) == N_SMALL
        for _ in range(3):
            got = _pipelined(idx, Q[:nq], k, 1)
            c = _counters(idx)
            print(f"after the truncation: {c}")
            assert c["pairs"] <= N_SMALL * nq and c["candidates"] <= N_SMALL and c["wave_overflow"] == 0
            assert got[0].max() < N_SMALL
        ref = _reference(idx, Q[:nq], k)
        assert _same_bits(got, ref)
    finally:
        idx.close()


# ---- padding rows: every score <= 0, so a zero row of the last panel's padding would be a hit, and the best lower bound there is
@pytest.mark.parametrize("n", [N_SMALL, N_MID])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_padding_rows_are_never_recorded(n, dtype):
    d = 128
    X, Q = _data("zeros", n, d)
    idx = _index(X, d, dtype)
    try:
        for k in (20, 64):
            ref = _reference(idx, Q[:33], k)
            got = _pipelined(idx, Q[:33], k, 1)
            c = _counters(idx)
            assert _same_bits(got, ref)
            assert c["candidates"] <= n and c["pairs"] <= n * 33
            assert got[0].max() < n
    finally:
        idx.close()


# ---- modes without records
@pytest.mark.parametrize("n", [N_SMALL, N_MID])
def test_modes_without_records(n):
    d = 128
    X, Q = _data("gauss", n, d)
    idx = _index(X, d, "bf16")
    try:
        ref = _reference(idx, Q[:33], 20)
        got = _pipelined(idx, Q[:33], 20, 2)
        c = _counters(idx)
        assert _same_bits(got, ref)
        assert c["candidates"] == n and c["pairs"] == 0
        got = _pipelined(idx, Q[:33], 20, 1, tighten=0)
        c = _counters(idx)
        assert _same_bits(got, ref)
        assert c["pairs"] == 0 and c["wave_overflow"] == 0
    finally:
        idx.close()
