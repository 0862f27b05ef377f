"""Threshold tightening of the certified int8 pre-filter on the device: with "prefilter" = 1 a pipelined call returns,
bit for bit, the same ids and scores whether "prefilter_tighten" is 1 or 0, and the same as "prefilter" = 0 and the synchronous
search — while the tightened pass hands the re-score fewer rows, never fewer than the results need and never fewer than the numpy
model (tests/prefilter_tighten_model.py) counts.  The model's threshold per query is the k-th largest lower bound over ALL rows — the
device selects among the pairs it stored, a subset — or the query's k-th best score where that is larger: the device's threshold is the
larger of its selection and the sampling threshold, and a sampling threshold is the k-th best score of a sample, never above the k-th
best of all rows (with wide bounds, the spike family, it does lie above every lower bound)."""
import functools

import numpy as np
import pytest

from tests import prefilter_model as pm
from tests import prefilter_tighten_model as tm
from tests import value_domain_inputs as vd
from tests.prefilter_gpu_helpers import BATCHES, MAX_K, N_BIG, N_MID, N_SMALL, _data, _enqueue, _index, _same_bits

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=2)
def _model_parts(family, n, d, dtype, seed=0):
    """what the model needs of the stored rows and all 64 queries, independent of the device's max ||x||: row scales and error norms,
    the queries' int8 parts and the integer sums [n, 64]"""
    X, Q = _data(family, n, d, seed)
    Xt, Qt = vd.ROUND[dtype](X), vd.ROUND[dtype](Q)
    a_r, m, b_r, nx = pm.quantise_rows(Xt)
    parts = [pm.quantise_query(Qt[j], 1.0, (d + 127) // 128 * 128)[1:3] for j in range(len(Qt))]
    hi = np.stack([p[0] for p in parts]).astype(np.float32)
    lo = np.stack([p[1] for p in parts]).astype(np.float32)
    mf = m.astype(np.float32)
    return a_r, b_r, mf @ hi.T, mf @ lo.T, Qt


def _model_count(family, n, d, dtype, nq, k, idx, ref, seed=0, queries=None):
    """rows the tightening must at least keep: the union over the queries of the rows with ub >= max(the k-th largest lb over all rows,
    the k-th best score); `ref`: the batch's result (its column k - 1 is the k-th best score), `queries`: the batch's rows of Q"""
    a_r, b_r, I_hi, I_lo, Qt = _model_parts(family, n, d, dtype, seed)
    Mx = idx.prefilter_stats()[0]
    keep = np.zeros(n, bool)
    for i, j in enumerate(range(nq) if queries is None else queries):
        a_q, _, _, B_q, c_q = pm.quantise_query(Qt[j], Mx, (d + 127) // 128 * 128)
        ub, lb = tm.bounds(a_r, b_r, I_hi[:, j], I_lo[:, j], a_q, B_q, c_q)
        tau = tm.kth_largest(lb, k)
        if tau is not None:
            tau = max(tau, ref[1][i, k - 1])
        keep |= tm.standing(ub, tau)
    return int(keep.sum())


def _pipelined(idx, Q, k, prefilter, tighten=1, cap=16384):
    idx.set_option("prefilter", prefilter)
    idx.set_option("prefilter_tighten", tighten)
    idx.set_option("prefilter_pair_cap", cap)
    done, _, oi, os_ = _enqueue(idx, Q, k)
    idx.sync(done)
    assert idx.query_status() is False
    assert idx.get_option("prefilter_active") == (1 if prefilter else 0)
    return oi.cpu().numpy(), os_.cpu().numpy()


def _check(idx, Q, k):
    """tightened and untightened pre-filter against the unfiltered pipeline and the synchronous search; returns (rows re-scored with
    the tightening, without it, the reference result)"""
    n = len(idx)
    ref = _pipelined(idx, Q, k, 0)
    sync = idx.search(Q, k, with_minmax=False)[:2]
    kk = min(k, n)
    assert _same_bits((ref[0][:, :kk], ref[1][:, :kk]), sync)
    loose = _pipelined(idx, Q, k, 1, tighten=0)
    kept0 = idx.get_option("prefilter_candidates")
    assert idx.get_option("prefilter_pairs") == 0 and idx.get_option("prefilter_pair_overflow") == 0
    assert _same_bits(loose, ref), "prefilter_tighten=0 differs from prefilter=0"
    tight = _pipelined(idx, Q, k, 1, tighten=1)
    kept1 = idx.get_option("prefilter_candidates")
    assert _same_bits(tight, ref), "prefilter_tighten=1 differs from prefilter=0"
    distinct = len(np.unique(ref[0][ref[0] >= 0]))
    assert distinct <= kept1 <= kept0 <= n, (distinct, kept1, kept0, n)
    return kept1, kept0, ref


# ---- every shape: d = 128 mostly, 768 once per size; bf16 / f16; the three corpus sizes, the three batches
SHAPES = [(128, "bf16", N_SMALL), (128, "f16", N_SMALL), (768, "bf16", N_SMALL),
          (128, "bf16", N_MID), (128, "f16", N_MID), (768, "f16", N_MID),
          (128, "f16", N_BIG), (768, "bf16", N_BIG)]


@pytest.mark.parametrize("d,dtype,n", SHAPES)
def test_same_bits_and_fewer_candidates(d, dtype, n):
    X, Q = _data("gauss", n, d)
    idx = _index(X, d, dtype, id_base=1000 if d == 128 else 0)
    try:
        for nq, k in BATCHES:
            kept1, kept0, ref = _check(idx, Q[:nq], k)
            print(f"n={n} d={d} {dtype} nq={nq} k={k}: re-scored {kept1} (untightened {kept0}), pairs {idx.get_option('prefilter_pairs')}")
            if n >= N_MID:      # Gaussian rows: the k-th lower bound lies above the sampling threshold (one query, k = 1 at 140 003 rows:
                distinct = len(np.unique(ref[0]))      # the sampling threshold already leaves the one result row alone — nothing to drop)
                assert kept1 < kept0 or kept0 == distinct, (kept1, kept0, distinct)
            want = _model_count("gauss", n, d, dtype, nq, k, idx, ref)
            assert kept1 >= want, (kept1, want)
    finally:
        idx.close()


# ---- padding rows: every score <= 0, so a zero row of the last panel's padding (s^ = 0) would be the best lower bound there is
@pytest.mark.parametrize("n", [N_SMALL, N_MID])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_padding_rows_stay_out_of_the_threshold(n, dtype):
    d = 128
    X, Q = _data("zeros", n, d)
    idx = _index(X, d, dtype)
    try:
        for k in (20, 64):
            kept1, _, ref = _check(idx, Q[:33], k)
            assert kept1 >= _model_count("zeros", n, d, dtype, 33, k, idx, ref)
    finally:
        idx.close()


# ---- the other input families, at the size with one sampling level and a partial last panel
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("family", ["one-signed", "equal", "norms", "spike"])
def test_input_families(family, dtype):
    d, n = 128, N_MID
    X, Q = _data(family, n, d)
    idx = _index(X, d, dtype)
    try:
        for nq, k in BATCHES[1:]:
            kept1, _, ref = _check(idx, Q[:nq], k)
            if family == "equal":
                assert kept1 == n      # every row ties: nothing may be dropped, and no row may be listed twice
            assert kept1 >= _model_count(family, n, d, dtype, nq, k, idx, ref)
    finally:
        idx.close()


# ---- duplicated queries: a row that several queries hit reaches the re-score once
@pytest.mark.parametrize("period", [1, 4])
def test_duplicated_queries(period):
    d, n, k = 128, N_MID, 20
    X, Q = _data("gauss", n, d)
    Qd = np.ascontiguousarray(Q[np.arange(64) % period])
    idx = _index(X, d, "bf16")
    try:
        _, _, ref = _check(idx, Qd, k)
        for row in ref[0]:
            assert len(np.unique(row)) == k
        for i in range(64):
            assert np.array_equal(ref[0][i], ref[0][i % period])
    finally:
        idx.close()


# ---- overflow: a list that fills tightens by what it holds, the rest of the query's hits are kept directly
def test_pair_list_overflow():
    d, n, k = 128, N_MID, 20
    X, Q = _data("gauss", n, d)
    idx = _index(X, d, "f16")
    try:
        ref = _pipelined(idx, Q, k, 0)
        loose = _pipelined(idx, Q, k, 1, tighten=0)
        kept0 = idx.get_option("prefilter_candidates")
        assert _same_bits(loose, ref)
        got = _pipelined(idx, Q, k, 1, tighten=1, cap=32)
        assert idx.get_option("prefilter_pair_overflow") > 0
        assert idx.get_option("prefilter_pairs") <= 64 * 32
        assert _same_bits(got, ref)
        assert len(np.unique(ref[0])) <= idx.get_option("prefilter_candidates") <= kept0
        for cap in (8, 0):      # fewer records than k (nothing to select from) / none at all: the untightened set
            got = _pipelined(idx, Q, k, 1, tighten=1, cap=cap)
            assert _same_bits(got, ref)
            assert idx.get_option("prefilter_candidates") == kept0
            assert idx.get_option("prefilter_pairs") <= 64 * cap
    finally:
        idx.close()


# ---- appends: across a panel boundary (no capacity growth), then beyond the capacity — keep[] follows the corpus buffer
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_appends_between_tightened_calls(dtype):
    d = 128
    X, Q = _data("gauss", 40_000, d, seed=3)
    idx = _index(X[:8170], d, dtype, capacity_hint=20_000)
    try:
        _check(idx, Q[:33], 20)
        idx.append(X[8170:8197])           # 8170 -> 8197 rows: fills panel 255 and starts panel 256
        _check(idx, Q[:33], 20)
        idx.append(X[8197:40_000])         # beyond the 20 000 rows allocated: the corpus buffer and every per-panel buffer are replaced
        kept1, kept0, _ = _check(idx, Q[:64], 20)
        assert kept1 < kept0
    finally:
        idx.close()


# ---- two workspaces in flight: six calls back to back on alternating pipeline slots, one synchronisation
def test_six_calls_in_flight():
    d, n = 128, N_BIG
    X, Q = _data("gauss", n, d)
    idx = _index(X, d, "bf16")
    try:
        idx.set_option("prefilter", 1)
        calls = [(Q[0:64], 20), (Q[5:38], 20), (Q[10:11], 1), (Q[::-1][:64], MAX_K), (Q[3:40], 7), (Q[20:52], 20)]
        inflight = [_enqueue(idx, np.ascontiguousarray(q), k) for q, k in calls]
        idx.sync(inflight[-1][0])
        import torch
        torch.cuda.synchronize()
        assert idx.query_status() is False
        for (q, k), (_, _, oi, os_) in zip(calls, inflight):
            assert _same_bits((oi.cpu().numpy(), os_.cpu().numpy()), idx.search(np.ascontiguousarray(q), k, with_minmax=False)[:2])
    finally:
        idx.close()


# ---- the route switching on and off inside one in-flight sequence.  Six calls of one pass each take the pipeline's three slots (the default)
# in turn, so calls i and i + 3 share a workspace whichever slot is next.  Both sequences grow the pre-filter's scratch in flight (1 -> 64
# queries); the first, modes 1 0 1 1 0 1, gives every workspace the same mode twice (1 -> 1, 0 -> 0, 1 -> 1: a route's own hand-over); the
# second, modes 1 0 1 0 1 1, puts an unfiltered pass behind a pre-filtered one (1 -> 0: the pre-phase has to wait for the re-score that
# still reads the workspace's query fragments), a pre-filtered pass behind an unfiltered one (0 -> 1) and 1 -> 1.
SWITCH_CALLS = [(1, 1), (64, 20), (33, 20), (64, MAX_K), (5, 20), (33, 1)]


@functools.lru_cache(maxsize=None)
def _switch_queries():
    """the six batches: disjoint slices of the 64 queries where nq allows, the first nq otherwise"""
    _, Q = _data("gauss", N_MID, 128)
    calls, off = [], 0
    for nq, k in SWITCH_CALLS:
        lo = off if off + nq <= 64 else 0
        off = lo + nq if off + nq <= 64 else off
        calls.append((np.ascontiguousarray(Q[lo:lo + nq]), k))
    return calls


def _check_switching(modes):
    d, n = 128, N_MID
    X, _ = _data("gauss", n, d)
    calls = _switch_queries()
    idx = _index(X, d, "bf16")
    try:
        refs = [_pipelined(idx, q, k, 0) for q, k in calls]      # one call at a time, each waited for
        inflight = []
        for (q, k), mode in zip(calls, modes):
            idx.set_option("prefilter", mode)
            inflight.append(_enqueue(idx, q, k))
        idx.sync(inflight[-1][0])
        for ref, (_, _, oi, os_) in zip(refs, inflight):
            assert _same_bits((oi.cpu().numpy(), os_.cpu().numpy()), ref)
        assert idx.query_status() is False
        assert idx.get_option("prefilter_active") == 1
        distinct = len(np.unique(refs[-1][0][refs[-1][0] >= 0]))
        assert distinct <= idx.get_option("prefilter_candidates") <= n
    finally:
        idx.close()


def test_route_switches_between_calls_in_flight():
    _check_switching((1, 0, 1, 1, 0, 1))


def test_route_switches_on_one_workspace_in_flight():
    _check_switching((1, 0, 1, 0, 1, 1))


# ---- mode 2: the filter keeps every row and stores no pair
@pytest.mark.parametrize("n", [N_SMALL, N_MID])
def test_mode_2_keeps_every_row(n):
    d = 128
    X, Q = _data("gauss", n, d)
    idx = _index(X, d, "bf16")
    try:
        ref = _pipelined(idx, Q[:33], 20, 0)
        got = _pipelined(idx, Q[:33], 20, 2)
        assert _same_bits(got, ref)
        assert idx.get_option("prefilter_candidates") == n
        assert idx.get_option("prefilter_pairs") == 0
    finally:
        idx.close()
