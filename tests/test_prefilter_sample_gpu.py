"""The int8 sample of the certified pre-filter on the device: with "prefilter_sample" = 1 the level-1 sampling threshold of a
pre-filtered pass comes from the int8 companion (the filter body over strided runs of panels, bucket, select).  Whatever the sample's
shape, its capacities and the history of the workspaces, a pipelined call returns, bit for bit (ids and scores), what
"prefilter_sample" = 0, "prefilter" = 0 and the synchronous search return."""
import ctypes as C

import numpy as np
import pytest

from tests import prefilter_model as pm
from tests.prefilter_gpu_helpers import BATCHES, MAX_K, N_BIG, N_SMALL, _data, _enqueue, _index, _same_bits

pytestmark = pytest.mark.gpu

NP_BIG = (N_BIG + 31) // 32      # 4376 panels: the smallest size at which sampling levels exist is 4096


def _pipelined(idx, Q, k, prefilter, sample=-1, panels=0, run=0, wave_cap=0, cap=16384, level0=0, active=None):
    idx.set_option("prefilter", prefilter)
    idx.set_option("prefilter_sample", sample)
    idx.set_option("prefilter_sample_panels", panels)
    idx.set_option("prefilter_sample_run", run)
    idx.set_option("prefilter_sample_wave_cap", wave_cap)
    idx.set_option("prefilter_sample_level0", level0)
    idx.set_option("prefilter_pair_cap", cap)
    done, _, oi, os_ = _enqueue(idx, Q, k)
    idx.sync(done)
    assert idx.query_status() is False
    assert idx.get_option("prefilter_active") == (1 if prefilter else 0)
    if active is None:
        active = 1 if (prefilter == 1 and sample == 1) else 0
    assert active < 0 or idx.get_option("prefilter_sample_active") == active      # (active < 0: whatever the plan's auto says)
    return oi.cpu().numpy(), os_.cpu().numpy()


def _references(idx, Q, k):
    """the unfiltered pipeline's result, checked against the synchronous search and against the pre-filter with the bf16 sampling"""
    ref = _pipelined(idx, Q, k, 0)
    kk = min(k, len(idx))
    assert _same_bits((ref[0][:, :kk], ref[1][:, :kk]), idx.search(Q, k, with_minmax=False)[:2])
    assert _same_bits(_pipelined(idx, Q, k, 1, sample=0), ref)
    assert idx.get_option("prefilter_sample_pairs") == 0
    return ref


def _sample_counters(idx):
    return idx.get_option("prefilter_sample_pairs"), idx.get_option("prefilter_sample_overflow")


# ---- every input family (all-equal rows: every lb ties; zero rows and a zero query), both dtypes, one and two query tiles, k = 1 / 20 / 128
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("family", pm.FAMILIES)
def test_families(family, dtype):
    d = 128
    X, Q = _data(family, N_BIG, d)
    idx = _index(X, d, dtype)
    try:
        for nq, k in BATCHES:
            ref = _references(idx, Q[:nq], k)
            got = _pipelined(idx, Q[:nq], k, 1, sample=1)
            pairs, over = _sample_counters(idx)
            print(f"{family} {dtype} nq={nq} k={k}: sample pairs {pairs} overflow {over} main pairs {idx.get_option('prefilter_pairs')} candidates {idx.get_option('prefilter_candidates')}")
            assert _same_bits(got, ref), (nq, k)
            assert pairs > 0
    finally:
        idx.close()


def test_auto_is_what_the_plan_says():
    """`prefilter_sample` = -1: the route the plan ships; whichever it is, the result is the same"""
    d = 128
    X, Q = _data("gauss", N_BIG, d)
    idx = _index(X, d, "bf16")
    try:
        ref = _references(idx, Q, 20)
        assert _same_bits(_pipelined(idx, Q, 20, 1, sample=1), ref)
        got = _pipelined(idx, Q, 20, 1, sample=-1, active=-1)
        assert idx.get_option("prefilter_sample_active") in (0, 1)
        assert _same_bits(got, ref)
    finally:
        idx.close()


# ---- d = 768: three 8-block chunks per panel
def test_dim_768():
    d = 768
    X, Q = _data("gauss", N_BIG, d)
    idx = _index(X, d, "bf16")
    try:
        ref = _references(idx, Q, 20)
        got = _pipelined(idx, Q, 20, 1, sample=1)
        pairs, _ = _sample_counters(idx)
        assert _same_bits(got, ref)
        assert pairs > 0
    finally:
        idx.close()


# ---- one-signed NEGATIVE scores, n no multiple of 32, the sample forced to every panel: without the mask a padding row of the last
# panel (a zero row: lb = -c_q) would hold the best lower bound there is
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_negative_scores_with_every_panel_sampled(dtype):
    d = 128
    X, Q = _data("one-signed", N_BIG, d)
    s = X[:256] @ Q.T
    Qn = -Q if s.min() >= 0 else Q
    assert ((X[:256] @ Qn.T) <= 0).all()
    idx = _index(X, d, dtype)
    try:
        for nq, k in ((33, 20), (64, 1)):
            ref = _references(idx, Qn[:nq], k)
            assert (ref[1] < 0).all()
            got = _pipelined(idx, Qn[:nq], k, 1, sample=1, panels=NP_BIG)
            pairs, _ = _sample_counters(idx)
            assert _same_bits(got, ref), (nq, k)
            assert 0 < pairs <= N_BIG * nq
    finally:
        idx.close()


# ---- forced run shapes: waves without a run (15 runs on 16 waves), single panels, full coverage whose last run the corpus' end cuts
# (4376 = 875 * 5 + 1 = 68 * 64 + 24), a sample beyond half the corpus laid end to end
@pytest.mark.parametrize("panels,run", [(100, 7), (8, 1), (NP_BIG, 5), (NP_BIG, 64), (3000, 16), (1 << 30, 0)])
def test_run_shapes(panels, run):
    d = 128
    X, Q = _data("gauss", N_BIG, d)
    idx = _index(X, d, "bf16")
    try:
        for nq, k in ((64, 20), (1, 1)):
            ref = _references(idx, Q[:nq], k)
            got = _pipelined(idx, Q[:nq], k, 1, sample=1, panels=panels, run=run)
            pairs, _ = _sample_counters(idx)
            print(f"panels={panels} run={run} nq={nq} k={k}: sample pairs {pairs}")
            assert _same_bits(got, ref), (nq, k)
            assert pairs <= min(panels, NP_BIG) * 32 * nq
            # (one query, k = 1: the sample has to beat the best of level 0's 2048 rows — a sample of 256 rows has no such row, a case of too
            # few records; 64 queries with k = 20 let ~2 % of any sample through)
            assert pairs > 0 or (nq, k) == (1, 1)
    finally:
        idx.close()


# ---- a wave's sample area fills: the rest of its hits are dropped; a query's sample list fills: the rest of its records are dropped
def test_sample_records_are_dropped():
    d, k = 128, MAX_K
    X, Q = _data("gauss", N_BIG, d)
    idx = _index(X, d, "f16")
    try:
        ref = _references(idx, Q, k)
        got = _pipelined(idx, Q, k, 1, sample=1)
        full, over = _sample_counters(idx)
        assert _same_bits(got, ref) and over == 0
        got = _pipelined(idx, Q, k, 1, sample=1, wave_cap=64)
        few, _ = _sample_counters(idx)
        print(f"wave_cap 64: sample pairs {few} of {full}")
        assert _same_bits(got, ref)
        assert 0 < few < full
        got = _pipelined(idx, Q, k, 1, sample=1, cap=32)
        pairs, over = _sample_counters(idx)
        print(f"pair_cap 32: sample pairs {pairs}, queries overflowed {over}")
        assert _same_bits(got, ref)
        assert over > 0 and 0 < pairs <= 64 * 32
    finally:
        idx.close()


# ---- fewer than k records: the level-0 key is passed on
def test_fewer_than_k_records():
    d, k = 128, MAX_K
    X, Q = _data("gauss", N_BIG, d)
    idx = _index(X, d, "bf16")
    try:
        ref = _references(idx, Q[:33], k)
        got = _pipelined(idx, Q[:33], k, 1, sample=1, panels=2, run=1)
        pairs, _ = _sample_counters(idx)
        assert pairs <= 64 * 33      # two panels: 64 rows, fewer than k = 128 records per query
        assert _same_bits(got, ref)
    finally:
        idx.close()


# ---- the sample's counters live in the workspaces: after large batches, a 70-row batch on the same index (three calls each, so that every
# slot of the pipeline has held the large batch and then holds the small one)
def test_small_batch_after_large_samples():
    from comorag_amd import _lib as L
    d, nq, k = 128, 64, 20
    X, Q = _data("gauss", N_BIG, d)
    idx = _index(X, d, "bf16")
    try:
        for _ in range(3):
            _pipelined(idx, Q[:nq], MAX_K, 1, sample=1)
        assert idx.get_option("prefilter_sample_pairs") > 0
        # int cmr_index_truncate(cmr_index_t*, long long) of cmr_internal.h: a C++ symbol of the library, not part of its C ABI
        truncate = getattr(L.lib(), "_Z18cmr_index_truncateP9cmr_indexx")
        truncate.argtypes, truncate.restype = [C.c_void_p, C.c_longlong], C.c_int
        L.check(truncate(idx._h, N_SMALL))
        assert len(idx) == N_SMALL
        for _ in range(3):
            got = _pipelined(idx, Q[:nq], k, 1, sample=1, active=0)      # (no sampling level on 70 rows)
            assert idx.get_option("prefilter_sample_pairs") == 0
            assert got[0].max() < N_SMALL
        ref = _pipelined(idx, Q[:nq], k, 0)
        assert _same_bits((ref[0], ref[1]), idx.search(Q[:nq], k, with_minmax=False)[:2])
        assert _same_bits(got, ref)
    finally:
        idx.close()


# ---- an append across a panel boundary between two calls (140 003 = 4375 panels + 3 rows; + 45 rows ends in the next panel)
def test_append_across_a_panel_boundary():
    d, nq, k = 128, 33, 20
    X, Q = _data("gauss", N_BIG + 45, d)
    idx = _index(X[:N_BIG], d, "bf16")
    try:
        ref = _references(idx, Q[:nq], k)
        assert _same_bits(_pipelined(idx, Q[:nq], k, 1, sample=1, panels=NP_BIG), ref)
        extra = np.concatenate([Q[:5] * 1.5, X[N_BIG + 5:N_BIG + 45]]).astype(np.float32)      # the first appended rows are the new best of the first queries
        idx.append(extra)
        assert len(idx) == N_BIG + 45
        ref = _references(idx, Q[:nq], k)
        assert (ref[0][:5, 0] == N_BIG + np.arange(5)).all()
        got = _pipelined(idx, Q[:nq], k, 1, sample=1, panels=NP_BIG + 2)
        assert idx.get_option("prefilter_sample_pairs") > 0
        assert _same_bits(got, ref)
    finally:
        idx.close()
