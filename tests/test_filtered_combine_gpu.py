"""Concurrent filtered host calls combined into ONE per-query-mask search (options "combine" + "combine_filtered"): every
caller gets the BITS of its solo call.  Solo results are taken first, on the same index, with combine = 0, and compared with
np.array_equal.  As in tests/test_combine_gpu.py every long-window batch fills exactly, so no test waits a window out."""
import threading

import numpy as np
import pytest

from comorag_amd import _lib as L
from comorag_amd.index import pack_row_mask, pack_row_masks
from oracle import retrieval_np as orc

pytestmark = pytest.mark.gpu

LONG_US = 500_000
K = 20
N = 5000
EACH = 1 << 13


def _run(fns, timeout=120.0):
    """every fn on a thread of its own, released by one barrier -> [result or exception]; a thread that does not come back fails the test"""
    out = [None] * len(fns)
    bar = threading.Barrier(len(fns))

    def work(i):
        try:
            bar.wait()
            out[i] = fns[i]()
        except Exception as e:          # noqa: BLE001
            out[i] = e
    ts = [threading.Thread(target=work, args=(i,), daemon=True) for i in range(len(fns))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout)
        assert not t.is_alive(), "deadlock: a combined call did not return"
    return out


def _same(got, want):
    assert not isinstance(got, Exception), repr(got)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)


def _moved(idx, before):
    now = idx.combine_stats()
    return now["batches"] - before["batches"], now["queries"] - before["queries"], now["max_width"]


@pytest.fixture(scope="module")
def corpus():
    X = orc.synthetic_corpus(N, 128, seed=301)
    Q = orc.synthetic_queries(800, 128, seed=302, planted=X)
    rng = np.random.default_rng(303)
    masks = np.stack([pack_row_mask(N, allow=rng.random(N) < (0.5 if t % 2 else 0.02)) for t in range(16)])      # one per thread
    return X, Q, masks


def _index(X, options=None):
    from comorag_amd.index import DenseIndex
    idx = DenseIndex(X.shape[1], "bf16", options=options)
    idx.append(X)
    return idx


def test_barrier_one_batch_of_sixteen(corpus):
    X, Q, masks = corpus
    idx = _index(X)
    solo = [idx.search_filtered(Q[i], K, mask=masks[i]) for i in range(16)]
    idx.set_option("combine", 16)
    idx.set_option("combine_filtered", 1)
    idx.set_option("combine_wait_us", LONG_US)
    before = idx.combine_stats()
    got = _run([lambda i=i: idx.search_filtered(Q[i], K, mask=masks[i]) for i in range(16)])
    for i in range(16):
        _same(got[i], solo[i])                                  # ids, scores, min, max
    assert _moved(idx, before) == (1, 16, 16)
    assert idx.get_option("last_route") & EACH                  # the batch ran as one per-query-mask search
    idx.close()


def test_no_window_sixteen_threads_fifty_calls(corpus):
    X, Q, masks = corpus
    idx = _index(X)
    solo = [idx.search_filtered(Q[i], K, mask=masks[i // 50]) for i in range(800)]
    idx.set_option("combine", 16)
    idx.set_option("combine_filtered", 1)
    before = idx.combine_stats()

    def worker(t):
        return [idx.search_filtered(Q[t * 50 + j], K, mask=masks[t]) for j in range(50)]
    got = _run([lambda t=t: worker(t) for t in range(16)])
    for t in range(16):
        assert not isinstance(got[t], Exception), repr(got[t])
        for j in range(50):
            _same(got[t][j], solo[t * 50 + j])
    batches, queries, width = _moved(idx, before)
    print(f"no window: 800 filtered calls in {batches} batches, widest {width}")
    assert queries == 800 and 1 <= batches <= 800 and width <= 16
    idx.close()


def test_filtered_and_unfiltered_calls_never_share_and_neither_do_different_k(corpus):
    X, Q, masks = corpus
    idx = _index(X)
    # eight filtered k = 20, four unfiltered k = 20, four filtered k = 5: with widths that fill exactly, three batches
    def call(i):
        if i < 8:
            return idx.search_filtered(Q[i], K, mask=masks[i])
        if i < 12:
            return idx.search(Q[i], K)
        return idx.search_filtered(Q[i], 5, mask=masks[i])
    solo = [call(i) for i in range(16)]
    idx.set_option("combine_filtered", 1)
    idx.set_option("combine_wait_us", LONG_US)
    before = idx.combine_stats()
    idx.set_option("combine", 8)
    got = _run([lambda i=i: call(i) for i in range(8)])
    idx.set_option("combine", 4)
    got += _run([lambda i=i: call(i) for i in range(8, 16)])          # four unfiltered and four filtered of another k at once: two batches of four
    for i in range(16):
        _same(got[i], solo[i])
    assert _moved(idx, before) == (3, 16, 8)
    idx.close()


def test_shared_mask_call_of_three_and_each_call_of_two_join_one_batch(corpus):
    X, Q, masks = corpus
    idx = _index(X)
    each_words = np.ascontiguousarray(masks[4:6])
    fns = [lambda: idx.search_filtered(Q[0:3], K, mask=masks[1]), lambda: idx.search_filtered_each(Q[3:5], K, masks=each_words)]
    solo = [f() for f in fns]
    idx.set_option("combine", 5)
    idx.set_option("combine_filtered", 1)
    idx.set_option("combine_wait_us", LONG_US)
    before = idx.combine_stats()
    got = _run(fns)
    for g, w in zip(got, solo):
        _same(g, w)
    assert _moved(idx, before) == (1, 5, 5)
    idx.close()


def test_default_is_off_filtered_calls_do_not_move_the_counters(corpus):
    X, Q, masks = corpus
    idx = _index(X, options={"combine": 16})
    assert idx.get_option("combine_filtered") == 0
    solo = [idx.search_filtered(Q[i], K, mask=masks[i]) for i in range(16)]
    before = idx.combine_stats()
    got = _run([lambda i=i: idx.search_filtered(Q[i], K, mask=masks[i]) for i in range(16)])
    got_each = idx.search_filtered_each(Q[:4], K, masks=np.ascontiguousarray(masks[:4]))
    for i in range(16):
        _same(got[i], solo[i])
    assert _moved(idx, before)[:2] == (0, 0)
    for i in range(4):
        assert np.array_equal(got_each[0][i], solo[i][0][0])
    idx.close()
    idx = _index(X[:64], options={"combine": 16, "combine_filtered": 1})          # the option goes through the constructor's plumbing
    assert idx.get_option("combine_filtered") == 1
    idx.close()


def test_one_nan_query_or_one_wrong_word_count_fails_alone(corpus):
    X, Q, masks = corpus
    Q = Q[:16].copy()
    idx = _index(X)
    solo = [idx.search_filtered(Q[i], K, mask=masks[i]) for i in range(16)]
    Q[6, 17] = np.nan
    short = masks[9][:-1].copy()

    def call(i):
        return idx.search_filtered(Q[i], K, mask=short if i == 9 else masks[i])
    idx.set_option("combine", 14)                               # the fourteen sound calls fill the batch
    idx.set_option("combine_filtered", 1)
    idx.set_option("combine_wait_us", LONG_US)
    before = idx.combine_stats()
    got = _run([lambda i=i: call(i) for i in range(16)])
    for i in range(16):
        if i == 6:
            assert isinstance(got[i], L.CmrError) and got[i].code == L.CMR_ERR_NONFINITE, repr(got[i])
        elif i == 9:
            assert isinstance(got[i], L.CmrError) and got[i].code == L.CMR_ERR_INVALID, repr(got[i])
        else:
            _same(got[i], solo[i])
    assert _moved(idx, before) == (1, 14, 14)                   # neither refused call queued: each got its error from its own single call
    idx.set_option("combine_wait_us", 0)
    _same(idx.search_filtered(Q[0], K, mask=masks[0]), solo[0])          # the index is none the worse for it
    idx.close()
