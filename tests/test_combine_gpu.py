"""Concurrent single calls combined into one batched call (option "combine", comorag_amd/csrc/combine.h) on the device: a
combined caller gets the BITS of its solo call.  Every test takes the solo results first, on the same index, with combine = 0, and compares
with np.array_equal.

Gather windows: a leader with a window waits until its batch is full or the window has passed, so every long-window batch here is one that
fills exactly (the width is set to what the test's threads bring) and no test waits a window out."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import retrieval_np as orc

pytestmark = pytest.mark.gpu

LONG_US = 500_000
K = 20


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
    for g, w in zip(got, want):
        assert np.array_equal(g, w)


def _moved(idx, before):
    now = idx.combine_stats()
    return now["batches"] - before["batches"], now["queries"] - before["queries"], now["max_width"]


@pytest.fixture(scope="module")
def corpus5k():
    X = orc.synthetic_corpus(5000, 128, seed=301)
    Q = orc.synthetic_queries(800, 128, seed=302, planted=X)
    return X, Q


def _index(X, dtype, options=None):
    from comorag_amd.index import DenseIndex
    idx = DenseIndex(X.shape[1], dtype, options=options)
    idx.append(X)
    return idx


CHAIN = {"scan_no_tiny": 1, "scan_no_small": 1, "small_max_panels": 32}      # no single-launch path: solo = the finishing-stage scan, 16 queries = the chain


@pytest.mark.parametrize("shape", ["300x64-f32", "5000x128-bf16", "5000x128-bf16-chain", "301x64-f16"])
def test_barrier_one_batch_of_sixteen(shape, corpus5k):
    if shape.startswith("5000"):
        X, Q, dtype, opts = corpus5k[0], corpus5k[1][:16], "bf16", (CHAIN if shape.endswith("chain") else None)
    else:
        n, dtype, opts = (300, "f32", None) if shape.startswith("300") else (301, "f16", None)
        X = orc.synthetic_corpus(n, 64, seed=311)
        Q = orc.synthetic_queries(16, 64, seed=312, planted=X)
    idx = _index(X, dtype, opts)
    solo = [idx.search(Q[i], K) for i in range(16)]
    idx.set_option("combine", 16)
    idx.set_option("combine_wait_us", LONG_US)
    before = idx.combine_stats()
    got = _run([lambda i=i: idx.search(Q[i], K) for i in range(16)])
    for i in range(16):
        _same(got[i], solo[i])                                  # ids, scores, min, max
    assert _moved(idx, before) == (1, 16, 16)
    idx.close()


def test_no_window_sixteen_threads_fifty_calls(corpus5k):
    X, Q = corpus5k
    idx = _index(X, "bf16")
    solo = [idx.search(Q[i], K) for i in range(800)]
    idx.set_option("combine", 16)
    before = idx.combine_stats()

    def worker(t):
        return [idx.search(Q[t * 50 + j], K) for j in range(50)]
    got = _run([lambda t=t: worker(t) for t in range(16)])
    for t in range(16):
        assert not isinstance(got[t], Exception), repr(got[t])
        for j in range(50):
            _same(got[t][j], solo[t * 50 + j])
    batches, queries, width = _moved(idx, before)
    print(f"no window: 800 calls in {batches} batches, widest {width}")
    assert queries == 800 and 1 <= batches <= 800 and width <= 16
    idx.close()


def test_mixed_k_never_shares_a_batch(corpus5k):
    X, Q = corpus5k
    idx = _index(X, "bf16")
    ks = [5 if i < 8 else 20 for i in range(16)]
    solo = [idx.search(Q[i], ks[i]) for i in range(16)]
    idx.set_option("combine", 8)                                # eight callers of either k: two batches that fill, none waits
    idx.set_option("combine_wait_us", LONG_US)
    before = idx.combine_stats()
    got = _run([lambda i=i: idx.search(Q[i], ks[i]) for i in range(16)])
    for i in range(16):
        _same(got[i], solo[i])
    assert _moved(idx, before) == (2, 16, 8)
    idx.close()


def test_mixed_query_counts_join_and_a_full_call_runs_solo(corpus5k):
    X, Q = corpus5k
    idx = _index(X, "bf16")
    cuts = [(0, 1), (1, 4), (4, 11), (11, 16), (16, 32)]       # nq = 1, 3, 7, 5 fill one batch of 16; nq = 16 cannot share
    solo = [idx.search(Q[a:b], K, with_minmax=(a != 1)) for a, b in cuts]
    idx.set_option("combine", 16)
    idx.set_option("combine_wait_us", LONG_US)
    before = idx.combine_stats()
    got = _run([lambda a=a, b=b: idx.search(Q[a:b], K, with_minmax=(a != 1)) for a, b in cuts])      # (one caller without min / max: NULL pointers)
    for g, w in zip(got, solo):
        assert not isinstance(g, Exception), repr(g)
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])
        assert (g[2] is None and w[2] is None) or (np.array_equal(g[2], w[2]) and np.array_equal(g[3], w[3]))
    assert _moved(idx, before) == (1, 16, 16)                   # the 16-query call went round the combiner
    idx.close()


def test_one_nan_query_fails_alone(corpus5k):
    from comorag_amd import _lib as L
    X, Q = corpus5k
    Q = Q[:16].copy()
    idx = _index(X, "bf16")
    solo = [idx.search(Q[i], K) for i in range(16)]
    Q[6, 17] = np.nan
    idx.set_option("combine", 15)                               # the fifteen finite queries fill the batch
    idx.set_option("combine_wait_us", LONG_US)
    before = idx.combine_stats()
    got = _run([lambda i=i: idx.search(Q[i], K) for i in range(16)])
    for i in range(16):
        if i == 6:
            assert isinstance(got[i], L.CmrError) and got[i].code == L.CMR_ERR_NONFINITE, repr(got[i])
        else:
            _same(got[i], solo[i])
    assert _moved(idx, before) == (1, 15, 15)
    idx.set_option("combine_wait_us", 0)
    _same(idx.search(Q[0], K), solo[0])                         # the index is none the worse for it
    idx.close()


@pytest.mark.parametrize("shape", ["301x64-f32", "5000x128-bf16"])
def test_scores_rows_equal_solo(shape, corpus5k):
    if shape.startswith("5000"):
        X, Q, dtype = corpus5k[0], corpus5k[1][:16], "bf16"
    else:
        X = orc.synthetic_corpus(301, 64, seed=321)
        Q, dtype = orc.synthetic_queries(16, 64, seed=322, planted=X), "f32"
    idx = _index(X, dtype)
    solo = [idx.scores(Q[i]) for i in range(16)]
    idx.set_option("combine", 16)
    idx.set_option("combine_wait_us", LONG_US)
    before = idx.combine_stats()
    got = _run([lambda i=i: idx.scores(Q[i]) for i in range(16)])
    for i in range(16):
        assert not isinstance(got[i], Exception), repr(got[i])
        assert got[i].shape == solo[i].shape and np.array_equal(got[i], solo[i])
    assert _moved(idx, before) == (1, 16, 16)
    idx.close()


def _degree_class_graph():
    """the graph of tests/test_ppr.py::test_device_ppr_degree_classes_hub_medium_and_short_rows: two hubs, medium rows, rows of exactly 4
    and 5 entries, parallel edges, a self-loop (9), isolated vertices (11, 12, 13)"""
    rng = np.random.default_rng(4242)
    n = 2600
    src, dst = [], []
    for h, fan in zip((7, 1901), (1500, 300)):
        nb = rng.choice(np.setdiff1d(np.arange(n), [h, 11, 12, 13]), fan, replace=False)
        src += [h] * fan; dst += nb.tolist()
    for v in rng.choice(np.arange(20, n), 120, replace=False):
        nb = rng.choice(np.setdiff1d(np.arange(n), [v, 11, 12, 13]), int(rng.integers(6, 41)), replace=False)
        src += [int(v)] * len(nb); dst += nb.tolist()
    src += [5, 5, 5, 5, 6, 6, 6, 6, 6, 3, 3, 9]
    dst += [1, 2, 4, 8, 1, 2, 4, 8, 10, 4, 4, 9]
    return n, np.array(src, np.int32), np.array(dst, np.int32), rng.uniform(0.2, 2.0, len(src))


def _index_ppr(idx, g, q, sv, sw, pnw):
    """cmr_index_ppr -> (doc scores, iters)"""
    from comorag_amd import _lib as L
    q = np.ascontiguousarray(q, np.float32)
    sv = np.ascontiguousarray(sv, np.int32); sw = np.ascontiguousarray(sw, np.float64)
    out = np.empty(g.n_rows, np.float64)
    it = C.c_int32(-1)
    L.check(L.lib().cmr_index_ppr(idx._h, g._h, q.ctypes.data_as(C.c_void_p), sv.ctypes.data_as(C.c_void_p), sw.ctypes.data_as(C.c_void_p), len(sv),
                                  float(pnw), 0.5, 1e-12, 200, out.ctypes.data_as(C.c_void_p), C.byref(it)))
    return out, np.int64(it.value)


def test_index_ppr_calls_share_one_batch():
    from comorag_amd.ppr import DeviceGraph
    nv, src, dst, w = _degree_class_graph()
    rng = np.random.default_rng(77)
    n_pass, d = 700, 64
    X = orc.synthetic_corpus(n_pass, d, seed=331)
    Q = orc.synthetic_queries(16, d, seed=332, planted=X)
    idx = _index(X, "bf16")
    g = DeviceGraph(nv, src, dst, w)
    g.set_passage_vertices(rng.permutation(nv)[:n_pass].astype(np.int32))
    seeds = []
    for i in range(16):
        m = int(rng.integers(1, 9))
        seeds.append((rng.integers(0, nv, m).astype(np.int32), rng.uniform(0.2, 1.0, m)))
    seeds[2] = (np.empty(0, np.int32), np.empty(0, np.float64))                               # no seeds at all
    seeds[3] = (np.array([7, 40, 7, 11], np.int32), np.array([0.3, 0.2, 0.25, 0.4]))          # a duplicate (the hub) and an isolated vertex
    seeds[4] = (np.array([11, 12, 9], np.int32), np.array([0.5, 0.1, 0.7]))                   # isolated seeds and the self-loop
    pnws = [0.05] * 16
    solo = [_index_ppr(idx, g, Q[i], *seeds[i], pnws[i]) for i in range(16)]
    solo_other = [_index_ppr(idx, g, Q[i], *seeds[i], 0.2) for i in range(2)]
    idx.set_option("combine", 16)
    idx.set_option("combine_wait_us", LONG_US)
    before = idx.combine_stats()
    got = _run([lambda i=i: _index_ppr(idx, g, Q[i], *seeds[i], pnws[i]) for i in range(16)])
    for i in range(16):
        _same(got[i], solo[i])                                                                # doc scores and iters
    assert _moved(idx, before) == (1, 16, 16)
    # another passage_node_weight is another key: two callers of either weight, width 2 — were the key blind to the weight, a batch would
    # mix them and its rows would carry the wrong weight
    idx.set_option("combine", 2)
    before = idx.combine_stats()
    got = _run([lambda i=i: _index_ppr(idx, g, Q[i % 2], *seeds[i % 2], 0.05 if i < 2 else 0.2) for i in range(4)])
    for i in range(4):
        _same(got[i], solo[i] if i < 2 else solo_other[i - 2])
    assert _moved(idx, before)[:2] == (2, 4)
    idx.close(); g.close()


def test_append_meanwhile_no_deadlock():
    """8 searchers through the combiner (width 8) and one appender whose chunks double the capacity again and again: a queued caller holds no
    index lock and the leader takes the shared lock once, so the appender waiting for the exclusive lock cannot wedge them.  Every answer is
    the exact top-k of some committed prefix (as tests/test_search_gpu.py::test_concurrent_append_and_search checks it)."""
    from comorag_amd.index import DenseIndex
    ERR = 4e-6
    d, k = 128, 10
    X = orc.synthetic_corpus(30_000, d, seed=341)
    Q = orc.synthetic_queries(8, d, seed=342)
    Xr, Qr = orc.bf16_round(X), orc.bf16_round(Q)
    exact = Qr.astype(np.float64) @ Xr.astype(np.float64).T
    chunks = [(0, 2000)] + [(a, min(a + 3500, len(X))) for a in range(2000, len(X), 3500)]
    bounds = [b for _, b in chunks]
    refs = {n: orc.topk_rule(exact[:, :n], k)[0] for n in bounds}
    idx = DenseIndex(d, "bf16", capacity_hint=16, options={"combine": 8, "combine_wait_us": 200})
    idx.append(X[:2000])
    stop, errors, seen = threading.Event(), [], []

    def reader(t):
        try:
            while not stop.is_set():
                n0 = len(idx)
                ids, sc, mn, mx = idx.search(Q[t], k)
                n1 = len(idx)
                ok = False
                for n in [b for b in bounds if n0 <= b <= n1]:
                    try:
                        orc.assert_topk_equivalent(ids[0], refs[n][t], exact[t], ERR)
                        ok = True
                        break
                    except AssertionError:
                        continue
                if not ok:
                    errors.append((t, n0, n1, ids[0, :3].tolist()))
                seen.append(n1)
        except Exception as e:              # noqa: BLE001
            errors.append((t, repr(e)))

    def appender():
        try:
            for a, b in chunks[1:]:
                idx.append(X[a:b])
        except Exception as e:              # noqa: BLE001
            errors.append(("append", repr(e)))
        stop.set()
    threads = [threading.Thread(target=reader, args=(t,), daemon=True) for t in range(8)] + [threading.Thread(target=appender, daemon=True)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(120.0)
        if th.is_alive():
            stop.set()
            pytest.fail("deadlock: searchers and the appender did not finish")
    assert not errors, errors[:3]
    assert len(idx) == len(X) and len(set(seen)) >= 2
    st = idx.combine_stats()
    assert st["queries"] == len(seen) and st["max_width"] <= 8
    idx.close()


def test_default_is_off_and_widths_are_checked():
    from comorag_amd import _lib as L
    X = orc.synthetic_corpus(300, 64, seed=351)
    Q = orc.synthetic_queries(4, 64, seed=352)
    idx = _index(X, "f32")
    assert idx.get_option("combine") == 0 and idx.get_option("combine_wait_us") == 0
    got = _run([lambda i=i: idx.search(Q[i], 5) for i in range(4)])
    assert not any(isinstance(g, Exception) for g in got)
    idx.scores(Q[0])
    assert idx.combine_stats() == {"batches": 0, "queries": 0, "max_width": 0}
    for bad in (1, 17, -1):
        with pytest.raises(L.CmrError):
            idx.set_option("combine", bad)
    assert idx.get_option("combine") == 0
    for good in (2, 16, 0):
        idx.set_option("combine", good)
        assert idx.get_option("combine") == good
    idx.close()
