"""The PageRank passage ranking on the device (cmr_index_ppr_ranked, cmr_index_ppr_ranked_batch, cmr_graph_ppr_ranked_batch; DESIGN
§4.9c): ids == np.argsort(-doc, kind="stable") and scores == doc[ids] BIT FOR BIT, where `doc` is what the existing unranked call returns
for the same inputs.  Every comparison is on integers or on bit patterns.  CPU twin (argument checks, the switch in ppr.py and hooks.py):
tests/test_ppr_rank_host.py."""
import ctypes as C
import threading

import numpy as np
import pytest

from oracle import retrieval_np as orc

pytestmark = pytest.mark.gpu

from comorag_amd import _lib as L

T = L.CMR_PPR_RANK_TILE  # the sort's tile (held against the header in tests/test_ppr_rank_host.py)
LONG_US = 500_000


def _want(doc, n_out=None):
    """(ids, scores) of the exported order: score descending, equal scores by ascending row."""
    ids = np.argsort(-doc, kind="stable")[:n_out]
    return ids, doc[ids]


def _check(ids, sc, doc, n_out=None, what=()):
    wi, ws = _want(doc, n_out)
    assert ids.dtype == np.int64 and sc.dtype == np.float64 and ids.shape == wi.shape and sc.shape == ws.shape, what
    assert np.array_equal(ids, wi), (what, int(np.flatnonzero(ids != wi)[0]))
    assert np.array_equal(sc.view(np.int64), ws.view(np.int64)), what


# ---- 1. key level: an edgeless graph of passages only, so score_i = reset_i / sum(reset) and the reset vector dictates the keys
def _key_resets(n, seed):
    """16 rows: magnitudes over 300 decades (every digit position above the mantissa's varies), blocks of exact zeros, negative and NaN
    entries (cleaned to 0: more ties), a row of zeros (uniform: ALL scores tie), a row with one non-zero entry."""
    rng = np.random.default_rng(seed)
    R = 10.0 ** rng.uniform(-300, 0, (16, n))
    for b in range(16):
        if n >= 8:
            a = int(rng.integers(0, n - n // 4))
            R[b, a:a + n // 4] = 0.0                                     # a block of exact zeros
        R[b, rng.integers(0, n, max(1, n // 16))] = -rng.uniform(0.1, 1.0)
        R[b, rng.integers(0, n, max(1, n // 16))] = np.nan
        R[b, rng.integers(0, n)] = 1.0                                   # never an all-cleaned row by accident
    R[5] = 0.0
    R[9] = 0.0; R[9, n // 2] = 3.0
    h = n // 2
    R[11, :h] = R[11, n - h:][::-1]                                      # equal pairs far apart
    return R


# 70001 and 3 * 65536 + 5: more than 32 tiles, so the scan kernel's loop over 8192 counters runs 2 and 4 times (its carry is handed over),
# all 16 of its waves hold counters, and the scatter's tile index passes the sizes the fused cases reach
@pytest.mark.parametrize("n_rows", [1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5, 70001, 3 * 65536 + 5])
def test_key_level_through_the_graph_call(n_rows):
    from comorag_amd.ppr import DeviceGraph
    NB = 16 if n_rows < 10000 else 3                                     # the large sizes: nb in {1, 3}
    g = DeviceGraph(n_rows, np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0, np.float64))
    pv = np.random.default_rng(n_rows).permutation(n_rows).astype(np.int32)
    g.set_passage_vertices(pv)
    R = _key_resets(n_rows, seed=1000 + n_rows)
    R = R[[0, 5, 11]] if NB == 3 else R                                  # (magnitudes + zero block, all tied, equal pairs far apart)
    doc = np.ascontiguousarray(g.ppr_batch(R)[:, pv])
    if n_rows > 64:
        assert len(np.unique(doc[0])) < n_rows and len(np.unique(doc[0])) > n_rows // 2      # ties AND many distinct keys
        assert np.ptp(np.log10(doc[0][doc[0] > 0])) > 200                                    # exponent digits vary
    single = [g.ppr_ranked_batch(R[b:b + 1]) for b in range(NB)]
    for b in range(NB):
        assert single[b][0].shape == (1, n_rows)
        _check(single[b][0][0], single[b][1][0], doc[b], what=(n_rows, "single", b))
    for nb in sorted({3, NB}):
        ids, sc = g.ppr_ranked_batch(R[:nb])
        assert ids.shape == (nb, n_rows)
        for b in range(nb):
            assert np.array_equal(ids[b], single[b][0][0]), (n_rows, nb, b)
            assert np.array_equal(sc[b].view(np.int64), single[b][1][0].view(np.int64)), (n_rows, nb, b)
    # other rows next to it, another position of the batch: a query's ranking does not depend on its neighbours
    order = (7, 5, 0) if NB == 16 else (2, 0, 1)
    ids, sc = g.ppr_ranked_batch(R[list(order)])
    for k, b in enumerate(order):
        _check(ids[k], sc[k], doc[b], what=(n_rows, "reordered", b))
    if n_rows >= 20:
        ids, sc = g.ppr_ranked_batch(R[:3], n_out=20)
        for b in range(3):
            _check(ids[b], sc[b], doc[b], 20, what=(n_rows, "n_out", b))
    g.close()


# ---- 2 .. 7: the fused call on the 5000-passage case of tests/test_ppr_batch_gpu.py::_fused_case
def _fused_case(n_pass=5000, n_ent=1500, d=128, nq=20, tied=0):
    """_fused_case of tests/test_ppr_batch_gpu.py.  tied > 0: the first `tied` embedding rows are copies of row 0 and their passage
    vertices have no edges, so their score depends on their (equal) reset entry alone."""
    X = orc.synthetic_corpus(n_pass, d, seed=8); Q = orc.synthetic_queries(nq, d, seed=9, planted=X)
    rng = np.random.default_rng(10)
    nv = n_ent + n_pass
    passage_vertex = (n_ent + rng.permutation(n_pass)).astype(np.int32)
    src = np.concatenate([rng.integers(0, n_ent, 3 * n_pass), rng.integers(0, n_ent, 2000)]).astype(np.int32)
    dst = np.concatenate([np.repeat(passage_vertex, 3), rng.integers(0, n_ent, 2000)]).astype(np.int32)
    keep = src != dst
    if tied:
        X = X.copy(); X[:tied] = X[0]
        keep &= ~np.isin(dst, passage_vertex[:tied])
    src, dst = src[keep], dst[keep]
    w = rng.uniform(0.5, 1.5, len(src))
    phrases = []
    for b in range(nq):
        if b % 5 == 1:
            phrases.append(None)
        elif b % 5 == 3:
            phrases.append((np.array([3, 9, 3, 3], np.int32), np.array([0.25, 0.5, 0.125, 0.0625])))
        else:
            ph = np.zeros(nv); ph[rng.integers(0, n_ent, 6)] = rng.uniform(0.2, 1.0, 6); phrases.append(ph)
    return X, Q, nv, passage_vertex, src, dst, w, phrases


@pytest.fixture(scope="module", params=["f32", "bf16"])
def fused(request):
    """(index, graph, Q, phrases, doc [20, n]): the unranked scores are computed once and left unchanged."""
    from comorag_amd.index import DenseIndex
    from comorag_amd.ppr import DeviceGraph, ppr_passage_scores
    X, Q, nv, passage_vertex, src, dst, w, phrases = _fused_case()
    idx = DenseIndex(X.shape[1], request.param); idx.append(X)
    g = DeviceGraph(nv, src, dst, w); g.set_passage_vertices(passage_vertex)
    doc = np.stack([ppr_passage_scores(idx, g, Q[b], phrases[b], 0.05) for b in range(len(Q))])
    doc.setflags(write=False)
    yield idx, g, Q, phrases, doc
    idx.close(); g.close()


def test_fused_call_equals_the_stable_argsort_of_the_unranked_call(fused):
    from comorag_amd.ppr import ppr_passage_ranked
    idx, g, Q, phrases, doc = fused
    n = doc.shape[1]
    for b in (0, 1, 3):                                                  # dense phrase weights, no seeds, duplicated seeds
        full = ppr_passage_ranked(idx, g, Q[b], phrases[b], 0.05)
        _check(full[0], full[1], doc[b], what=("full", b))
        for n_out in (1, 20, n):
            ids, sc = ppr_passage_ranked(idx, g, Q[b], phrases[b], 0.05, n_out=n_out)
            assert ids.shape == (n_out,) and np.array_equal(ids, full[0][:n_out])
            assert np.array_equal(sc.view(np.int64), full[1][:n_out].view(np.int64))


def test_batch_equals_singles_bit_for_bit(fused):
    from comorag_amd.ppr import ppr_passage_ranked, ppr_passage_ranked_batch
    idx, g, Q, phrases, doc = fused
    single = [ppr_passage_ranked(idx, g, Q[b], phrases[b], 0.05) for b in range(20)]
    for b in range(20):
        _check(single[b][0], single[b][1], doc[b], what=("single", b))
    for B in (2, 7, 16, 20):                                             # 20: two chunks through the Python layer
        ids, sc = ppr_passage_ranked_batch(idx, g, Q[:B], phrases[:B], 0.05)
        assert ids.shape == (B, doc.shape[1]) and sc.shape == ids.shape
        for b in range(B):
            assert np.array_equal(ids[b], single[b][0]), (B, b)
            assert np.array_equal(sc[b].view(np.int64), single[b][1].view(np.int64)), (B, b)
    ids, sc = ppr_passage_ranked_batch(idx, g, Q[:7], phrases[:7], 0.05, n_out=20)
    for b in range(7):
        assert np.array_equal(ids[b], single[b][0][:20]) and np.array_equal(sc[b].view(np.int64), single[b][1][:20].view(np.int64))


@pytest.fixture(scope="module")
def tied():
    from comorag_amd.index import DenseIndex
    from comorag_amd.ppr import DeviceGraph, ppr_passage_scores
    X, Q, nv, passage_vertex, src, dst, w, phrases = _fused_case(nq=4, tied=200)
    idx = DenseIndex(X.shape[1], "f32"); idx.append(X)
    g = DeviceGraph(nv, src, dst, w); g.set_passage_vertices(passage_vertex)
    doc = np.stack([ppr_passage_scores(idx, g, Q[b], phrases[b], 0.05) for b in range(4)])
    doc.setflags(write=False)
    yield idx, g, Q, phrases, doc
    idx.close(); g.close()


def test_equal_scores_come_by_ascending_row(tied):
    from comorag_amd.ppr import ppr_passage_ranked_batch
    idx, g, Q, phrases, doc = tied
    n = doc.shape[1]
    ids, sc = ppr_passage_ranked_batch(idx, g, Q, phrases, 0.05)
    for b in range(4):
        assert len(np.unique(doc[b])) <= n - 150                        # ties exist: the test cannot pass vacuously
        assert sorted(ids[b].tolist()) == list(range(n))
        same = sc[b][1:].view(np.int64) == sc[b][:-1].view(np.int64)
        assert same.sum() >= 150
        assert np.all(ids[b][1:][same] > ids[b][:-1][same])             # ascending rows inside every run of equal scores
        assert np.all(sc[b][1:][~same] < sc[b][:-1][~same])
        _check(ids[b], sc[b], doc[b], what=("tied", b))


def test_the_switch_keeps_the_host_lines_below_the_threshold(tied, monkeypatch):
    from comorag_amd import ppr
    idx, g, Q, phrases, doc = tied
    thr = ppr.DEVICE_RANK_MIN_ROWS                                       # None: the switch is off; else the sweep's crossover, floor 8192
    assert thr is None or (thr >= 8192 and thr % 1024 == 0)
    calls = []
    real = ppr.ppr_passage_ranked
    monkeypatch.setattr(ppr, "ppr_passage_ranked", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    # 5000 rows with the shipped threshold: exactly the two numpy lines on ppr_passage_scores — existing behaviour
    ids, sc = ppr.ppr_passage_ranking(idx, g, Q[0], phrases[0], 0.05)
    host_ids = np.argsort(doc[0])[::-1]
    assert not calls and np.array_equal(ids, host_ids) and np.array_equal(sc.view(np.int64), doc[0][host_ids.tolist()].view(np.int64))
    got = ppr.ppr_passage_ranking_batch(idx, g, Q[:2], phrases[:2], 0.05)
    for b in range(2):
        h = np.argsort(doc[b])[::-1]
        assert np.array_equal(got[b][0], h) and np.array_equal(got[b][1], doc[b][h.tolist()])
    # threshold 0: the device ranking
    monkeypatch.setattr(ppr, "DEVICE_RANK_MIN_ROWS", 0)
    ids, sc = ppr.ppr_passage_ranking(idx, g, Q[0], phrases[0], 0.05)
    assert calls == [1]
    _check(ids, sc, doc[0], what="switch")
    got = ppr.ppr_passage_ranking_batch(idx, g, Q[:2], phrases[:2], 0.05)
    for b in range(2):
        _check(got[b][0], got[b][1], doc[b], what=("switch batch", b))
    rs = np.zeros(g.n_vertices); rs[g.passage_vertices[:50]] = np.arange(1, 51)
    ids, sc = ppr.run_ppr(g, rs, g.passage_vertices.tolist(), 0.5)
    _check(ids, sc, g.ppr(rs)[g.passage_vertices], what="run_ppr")


# ---- 6. combine: concurrent cmr_index_ppr_ranked calls share one batched PageRank and one segmented sort
def _run(fns, timeout=120.0):
    """tests/test_combine_gpu.py::_run: every fn on a thread of its own, released by one barrier"""
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


def _index_ppr_ranked(idx, g, q, pw, n_out):
    """cmr_index_ppr_ranked -> (ids, scores, iters)"""
    from comorag_amd import _lib as L
    from comorag_amd.ppr import _seed_arrays
    q = np.ascontiguousarray(q, np.float32)
    sv, sw = _seed_arrays(pw)
    ids = np.empty(n_out, np.int64); sc = np.empty(n_out, np.float64)
    it = C.c_int32(-1)
    L.check(L.lib().cmr_index_ppr_ranked(idx._h, g._h, q.ctypes.data_as(C.c_void_p), sv.ctypes.data_as(C.c_void_p), sw.ctypes.data_as(C.c_void_p), len(sv),
                                         0.05, 0.5, 1e-12, 200, n_out, ids.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), C.byref(it)))
    return ids, sc.view(np.int64), np.int64(it.value)


def test_combined_ranked_calls_equal_their_solo_calls(fused):
    idx, g, Q, phrases, doc = fused
    n = doc.shape[1]

    def moved(before):
        now = idx.combine_stats()
        return now["batches"] - before["batches"], now["queries"] - before["queries"]
    try:
        solo = [_index_ppr_ranked(idx, g, Q[i], phrases[i], n) for i in range(16)]
        for i in range(16):
            _check(solo[i][0], solo[i][1].view(np.float64), doc[i], what=("solo", i))
        idx.set_option("combine", 16)
        idx.set_option("combine_wait_us", LONG_US)
        before = idx.combine_stats()
        got = _run([lambda i=i: _index_ppr_ranked(idx, g, Q[i], phrases[i], n) for i in range(16)])
        for i in range(16):
            assert not isinstance(got[i], Exception), repr(got[i])
            for a, b in zip(got[i], solo[i]):
                assert np.array_equal(a, b), i
        assert moved(before) == (1, 16)
        # another n_out is another key: two callers of either, width 2 -> two batches that fill
        idx.set_option("combine", 2)
        before = idx.combine_stats()
        got = _run([lambda i=i: _index_ppr_ranked(idx, g, Q[i % 2], phrases[i % 2], n if i < 2 else 20) for i in range(4)])
        for i in range(4):
            assert not isinstance(got[i], Exception), repr(got[i])
            m = n if i < 2 else 20
            assert np.array_equal(got[i][0], solo[i % 2][0][:m]) and np.array_equal(got[i][1], solo[i % 2][1][:m])
        assert moved(before) == (2, 4)
    finally:
        idx.set_option("combine_wait_us", 0)
        idx.set_option("combine", 0)


# ---- 7. a row-sharded index: reset vectors on the host, the graph-ranked entry
def test_two_logical_shards_equal_one_dense_index():
    from comorag_amd.index import DenseIndex
    from comorag_amd.multi_index import MultiDeviceIndex
    from comorag_amd.ppr import DeviceGraph, ppr_passage_ranked, ppr_passage_ranked_batch, ppr_passage_scores_batch
    X, Q, nv, passage_vertex, src, dst, w, phrases = _fused_case()
    one = DenseIndex(X.shape[1], "f32"); one.append(X)
    two = MultiDeviceIndex(X.shape[1], "f32", devices=[0, 0], options={"append_block_rows": 1024}); two.append(X)
    assert hasattr(two, "n_shards")
    g = DeviceGraph(nv, src, dst, w); g.set_passage_vertices(passage_vertex)
    doc = ppr_passage_scores_batch(two, g, Q[:7], phrases[:7], 0.05)
    ids2, sc2 = ppr_passage_ranked_batch(two, g, Q[:7], phrases[:7], 0.05)
    ids1, sc1 = ppr_passage_ranked_batch(one, g, Q[:7], phrases[:7], 0.05)
    for b in range(7):
        _check(ids2[b], sc2[b], doc[b], what=("two shards", b))
    assert np.array_equal(ids2, ids1) and np.array_equal(sc2.view(np.int64), sc1.view(np.int64))
    a, b = ppr_passage_ranked(two, g, Q[2], phrases[2], 0.05, n_out=20)
    assert np.array_equal(a, ids1[2][:20]) and np.array_equal(b.view(np.int64), sc1[2][:20].view(np.int64))
    one.close(); two.close(); g.close()
