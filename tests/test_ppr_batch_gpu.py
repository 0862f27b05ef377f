"""Batched personalised PageRank on the device: a batch returns, bit for bit, what the same queries return one by one
(cmr_graph_ppr_batch vs cmr_graph_ppr, cmr_index_ppr_batch vs cmr_index_ppr), and each row stays within the single call's tolerance of
the oracle.  CPU twin (argument checks, Python glue): tests/test_ppr_batch_host.py."""
import numpy as np
import pytest

from oracle import ppr_np
from oracle import retrieval_np as orc

BATCHES = (1, 2, 3, 5, 8, 11, 16)


def _random_graph(n, m, seed, isolated=()):
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, m); dst = rng.integers(0, n, m)
    keep = (src != dst) & ~np.isin(src, isolated) & ~np.isin(dst, isolated)
    w = rng.uniform(0.1, 2.0, m)
    return src[keep].astype(np.int32), dst[keep].astype(np.int32), w[keep]


def _degree_class_graph():
    """The graph of test_ppr.py::test_device_ppr_degree_classes_hub_medium_and_short_rows."""
    rng = np.random.default_rng(4242)
    n = 2600
    src, dst = [], []
    for h, fan in zip((7, 1901), (1500, 300)):
        nb = rng.choice(np.setdiff1d(np.arange(n), [h, 11, 12, 13]), fan, replace=False)
        src += [h] * fan; dst += nb.tolist()
    med = rng.choice(np.arange(20, n), 120, replace=False)
    for v in med:
        nb = rng.choice(np.setdiff1d(np.arange(n), [v, 11, 12, 13]), int(rng.integers(6, 41)), replace=False)
        src += [int(v)] * len(nb); dst += nb.tolist()
    src += [5, 5, 5, 5, 6, 6, 6, 6, 6, 3, 3, 9]
    dst += [1, 2, 4, 8, 1, 2, 4, 8, 10, 4, 4, 9]
    src, dst = np.array(src, np.int32), np.array(dst, np.int32)
    return n, src, dst, rng.uniform(0.2, 2.0, len(src))


def _graph(kind):
    if kind == "degree_classes":
        return _degree_class_graph()
    if kind == "all_medium":
        n = 12; src, dst = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], np.int32).T
    elif kind == "all_short":
        n = 40; src = np.arange(n, dtype=np.int32); dst = ((src + 1) % n).astype(np.int32)
    elif kind == "one_hub_only":
        n = 401; src = np.zeros(400, np.int32); dst = np.arange(1, 401, dtype=np.int32)
    elif kind == "two_vertices":
        return 2, np.array([0], np.int32), np.array([1], np.int32), np.array([1.0])
    else:
        n = 100_000
        return (n,) + _random_graph(n, 600_000, n)
    w = np.random.default_rng(len(src)).uniform(0.5, 1.5, len(src))
    return n, np.ascontiguousarray(src), np.ascontiguousarray(dst), w


def _resets(n, B, seed):
    """B different reset rows: sparse positive rows with a negative and a NaN entry, an all-zero row (-> uniform), a single-vertex row,
    a seed on vertex 11 (isolated in the degree-class graph)."""
    rng = np.random.default_rng(seed)
    R = np.where(rng.uniform(0, 1, (B, n)) < 0.1, rng.uniform(0, 1, (B, n)), 0.0)
    R[:, 0] = rng.uniform(0.1, 1.0, B)
    if n > 2:
        R[:, 1] = -0.5
        R[::2, 2] = np.nan
    if n > 11:
        R[:, 11] = 0.4
    if B > 1:
        R[1] = 0.0
    if B > 2:
        R[2] = 0.0; R[2, n // 2] = 3.0
    return R


def _oracle(n, src, dst, w, reset, damping):
    if n <= 3000:
        return ppr_np.personalized_pagerank(n, src, dst, w, reset, damping)
    import scipy.sparse as sp                     # the large-size check of test_ppr.py: sparse power iteration in fp64
    W = sp.coo_matrix((np.concatenate([w, w]), (np.concatenate([src, dst]), np.concatenate([dst, src]))), shape=(n, n)).tocsr()
    s = np.asarray(W.sum(axis=1)).ravel()
    r = np.where(np.isnan(reset) | (reset < 0), 0, reset)
    r = r / r.sum() if r.sum() > 0 else np.full(n, 1.0 / n)
    x = r.copy()
    inv = np.where(s > 0, 1.0 / np.where(s > 0, s, 1), 0.0)
    steps = int(np.ceil(np.log(1e-13) / np.log(damping)))
    for _ in range(steps):
        x = damping * (W.T @ (x * inv) + x[s == 0].sum() * r) + (1 - damping) * r
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["degree_classes", "all_medium", "all_short", "one_hub_only", "two_vertices", "random_100k"])
def test_graph_ppr_batch_equals_the_single_call_bit_for_bit(kind):
    from comorag_amd.ppr import DeviceGraph
    n, src, dst, w = _graph(kind)
    g = DeviceGraph(n, src, dst, w)
    for damping, tol in ((0.5, 1e-12), (0.85, 1e-13)):
        R = _resets(n, 16, seed=n + int(damping * 100))
        single = np.stack([g.ppr(R[b], damping=damping, tol=tol) for b in range(16)])
        for B in BATCHES:
            got = g.ppr_batch(R[:B], damping=damping, tol=tol)
            assert got.shape == (B, n)
            for b in range(B):
                assert np.array_equal(got[b], single[b]), (kind, damping, B, b, float(np.abs(got[b] - single[b]).max()))
            assert np.array_equal(g.ppr_batch(R[:B], damping=damping, tol=tol), got), (kind, damping, B, "replay")
        # rows in another order and another position of the batch: a row's result does not depend on its neighbours
        perm = np.random.default_rng(3).permutation(16)
        assert np.array_equal(g.ppr_batch(R[perm], damping=damping, tol=tol), single[perm])
    g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,atol", [("degree_classes", 2e-11), ("all_medium", 1e-10), ("all_short", 1e-10), ("one_hub_only", 1e-10),
                                       ("two_vertices", 1e-10), ("random_100k", 1e-10)])
def test_graph_ppr_batch_against_the_oracle(kind, atol):
    from comorag_amd.ppr import DeviceGraph
    n, src, dst, w = _graph(kind)
    g = DeviceGraph(n, src, dst, w)
    B = 5 if n > 3000 else 11
    for damping in (0.5, 0.85):
        R = _resets(n, B, seed=n + 7)
        got = g.ppr_batch(R, damping=damping, tol=1e-13)
        for b in range(B):
            want = _oracle(n, src, dst, w, R[b], damping)
            np.testing.assert_allclose(got[b], want, atol=atol, rtol=0)
            assert abs(got[b].sum() - 1.0) < 1e-9
    g.close()


def _fused_case(dtype, n_pass=5000, n_ent=1500, d=128, nq=20):
    """The 5000-passage case of test_ppr.py::test_fused_dpr_seeded_ppr_equals_the_reference_pipeline."""
    X = orc.synthetic_corpus(n_pass, d, seed=8); Q = orc.synthetic_queries(nq, d, seed=9, planted=X)
    rng = np.random.default_rng(10)
    nv = n_ent + n_pass
    passage_vertex = (n_ent + rng.permutation(n_pass)).astype(np.int32)
    src = np.concatenate([rng.integers(0, n_ent, 3 * n_pass), rng.integers(0, n_ent, 2000)]).astype(np.int32)
    dst = np.concatenate([np.repeat(passage_vertex, 3), rng.integers(0, n_ent, 2000)]).astype(np.int32)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    w = rng.uniform(0.5, 1.5, len(src))
    phrases = []
    for b in range(nq):
        if b % 5 == 1:
            phrases.append(None)                                                     # an empty seed list
        elif b % 5 == 3:
            phrases.append((np.array([3, 9, 3, 3], np.int32), np.array([0.25, 0.5, 0.125, 0.0625])))      # duplicated seed vertices
        else:
            ph = np.zeros(nv); ph[rng.integers(0, n_ent, 6)] = rng.uniform(0.2, 1.0, 6); phrases.append(ph)
    return X, Q, nv, passage_vertex, src, dst, w, phrases


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_batch_equals_the_fused_single_call_bit_for_bit(dtype):
    from comorag_amd.index import DenseIndex
    from comorag_amd.ppr import DeviceGraph, ppr_passage_ranking_batch, ppr_passage_scores, ppr_passage_scores_batch
    X, Q, nv, passage_vertex, src, dst, w, phrases = _fused_case(dtype)
    idx = DenseIndex(X.shape[1], dtype); idx.append(X)
    g = DeviceGraph(nv, src, dst, w); g.set_passage_vertices(passage_vertex)
    single = [ppr_passage_scores(idx, g, Q[b], phrases[b], 0.05) for b in range(20)]
    for B in (2, 7, 16, 20):
        got = ppr_passage_scores_batch(idx, g, Q[:B], phrases[:B], 0.05)
        assert got.shape == (B, len(X))
        for b in range(B):
            assert np.array_equal(got[b], single[b]), (dtype, B, b, float(np.abs(got[b] - single[b]).max()))
    rnd = orc.bf16_round if dtype == "bf16" else (lambda a: a)
    ranked = ppr_passage_ranking_batch(idx, g, Q[:3], phrases[:3], 0.05)
    for b in range(3):
        ids, sc = orc.dense_passage_retrieval(rnd(X), rnd(Q[b:b + 1]))
        ph = np.zeros(nv) if phrases[b] is None else phrases[b]
        node_w = ph + ppr_np.passage_weights(ids, sc, passage_vertex, nv, 0.05)
        want = ppr_np.personalized_pagerank(nv, src, dst, w, node_w, 0.5)[passage_vertex]
        assert ranked[b][0][:20].tolist() == np.argsort(want)[::-1][:20].tolist()
        np.testing.assert_allclose(ranked[b][1], np.sort(want)[::-1], atol=1e-6 * want.max(), rtol=0)
    idx.close(); g.close()


@pytest.mark.gpu
def test_fused_batch_through_a_two_shard_index_equals_its_single_call():
    from comorag_amd.multi_index import MultiDeviceIndex
    from comorag_amd.ppr import DeviceGraph, ppr_passage_scores, ppr_passage_scores_batch
    X, Q, nv, passage_vertex, src, dst, w, phrases = _fused_case("f32")
    idx = MultiDeviceIndex(X.shape[1], "f32", devices=[0, 0], options={"append_block_rows": 1024})
    idx.append(X)
    assert hasattr(idx, "n_shards")
    g = DeviceGraph(nv, src, dst, w); g.set_passage_vertices(passage_vertex)
    # the scores reach the host branch through index.scores: one [B, N] call in the batch, [1, N] calls one by one — the branch is
    # bit-equal to its single twin exactly when that route is
    S = idx.scores(Q[:7])
    rows_equal = all(np.array_equal(S[b], idx.scores(Q[b:b + 1])[0]) for b in range(7))
    got = ppr_passage_scores_batch(idx, g, Q[:7], phrases[:7], 0.05)
    for b in range(7):
        one = ppr_passage_scores(idx, g, Q[b], phrases[b], 0.05)
        print(f"shard row {b}: scores rows equal {rows_equal}, max |batch - single| = {np.abs(got[b] - one).max():.3e}")
        assert np.array_equal(got[b], one), (b, rows_equal)
    idx.close(); g.close()


@pytest.mark.gpu
def test_a_nan_query_fails_the_whole_batch_and_the_next_batch_is_clean():
    from comorag_amd import _lib as L
    from comorag_amd.index import DenseIndex
    from comorag_amd.ppr import DeviceGraph, ppr_passage_scores_batch
    X, Q, nv, passage_vertex, src, dst, w, phrases = _fused_case("f32", nq=8)
    idx = DenseIndex(X.shape[1], "f32"); idx.append(X)
    g = DeviceGraph(nv, src, dst, w); g.set_passage_vertices(passage_vertex)
    before = ppr_passage_scores_batch(idx, g, Q, phrases, 0.05)
    bad = Q.copy(); bad[3, 5] = np.nan
    with pytest.raises(L.CmrError) as e:
        ppr_passage_scores_batch(idx, g, bad, phrases, 0.05)
    assert e.value.code == L.CMR_ERR_NONFINITE
    assert np.array_equal(ppr_passage_scores_batch(idx, g, Q, phrases, 0.05), before)
    idx.close(); g.close()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_concurrent_batches_and_single_calls_on_one_graph_do_not_share_scratch():
    """Four threads issue batches of four different queries on ONE graph and ONE index, ten rounds each, while two more threads issue
    single calls (both entry points): every result equals its solo value bit for bit."""
    import threading
    from comorag_amd.index import DenseIndex
    from comorag_amd.ppr import DeviceGraph, ppr_passage_scores, ppr_passage_scores_batch
    n_pass, n_ent, d = 4000, 1000, 64
    X = orc.synthetic_corpus(n_pass, d, seed=21); Q = orc.synthetic_queries(18, d, seed=22, planted=X)
    rng = np.random.default_rng(23)
    nv = n_ent + n_pass
    passage_vertex = (n_ent + rng.permutation(n_pass)).astype(np.int32)
    src = np.concatenate([rng.integers(0, n_ent, 3 * n_pass), rng.integers(0, n_ent, 1500)]).astype(np.int32)
    dst = np.concatenate([np.repeat(passage_vertex, 3), rng.integers(0, n_ent, 1500)]).astype(np.int32)
    keep = src != dst
    src, dst = src[keep], dst[keep]
    idx = DenseIndex(d, "f32"); idx.append(X)
    g = DeviceGraph(nv, src, dst, rng.uniform(0.5, 1.5, len(src))); g.set_passage_vertices(passage_vertex)
    phrases, resets = [], []
    for t in range(18):
        ph = np.zeros(nv); ph[rng.integers(0, n_ent, 5)] = rng.uniform(0.2, 1.0, 5); phrases.append(ph)
        rs = np.zeros(nv); rs[rng.integers(0, nv, 20)] = rng.uniform(0.1, 1.0, 20); resets.append(rs)
    solo_a = [ppr_passage_scores(idx, g, Q[t], phrases[t], 0.05) for t in range(18)]
    solo_b = [g.ppr(resets[t]) for t in range(18)]
    bad = []

    def batch_worker(t):
        sel = list(range(4 * t, 4 * t + 4))
        for it in range(10):
            a = ppr_passage_scores_batch(idx, g, Q[sel], [phrases[i] for i in sel], 0.05)
            b = g.ppr_batch(np.stack([resets[i] for i in sel]))
            if not all(np.array_equal(a[k], solo_a[i]) and np.array_equal(b[k], solo_b[i]) for k, i in enumerate(sel)):
                bad.append(("batch", t, it))

    def single_worker(t):
        for it in range(10):
            a = ppr_passage_scores(idx, g, Q[t], phrases[t], 0.05)
            b = g.ppr(resets[t])
            if not (np.array_equal(a, solo_a[t]) and np.array_equal(b, solo_b[t])):
                bad.append(("single", t, it))
    th = [threading.Thread(target=batch_worker, args=(t,)) for t in range(4)] + [threading.Thread(target=single_worker, args=(t,)) for t in (16, 17)]
    for x in th: x.start()
    for x in th: x.join()
    assert not bad, bad[:5]
    idx.close(); g.close()


@pytest.mark.gpu
def test_batch_hook_equals_three_single_hook_calls(golden_dir):
    """The Rag stand-in of test_ppr.py::test_hooks_put_run_ppr_and_graph_search_on_the_device: three calls through
    graph_search_with_fact_entities_batch equal the three single calls (ids identical, scores array_equal)."""
    import os, sys, types
    from comorag_amd import hooks
    from comorag_amd.ppr import DeviceGraph
    gd = np.load(os.path.join(golden_dir, "dpr_mid.npz"))
    X, F, Q = gd["X"], gd["F"], gd["Q"]
    n_ent = 40
    rng = np.random.default_rng(3)
    src = rng.integers(0, n_ent, 4 * len(X)).tolist(); dst = (n_ent + np.repeat(np.arange(len(X)), 4)).tolist()
    w = rng.uniform(0.5, 1.5, len(src)).tolist()
    names = [f"entity-{i}" for i in range(n_ent)] + [f"chunk-{i}" for i in range(len(X))]

    class G:
        vs = {"name": names}
        es = {"weight": w}
        def vcount(self): return len(names)
        def get_edgelist(self): return list(zip(src, dst))

    class Enc:
        def batch_encode(self, text, **kw): return Q[int(text[1:]):int(text[1:]) + 1]

    class Rag:
        def __init__(self):
            self.global_config = types.SimpleNamespace(need_cluster=False, index_dtype="f32")
            self.embedding_model, self.graph, self.ready_to_retrieve = Enc(), G(), False
            self.node_name_to_vertex_idx = {n: i for i, n in enumerate(names)}
            self.ent_node_to_num_chunk = {f"entity-{i}": 1 + i % 2 for i in range(n_ent)}
        def prepare_retrieval_objects(self):
            self.query_to_embedding = {"triple": {}, "passage": {}}
            self.passage_embeddings, self.fact_embeddings = X, F
            self.passage_node_idxs = list(range(n_ent, n_ent + len(X)))
            self.ready_to_retrieve = True
        def run_ppr(self, reset_prob, damping=0.5): raise AssertionError("the reference path must not run")
        def graph_search_with_fact_entities(self, *a, **k): raise AssertionError("the reference path must not run")
        def get_top_k_weights(self, link_top_k, w_, m_): return w_, m_

    mod = sys.modules[Rag.__module__]
    mod.get_query_instruction = lambda k: k
    mod.compute_mdhash_id = lambda content, prefix="": prefix + content
    rag = hooks.install(Rag(), patch_module_functions=False)
    rag.prepare_retrieval_objects()
    assert isinstance(rag._hip["graph"], DeviceGraph)
    calls = [("q1", 0, rag.get_fact_scores("q1"), [("1", "rel", "5"), ("7", "rel", "9")], [0, 1]),
             ("q0", 0, rag.get_fact_scores("q0"), [], []),
             ("q2", 0, rag.get_fact_scores("q2"), [("3", "rel", "3"), ("12", "rel", "30")], [2, 0], 0.05)]
    single = [rag.graph_search_with_fact_entities(*c) for c in calls]
    got = rag.graph_search_with_fact_entities_batch(calls)
    assert len(got) == 3
    for (ids, sc, used), (ids1, sc1, used1) in zip(got, single):
        assert ids.tolist() == ids1.tolist() and used == used1
        assert np.array_equal(sc, sc1)
    rag._hip["graph"].close()
