"""Batched personalised PageRank, CPU tier: the two C-ABI symbols exist and check their arguments before any device call; the Python
layer (chunking, seed packing, the row-sharded host branch) and the batch hook give, call for call, what the single-query path gives —
against a graph stand-in whose `ppr_batch` is the oracle's solve row by row (GPU twin: tests/test_ppr_batch_gpu.py)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

from comorag_amd import _lib as L
from oracle import ppr_np


def _err():
    return L.lib().cmr_last_error().decode()


def test_batch_symbols_are_exported_and_bound():
    lib = L.lib()
    for s in ("cmr_graph_ppr_batch", "cmr_index_ppr_batch"):
        assert hasattr(lib, s) and s in L.SIGNATURES
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "comorag_hip.h")).read()
    assert "#define CMR_PPR_MAX_BATCH 16" in hdr and L.CMR_PPR_MAX_BATCH == 16
    assert lib.cmr_abi_version() == 2


def test_batch_entry_points_check_their_arguments_without_a_device():
    """Integers and pointers are judged before a handle is dereferenced: `fake` is a non-NULL pointer to zeros, never a real handle."""
    lib = L.lib()
    buf = np.zeros(64, np.float64)
    fake = C.c_void_p(buf.ctypes.data)
    p = buf.ctypes.data_as(C.c_void_p)
    it = C.c_int32(0)
    asc = np.zeros(18, np.int32).ctypes.data_as(C.c_void_p)
    desc = np.array([0, 3, 1], np.int32).ctypes.data_as(C.c_void_p)

    assert lib.cmr_graph_ppr_batch(None, p, 2, 0.5, 1e-12, 200, p, C.byref(it)) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert lib.cmr_graph_ppr_batch(fake, None, 2, 0.5, 1e-12, 200, p, C.byref(it)) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert lib.cmr_graph_ppr_batch(fake, p, 0, 0.5, 1e-12, 200, p, C.byref(it)) == L.CMR_ERR_INVALID and "nb" in _err()
    assert lib.cmr_graph_ppr_batch(fake, p, 17, 0.5, 1e-12, 200, p, C.byref(it)) == L.CMR_ERR_UNSUPPORTED and "CMR_PPR_MAX_BATCH" in _err()

    def fused(idx, g, nb, off):
        return lib.cmr_index_ppr_batch(idx, g, p, nb, off, p, p, 0.05, 0.5, 1e-12, 200, p, C.byref(it))
    assert fused(None, fake, 2, asc) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert fused(fake, None, 2, asc) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert fused(fake, fake, 2, None) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert fused(fake, fake, 0, asc) == L.CMR_ERR_INVALID and "nb" in _err()
    assert fused(fake, fake, -3, asc) == L.CMR_ERR_INVALID and "nb" in _err()
    assert fused(fake, fake, 17, asc) == L.CMR_ERR_UNSUPPORTED and "CMR_PPR_MAX_BATCH" in _err()
    assert fused(fake, fake, 2, desc) == L.CMR_ERR_INVALID and "ascending" in _err()


class _OracleGraph:
    """comorag_amd.ppr.DeviceGraph's call surface with the oracle's arithmetic; `ppr_batch` is `ppr` row by row."""

    def __init__(self, n, src, dst, w):
        self.n_vertices, self._src, self._dst, self._w = n, list(src), list(dst), list(w)
        self.batch_sizes = []

    @classmethod
    def from_igraph(cls, g, device=0):
        e = g.get_edgelist()
        return cls(g.vcount(), [a for a, _ in e], [b for _, b in e], list(g.es["weight"]))

    def set_passage_vertices(self, idxs):
        self.passage_vertices = np.asarray(idxs, np.int32); self.n_rows = len(idxs)

    def ppr(self, reset, damping=0.5, tol=1e-12, max_iter=200):
        return ppr_np.personalized_pagerank(self.n_vertices, self._src, self._dst, self._w, np.asarray(reset, np.float64), damping)

    def ppr_batch(self, resets, damping=0.5, tol=1e-12, max_iter=200):
        self.batch_sizes.append(len(resets))
        return np.stack([self.ppr(r, damping) for r in resets])


def _row_by_row(numpy_index_cls):
    class Idx(numpy_index_cls):        # a BLAS product may round a row differently at another batch size; the device index is pinned in the GPU tier
        def scores(self, q):
            q = np.asarray(q, np.float32).reshape(-1, self.dim)
            return np.stack([(self._x @ r).astype(np.float32) for r in q])
    return Idx


def _case(numpy_index_cls, n_pass=60, n_ent=25, d=16, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n_pass, d)).astype(np.float32); X /= np.linalg.norm(X, axis=1, keepdims=True)
    nv = n_ent + n_pass
    pv = (n_ent + rng.permutation(n_pass)).astype(np.int32)
    src = np.concatenate([rng.integers(0, n_ent, 3 * n_pass), rng.integers(0, n_ent, 30)])
    dst = np.concatenate([np.repeat(pv, 3), rng.integers(0, n_ent, 30)])
    keep = src != dst
    g = _OracleGraph(nv, src[keep], dst[keep], rng.uniform(0.5, 1.5, int(keep.sum())))
    g.set_passage_vertices(pv)
    idx = _row_by_row(numpy_index_cls)(d); idx.append(X)
    return rng, idx, g, nv, n_ent, d


def test_passage_scores_batch_equals_the_single_call_per_query(numpy_index_cls):
    from comorag_amd.ppr import ppr_passage_ranking, ppr_passage_ranking_batch, ppr_passage_scores, ppr_passage_scores_batch
    rng, idx, g, nv, n_ent, d = _case(numpy_index_cls)
    B = 37                                                      # three chunks of at most CMR_PPR_MAX_BATCH
    Q = rng.standard_normal((B, d)).astype(np.float32)
    pws = []
    for b in range(B):
        if b % 4 == 0:
            pws.append(None)                                    # no phrase at all: the reset vector is the passage part alone
        elif b % 4 == 1:
            pws.append((np.array([3, 9, 3, 3], np.int32), np.array([0.25, 0.5, 0.125, 0.0625])))      # duplicates add up
        else:
            ph = np.zeros(nv); ph[rng.integers(0, n_ent, 4)] = rng.uniform(0.2, 1.0, 4); pws.append(ph)
    got = ppr_passage_scores_batch(idx, g, Q, pws, 0.05)
    assert got.shape == (B, g.n_rows) and got.dtype == np.float64
    assert g.batch_sizes == [B]                                 # the host branch hands ONE batch to the graph (DeviceGraph.ppr_batch chunks)
    for b in range(B):
        np.testing.assert_array_equal(got[b], ppr_passage_scores(idx, g, Q[b], pws[b], 0.05))
    ranked = ppr_passage_ranking_batch(idx, g, Q[:5], pws[:5], 0.05)
    for b in range(5):
        ids, sc = ppr_passage_ranking(idx, g, Q[b], pws[b], 0.05)
        assert ranked[b][0].tolist() == ids.tolist()
        np.testing.assert_array_equal(ranked[b][1], sc)
    np.testing.assert_array_equal(ppr_passage_scores_batch(idx, g, Q[:3], None, 0.05), np.stack([ppr_passage_scores(idx, g, q, None, 0.05) for q in Q[:3]]))
    with pytest.raises(ValueError):
        ppr_passage_scores_batch(idx, g, Q[:3], pws[:2], 0.05)

    class NoBatch:                                              # a custom graph object without ppr_batch: its ppr, row by row
        n_vertices, passage_vertices, ppr = g.n_vertices, g.passage_vertices, staticmethod(g.ppr)
    np.testing.assert_array_equal(ppr_passage_scores_batch(idx, NoBatch(), Q[:4], pws[:4], 0.05), got[:4])


def test_batch_hook_equals_the_single_hook_call_for_call(numpy_index_cls):
    from comorag_amd import hooks
    rng = np.random.default_rng(7)
    n_ent, n_pass, d = 40, 120, 24
    X = rng.standard_normal((n_pass, d)).astype(np.float32); X /= np.linalg.norm(X, axis=1, keepdims=True)
    F = rng.standard_normal((30, d)).astype(np.float32); F /= np.linalg.norm(F, axis=1, keepdims=True)
    Q = rng.standard_normal((40, d)).astype(np.float32)
    src = rng.integers(0, n_ent, 4 * n_pass).tolist(); dst = (n_ent + np.repeat(np.arange(n_pass), 4)).tolist()
    w = rng.uniform(0.5, 1.5, len(src)).tolist()
    names = [f"entity-{i}" for i in range(n_ent)] + [f"chunk-{i}" for i in range(n_pass)]

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
            self.passage_node_idxs = list(range(n_ent, n_ent + n_pass))
            self.ready_to_retrieve = True
        def run_ppr(self, reset_prob, damping=0.5): raise AssertionError("the reference path must not run")
        def graph_search_with_fact_entities(self, *a, **k): raise AssertionError("the reference path must not run")
        def get_top_k_weights(self, link_top_k, w_, m_): return w_, m_

    mod = sys.modules[Rag.__module__]
    mod.get_query_instruction = lambda k: k
    mod.compute_mdhash_id = lambda content, prefix="": prefix + content
    Idx = _row_by_row(numpy_index_cls)

    def factory(mat, dtype, device):
        ix = Idx(np.asarray(mat).shape[1], dtype, device); ix.append(mat)
        return ix
    rag = hooks.install(Rag(), index_factory=factory, graph_factory=_OracleGraph.from_igraph, patch_module_functions=False)
    rag.prepare_retrieval_objects()
    g = rag._hip["graph"]
    assert isinstance(g, _OracleGraph)
    calls = []
    for i in range(37):
        fs = rag.get_fact_scores(f"q{i}")
        if i % 5 == 0:
            calls.append((f"q{i}", 0, fs, [], []))                                   # no phrase in the graph: the passage scores alone seed the walk
        elif i % 5 == 1:
            calls.append((f"q{i}", 0, fs, [("1", "rel", "5"), ("5", "rel", "1"), ("zzz", "rel", "9")], [0, 1, 2], 0.1))     # a phrase named twice, one unknown, another weight
        else:
            a, b, c = (int(x) for x in rng.integers(0, n_ent, 3))
            calls.append((f"q{i}", 0, fs, [(str(a), "rel", str(b)), (str(c), "rel", str(a))], [int(i % 7), int(i % 11)]))
    single = [rag.graph_search_with_fact_entities(*c) for c in calls]
    g.batch_sizes.clear()
    got = rag.graph_search_with_fact_entities_batch(calls)
    assert sorted(g.batch_sizes) == sorted([sum(1 for c in calls if len(c) > 5), sum(1 for c in calls if len(c) == 5)])      # one batch per passage_node_weight
    assert len(got) == len(calls)
    for (ids, sc, used), (ids1, sc1, used1) in zip(got, single):
        assert ids.tolist() == ids1.tolist() and used == used1
        np.testing.assert_array_equal(sc, sc1)
    assert rag.graph_search_with_fact_entities_batch([]) == []

    class OwnScores(_OracleGraph):                              # brings passage_scores and nothing batched: served call by call
        def passage_scores(self, index, q, phrase_w, pnw, damping):
            from comorag_amd.ppr import ppr_passage_scores
            return ppr_passage_scores(index, self, q, phrase_w, pnw, damping)
    rag2 = hooks.install(Rag(), index_factory=factory, graph_factory=OwnScores.from_igraph, patch_module_functions=False)
    rag2.prepare_retrieval_objects()
    got2 = rag2.graph_search_with_fact_entities_batch(calls[:6])
    assert rag2._hip["graph"].batch_sizes == []
    for (ids, sc, used), (ids1, sc1, used1) in zip(got2, single[:6]):
        assert ids.tolist() == ids1.tolist() and used == used1
        np.testing.assert_array_equal(sc, sc1)
