"""The PageRank passage ranking, CPU tier: the three ranked C-ABI symbols exist and check their arguments before any device call; the
selection logic of comorag_amd.ppr and comorag_amd.hooks — host lines below DEVICE_RANK_MIN_ROWS and for every graph object without
`ppr_ranked_batch`, the ranked entry from the threshold up — on the numpy stand-ins of tests/test_ppr_batch_host.py (GPU twin:
tests/test_ppr_rank_gpu.py)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

from comorag_amd import _lib as L
from oracle import ppr_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANKED = ("cmr_index_ppr_ranked", "cmr_index_ppr_ranked_batch", "cmr_graph_ppr_ranked_batch")


def _err():
    return L.lib().cmr_last_error().decode()


def test_ranked_symbols_are_exported_bound_and_cite_the_reference():
    lib = L.lib()
    hdr = open(os.path.join(ROOT, "include", "comorag_hip.h")).read()
    for s in RANKED:
        assert hasattr(lib, s) and s in L.SIGNATURES
        assert f"int32_t {s}(" in hdr
    assert hdr.count("ComoRAG.py:1101-1105") >= 1 and lib.cmr_abi_version() == 2
    assert f"#define CMR_PPR_RANK_TILE {L.CMR_PPR_RANK_TILE}\n" in hdr


def test_ranked_entry_points_check_their_arguments_without_a_device():
    """NULL handles and pointers, nb and n_out are judged before a handle is dereferenced: `fake` is a non-NULL pointer to zeros (as a graph
    it has no passage map), never a real handle."""
    lib = L.lib()
    buf = np.zeros(512, np.float64)
    fake = C.c_void_p(buf.ctypes.data)
    p = np.zeros(64, np.float64).ctypes.data_as(C.c_void_p)
    it = C.c_int32(0)
    asc = np.zeros(18, np.int32).ctypes.data_as(C.c_void_p)

    def graph(g, reset, nb, n_out, ids, sc):
        return lib.cmr_graph_ppr_ranked_batch(g, reset, nb, 0.5, 1e-12, 200, n_out, ids, sc, C.byref(it))
    assert graph(None, p, 1, 1, p, p) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert graph(fake, None, 1, 1, p, p) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert graph(fake, p, 1, 1, None, p) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert graph(fake, p, 1, 1, p, None) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert graph(fake, p, 0, 1, p, p) == L.CMR_ERR_INVALID and "nb" in _err()
    assert graph(fake, p, 17, 1, p, p) == L.CMR_ERR_UNSUPPORTED and "CMR_PPR_MAX_BATCH" in _err()
    assert graph(fake, p, 2, 0, p, p) == L.CMR_ERR_INVALID and "n_out" in _err()
    assert graph(fake, p, 2, -5, p, p) == L.CMR_ERR_INVALID and "n_out" in _err()
    assert graph(fake, p, 2, 3, p, p) == L.CMR_ERR_INVALID and "cmr_graph_set_passage_vertices" in _err()

    def batch(idx, g, nb, n_out, ids, sc, off=asc):
        return lib.cmr_index_ppr_ranked_batch(idx, g, p, nb, off, p, p, 0.05, 0.5, 1e-12, 200, n_out, ids, sc, C.byref(it))
    assert batch(None, fake, 2, 1, p, p) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert batch(fake, None, 2, 1, p, p) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert batch(fake, fake, 2, 1, None, p) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert batch(fake, fake, 2, 1, p, None) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert batch(fake, fake, 2, 1, p, p, off=None) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert batch(fake, fake, 0, 1, p, p) == L.CMR_ERR_INVALID and "nb" in _err()
    assert batch(fake, fake, 17, 1, p, p) == L.CMR_ERR_UNSUPPORTED and "CMR_PPR_MAX_BATCH" in _err()
    assert batch(fake, fake, 2, 0, p, p) == L.CMR_ERR_INVALID and "n_out" in _err()

    def single(idx, g, n_out, ids, sc, n_seeds=0):
        return lib.cmr_index_ppr_ranked(idx, g, p, p, p, n_seeds, 0.05, 0.5, 1e-12, 200, n_out, ids, sc, C.byref(it))
    assert single(None, None, 1, p, p) == L.CMR_ERR_INVALID and "NULL" in _err()
    assert single(None, None, 1, p, p, n_seeds=-1) == L.CMR_ERR_INVALID


class _OracleGraph:
    """_OracleGraph of tests/test_ppr_batch_host.py: DeviceGraph's UNRANKED call surface with the oracle's arithmetic."""

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


class _RankedGraph(_OracleGraph):
    """... plus DeviceGraph.ppr_ranked_batch by its contract: the stable descending order of pagerank[passage vertices]."""

    def __init__(self, *a):
        super().__init__(*a)
        self.ranked_calls = []

    def ppr_ranked_batch(self, resets, n_out=None, damping=0.5, tol=1e-12, max_iter=200):
        self.ranked_calls.append((len(resets), n_out))
        doc = self.ppr_batch(resets, damping)[:, self.passage_vertices]
        ids = np.stack([np.argsort(-d, kind="stable")[:n_out] for d in doc]).astype(np.int64)
        return ids, np.take_along_axis(doc, ids, axis=1)


def _row_by_row(numpy_index_cls):
    class Idx(numpy_index_cls):        # a BLAS product may round a row differently at another batch size (tests/test_ppr_batch_host.py)
        def scores(self, q):
            q = np.asarray(q, np.float32).reshape(-1, self.dim)
            return np.stack([(self._x @ r).astype(np.float32) for r in q])
    return Idx


def _case(numpy_index_cls, graph_cls, n_pass=60, n_ent=25, d=16, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n_pass, d)).astype(np.float32); X /= np.linalg.norm(X, axis=1, keepdims=True)
    nv = n_ent + n_pass
    pv = (n_ent + rng.permutation(n_pass)).astype(np.int32)
    src = np.concatenate([rng.integers(0, n_ent, 3 * n_pass), rng.integers(0, n_ent, 30)])
    dst = np.concatenate([np.repeat(pv, 3), rng.integers(0, n_ent, 30)])
    keep = src != dst
    g = graph_cls(nv, src[keep], dst[keep], rng.uniform(0.5, 1.5, int(keep.sum())))
    g.set_passage_vertices(pv)
    idx = _row_by_row(numpy_index_cls)(d); idx.append(X)
    Q = rng.standard_normal((20, d)).astype(np.float32)
    pws = []
    for b in range(20):
        ph = np.zeros(nv); ph[rng.integers(0, n_ent, 4)] = rng.uniform(0.2, 1.0, 4)
        pws.append(None if b % 4 == 0 else ph)
    return idx, g, Q, pws


def _host_lines(doc):
    ids = np.argsort(doc)[::-1]
    return ids, doc[ids.tolist()]


def test_the_shipped_threshold():
    """None (the switch is off until the crossover is measured) or the measured crossover: a multiple of 1024, never below 8192."""
    from comorag_amd import ppr
    thr = ppr.DEVICE_RANK_MIN_ROWS
    assert thr is None or (thr >= 8192 and thr % 1024 == 0)
    assert not ppr._device_rank(types.SimpleNamespace(ppr_ranked_batch=None), 5000)
    if thr is None:
        assert not ppr._device_rank(types.SimpleNamespace(ppr_ranked_batch=None), 10**9)


def test_a_graph_without_the_ranked_method_always_takes_the_host_lines(numpy_index_cls, monkeypatch):
    from comorag_amd import ppr
    idx, g, Q, pws = _case(numpy_index_cls, _OracleGraph)
    monkeypatch.setattr(ppr, "DEVICE_RANK_MIN_ROWS", 0)       # even with every size above the threshold
    doc = ppr.ppr_passage_scores_batch(idx, g, Q[:5], pws[:5], 0.05)
    for b in range(5):
        ids, sc = ppr.ppr_passage_ranking(idx, g, Q[b], pws[b], 0.05)
        hi, hs = _host_lines(doc[b])
        assert ids.dtype == np.int64 and sc.dtype == np.float64 and len(ids) == len(sc) == g.n_rows
        assert np.array_equal(ids, hi) and np.array_equal(sc, hs)
    for (ids, sc), d in zip(ppr.ppr_passage_ranking_batch(idx, g, Q[:5], pws[:5], 0.05), doc):
        assert np.array_equal(ids, _host_lines(d)[0]) and np.array_equal(sc, _host_lines(d)[1])
    rs = np.zeros(g.n_vertices); rs[3] = 1.0
    ids, sc = ppr.run_ppr(g, rs, g.passage_vertices.tolist(), 0.5)
    assert np.array_equal(ids, _host_lines(g.ppr(rs)[g.passage_vertices])[0])


def test_the_threshold_selects_the_ranked_entry(numpy_index_cls, monkeypatch):
    from comorag_amd import ppr
    idx, g, Q, pws = _case(numpy_index_cls, _RankedGraph)
    doc = ppr.ppr_passage_scores_batch(idx, g, Q, pws, 0.05)
    # below the shipped threshold: today's lines, the ranked method is not touched
    for b in range(3):
        ids, sc = ppr.ppr_passage_ranking(idx, g, Q[b], pws[b], 0.05)
        assert np.array_equal(ids, _host_lines(doc[b])[0]) and np.array_equal(sc, _host_lines(doc[b])[1])
    got = ppr.ppr_passage_ranking_batch(idx, g, Q[:3], pws[:3], 0.05)
    assert all(np.array_equal(got[b][0], _host_lines(doc[b])[0]) for b in range(3))
    rs = np.zeros(g.n_vertices); rs[3] = 1.0
    ppr.run_ppr(g, rs, g.passage_vertices.tolist(), 0.5)
    assert g.ranked_calls == []
    # one row below / at the threshold
    for thr, ranked in ((g.n_rows + 1, False), (g.n_rows, True)):
        monkeypatch.setattr(ppr, "DEVICE_RANK_MIN_ROWS", thr)
        g.ranked_calls.clear()
        ids, sc = ppr.ppr_passage_ranking(idx, g, Q[0], pws[0], 0.05)
        assert bool(g.ranked_calls) == ranked
        assert ids.dtype == np.int64 and sc.dtype == np.float64 and ids.shape == sc.shape == (g.n_rows,)
    # from the threshold up: score descending, equal scores by ascending row; the batch hands ONE call to the graph
    g.ranked_calls.clear()
    got = ppr.ppr_passage_ranking_batch(idx, g, Q, pws, 0.05)
    assert g.ranked_calls == [(20, g.n_rows)] and len(got) == 20
    for b in range(20):
        ids, sc = got[b]
        want = np.argsort(-doc[b], kind="stable")
        assert ids.dtype == np.int64 and sc.dtype == np.float64 and len(ids) == len(sc) == g.n_rows
        assert np.array_equal(ids, want) and np.array_equal(sc.view(np.int64), doc[b][want].view(np.int64))
    ids, sc = ppr.ppr_passage_ranked(idx, g, Q[1], pws[1], 0.05, n_out=7)
    assert ids.shape == sc.shape == (7,) and np.array_equal(ids, got[1][0][:7])
    ids, sc = ppr.ppr_passage_ranked_batch(idx, g, Q[:0], None, 0.05)
    assert ids.shape == sc.shape == (0, g.n_rows)
    for bad in (0, g.n_rows + 1):
        with pytest.raises(ValueError):
            ppr.ppr_passage_ranked(idx, g, Q[1], pws[1], 0.05, n_out=bad)
    g.ranked_calls.clear()
    ids, sc = ppr.run_ppr(g, rs, g.passage_vertices.tolist(), 0.5)
    assert g.ranked_calls == [(1, None)] and np.array_equal(ids, np.argsort(-g.ppr(rs)[g.passage_vertices], kind="stable"))
    g.ranked_calls.clear()                                      # another passage list than the graph's map: the host lines
    ids, sc = ppr.run_ppr(g, rs, g.passage_vertices[::-1].tolist(), 0.5)
    assert g.ranked_calls == [] and np.array_equal(ids, _host_lines(g.ppr(rs)[g.passage_vertices[::-1]])[0])


def _rag(numpy_index_cls, graph_cls, n_ent=40, n_pass=120, d=24):
    from comorag_amd import hooks
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n_pass, d)).astype(np.float32); X /= np.linalg.norm(X, axis=1, keepdims=True)
    F = rng.standard_normal((30, d)).astype(np.float32); F /= np.linalg.norm(F, axis=1, keepdims=True)
    Q = rng.standard_normal((10, d)).astype(np.float32)
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

    def factory(mat, dtype, device):
        ix = _row_by_row(numpy_index_cls)(np.asarray(mat).shape[1], dtype, device); ix.append(mat)
        return ix
    rag = hooks.install(Rag(), index_factory=factory, graph_factory=graph_cls.from_igraph, patch_module_functions=False)
    rag.prepare_retrieval_objects()
    calls = [(f"q{i}", 0, rag.get_fact_scores(f"q{i}"), [(str(i), "rel", str(i + 3))], [i % 5]) for i in range(4)]
    return rag, calls, n_pass


def test_hooks_rank_on_the_graph_from_the_threshold_up_and_assert_the_length(numpy_index_cls, monkeypatch):
    from comorag_amd import ppr
    rag, calls, n_pass = _rag(numpy_index_cls, _RankedGraph)
    g = rag._hip["graph"]
    below = [rag.graph_search_with_fact_entities(*c) for c in calls]
    below_b = rag.graph_search_with_fact_entities_batch(calls)
    assert g.ranked_calls == []                                 # the shipped threshold: the host lines
    monkeypatch.setattr(ppr, "DEVICE_RANK_MIN_ROWS", n_pass)
    above = [rag.graph_search_with_fact_entities(*c) for c in calls]
    assert g.ranked_calls == [(1, n_pass)] * 4
    above_b = rag.graph_search_with_fact_entities_batch(calls)
    assert g.ranked_calls[4:] == [(4, n_pass)]
    for lo, lob, hi, hib in zip(below, below_b, above, above_b):
        for ids, sc, used in (lo, lob, hi, hib):
            assert ids.dtype == np.int64 and sc.dtype == np.float64 and len(ids) == len(sc) == n_pass and used == lo[2]
        # (no ties in this case: both orders are THE descending order)
        assert np.array_equal(lo[0], hi[0]) and np.array_equal(lo[1], hi[1]) and np.array_equal(lob[0], hib[0]) and np.array_equal(hi[0], hib[0])
    ids, sc = rag.run_ppr(np.arange(g.n_vertices, dtype=np.float64))
    assert len(ids) == n_pass and g.ranked_calls[-1] == (1, None)
    # hooks' own assertion (ComoRAG.py:1105): a ranking that does not cover every passage is refused
    monkeypatch.setattr(_RankedGraph, "ppr_ranked_batch", lambda self, resets, n_out=None, **k: (np.zeros((len(resets), 5), np.int64), np.zeros((len(resets), 5))))
    with pytest.raises(AssertionError):
        rag.graph_search_with_fact_entities(*calls[0])
    with pytest.raises(AssertionError):
        rag.graph_search_with_fact_entities_batch(calls)
