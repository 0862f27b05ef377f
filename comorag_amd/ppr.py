"""Device-side PPR seeding + personalised PageRank — host mirror of
ComoRAG.graph_search_with_fact_entities' passage loop (src/comorag/ComoRAG.py:1034-1045) and ComoRAG.run_ppr (:1086-1105).

The reference copies all N (passage id, normalised score) pairs to the host, scatters them one by one into a vertex
vector and hands that to igraph's prpack PageRank.  Here the graph lives in HBM as a CSR copy (`DeviceGraph`), and
`ppr_passage_scores` keeps scan -> min-max -> scatter -> power iteration -> gather on the device: only n_passages
doubles come back.  igraph itself is not needed (it is absent from this image): `DeviceGraph.from_igraph` only reads an
edge list + weights from anything that offers `vcount() / get_edgelist() / es['weight']`.
`ppr_passage_ranked(_batch)` / `DeviceGraph.ppr_ranked_batch` also rank the passages on the device (ComoRAG.py:1101-1105);
`run_ppr` and `ppr_passage_ranking(_batch)` switch to them at DEVICE_RANK_MIN_ROWS passage rows (None: never).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib as L

# From this many passage rows up the ranking of the PageRank scores (ComoRAG.py:1101-1105) runs on the device (cmr_*_ppr_ranked*, DESIGN
# §4.9c); below it the reference's two numpy lines run on the host, unchanged.  The measured crossover of `tools/ppr_batch_bench.py
# --rank`'s sweep (profiles/ppr_rank.json: the ranked call takes 1.14 of the host path at 4096 rows, 0.86 at 8192, 0.27 at 65536), rounded up
# to a multiple of 1024 and never below 8192.  None switches it off: run_ppr, ppr_passage_ranking(_batch) and the hooks then keep the host
# lines at every size.  From the threshold up, rows with equal fp64 scores come by ascending row, where numpy's argsort leaves their order
# unspecified; scores, and ids wherever scores differ, are the same.
DEVICE_RANK_MIN_ROWS: Optional[int] = 8192


def _n_out(n_out, n_rows: int) -> int:
    n = int(n_rows) if n_out is None else int(n_out)
    if not 1 <= n <= int(n_rows):
        raise ValueError(f"n_out must be in [1, {int(n_rows)}] (got {n})")
    return n


class DeviceGraph:
    def __init__(self, n_vertices: int, src, dst, weight=None, device: int = 0):
        src = np.ascontiguousarray(src, dtype=np.int32)
        dst = np.ascontiguousarray(dst, dtype=np.int32)
        if src.shape != dst.shape:
            raise ValueError("src / dst length mismatch")
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
        if w is not None and w.shape != src.shape:
            raise ValueError("weight length mismatch")
        self.n_vertices, self.device = int(n_vertices), int(device)
        self.n_rows = 0
        self._h = C.c_void_p()
        L.check(L.lib().cmr_graph_create(self.device, self.n_vertices, len(src), src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p),
                                         w.ctypes.data_as(C.c_void_p) if w is not None else None, C.byref(self._h)))

    @classmethod
    def from_igraph(cls, graph, device: int = 0, weight_attr: str = "weight"):
        """Anything with igraph's vcount() / get_edgelist() / es[attr] (ComoRAG.graph)."""
        edges = graph.get_edgelist()
        src = [e[0] for e in edges]
        dst = [e[1] for e in edges]
        try:
            w = list(graph.es[weight_attr]) if len(edges) else []
        except Exception:
            w = None
        return cls(graph.vcount(), src, dst, w, device=device)

    def set_passage_vertices(self, passage_node_idxs: Sequence[int]) -> None:
        v = np.ascontiguousarray(passage_node_idxs, dtype=np.int32)
        L.check(L.lib().cmr_graph_set_passage_vertices(self._h, v.ctypes.data_as(C.c_void_p), len(v)))
        self.n_rows = len(v)
        self.passage_vertices = v

    def ppr(self, reset, damping: float = 0.5, tol: float = 1e-12, max_iter: int = 200) -> np.ndarray:
        """personalized_pagerank(reset=...) over every vertex (negative / NaN reset entries count as 0)."""
        r = np.ascontiguousarray(reset, dtype=np.float64)
        if r.shape != (self.n_vertices,):
            raise ValueError(f"reset must have {self.n_vertices} entries")
        out = np.empty(self.n_vertices, dtype=np.float64)
        it = C.c_int32(0)
        L.check(L.lib().cmr_graph_ppr(self._h, r.ctypes.data_as(C.c_void_p), float(damping), float(tol), int(max_iter),
                                      out.ctypes.data_as(C.c_void_p), C.byref(it)))
        self.last_iters = it.value
        return out

    def ppr_batch(self, resets, damping: float = 0.5, tol: float = 1e-12, max_iter: int = 200) -> np.ndarray:
        """`ppr` for B reset vectors [B, n_vertices] at once -> [B, n_vertices]; row b is `ppr(resets[b])` bit for bit.  The device runs
        up to CMR_PPR_MAX_BATCH queries per power iteration (the graph is read once per step for all of them); larger B goes in chunks."""
        r = np.ascontiguousarray(resets, dtype=np.float64)
        if r.ndim != 2 or r.shape[1] != self.n_vertices:
            raise ValueError(f"resets must be [B, {self.n_vertices}]")
        out = np.empty(r.shape, dtype=np.float64)
        it = C.c_int32(0)
        for b0 in range(0, r.shape[0], L.CMR_PPR_MAX_BATCH):
            nb = min(L.CMR_PPR_MAX_BATCH, r.shape[0] - b0)
            L.check(L.lib().cmr_graph_ppr_batch(self._h, r[b0:b0 + nb].ctypes.data_as(C.c_void_p), nb, float(damping), float(tol), int(max_iter),
                                                out[b0:b0 + nb].ctypes.data_as(C.c_void_p), C.byref(it)))
            self.last_iters = it.value
        return out

    def ppr_ranked_batch(self, resets, n_out: Optional[int] = None, damping: float = 0.5, tol: float = 1e-12,
                         max_iter: int = 200) -> Tuple[np.ndarray, np.ndarray]:
        """`ppr_batch`, then pagerank[passage vertices] ranked on the device (ComoRAG.py:1101-1105): (ids [B, n_out] int64 passage rows,
        scores [B, n_out] float64), score descending, equal scores by ascending row; n_out = None: every row.  ids[b] equals
        np.argsort(-doc, kind="stable") and scores[b] equals doc[ids[b]] bit for bit, doc = ppr(resets[b])[passage vertices].  Needs
        `set_passage_vertices`; B above CMR_PPR_MAX_BATCH goes in chunks."""
        r = np.ascontiguousarray(resets, dtype=np.float64)
        if r.ndim != 2 or r.shape[1] != self.n_vertices:
            raise ValueError(f"resets must be [B, {self.n_vertices}]")
        n = _n_out(n_out, self.n_rows)
        ids = np.empty((r.shape[0], n), dtype=np.int64)
        sc = np.empty((r.shape[0], n), dtype=np.float64)
        it = C.c_int32(0)
        for b0 in range(0, r.shape[0], L.CMR_PPR_MAX_BATCH):
            nb = min(L.CMR_PPR_MAX_BATCH, r.shape[0] - b0)
            L.check(L.lib().cmr_graph_ppr_ranked_batch(self._h, r[b0:b0 + nb].ctypes.data_as(C.c_void_p), nb, float(damping), float(tol), int(max_iter), n,
                                                       ids[b0:b0 + nb].ctypes.data_as(C.c_void_p), sc[b0:b0 + nb].ctypes.data_as(C.c_void_p), C.byref(it)))
            self.last_iters = it.value
        return ids, sc

    def close(self) -> None:
        if getattr(self, "_h", None):
            L.lib().cmr_graph_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_ppr(graph: DeviceGraph, reset_prob, passage_node_idxs, damping: Optional[float] = 0.5) -> Tuple[np.ndarray, np.ndarray]:
    """ComoRAG.run_ppr (ComoRAG.py:1086-1105) with the PageRank itself on the device; the last three lines are the reference's."""
    if damping is None:
        damping = 0.5
    if _device_rank(graph, len(passage_node_idxs)) and np.array_equal(getattr(graph, "passage_vertices", None), np.asarray(passage_node_idxs)):
        ids, sc = graph.ppr_ranked_batch(np.asarray(reset_prob, dtype=np.float64)[None, :], damping=damping)
        return ids[0], sc[0]
    pagerank_scores = graph.ppr(np.asarray(reset_prob, dtype=np.float64), damping=damping)
    doc_scores = np.array([pagerank_scores[idx] for idx in passage_node_idxs])
    sorted_doc_ids = np.argsort(doc_scores)[::-1]
    sorted_doc_scores = doc_scores[sorted_doc_ids.tolist()]
    return sorted_doc_ids, sorted_doc_scores


def _seed_arrays(phrase_weights) -> Tuple[np.ndarray, np.ndarray]:
    """(vertices int32, weights float64) of one query's phrase weights, as the fused calls ship them."""
    if phrase_weights is None:
        return np.empty(0, np.int32), np.empty(0, np.float64)
    if isinstance(phrase_weights, tuple):
        return np.ascontiguousarray(phrase_weights[0], np.int32), np.ascontiguousarray(phrase_weights[1], np.float64)
    pw = np.asarray(phrase_weights, dtype=np.float64)
    sv = np.flatnonzero(pw != 0).astype(np.int32)
    return sv, np.ascontiguousarray(pw[sv])


def _device_rank(graph, n_rows: int) -> bool:
    """Rank on the device?  From DEVICE_RANK_MIN_ROWS passage rows up, for a graph object that can (the numpy stand-ins and custom graph
    objects without `ppr_ranked_batch` always take the host lines, as `_graph_ppr_batch` falls back)."""
    return DEVICE_RANK_MIN_ROWS is not None and n_rows >= DEVICE_RANK_MIN_ROWS and n_rows > 0 and hasattr(graph, "ppr_ranked_batch")


def _host_branch(index) -> bool:
    """A row-sharded index (MultiDeviceIndex) or any index without a device handle: its shards live on several devices, the graph on
    one — the N scores come to the host once (4 N bytes), the reset vector is built there, PageRank runs on the device."""
    return hasattr(index, "n_shards") or not hasattr(index, "_h")


def _host_reset(graph, scores, phrase_weights, passage_node_weight: float) -> np.ndarray:
    """One query's reset vector by the reference's own lines (ComoRAG.py:1034-1045): min-max, score x passage_node_weight into the
    passages' vertices, product in float64 as numpy 1.26 forms it."""
    from .utils.misc_utils import min_max_normalize
    norm = min_max_normalize(scores)
    reset = np.zeros(graph.n_vertices, dtype=np.float64)
    if phrase_weights is not None:
        if isinstance(phrase_weights, tuple):
            np.add.at(reset, np.asarray(phrase_weights[0], np.int64), np.asarray(phrase_weights[1], np.float64))
        else:
            reset += np.asarray(phrase_weights, dtype=np.float64)
    reset[graph.passage_vertices] += norm.astype(np.float64) * float(passage_node_weight)
    return reset


def ppr_passage_scores(index, graph: DeviceGraph, query_embedding, phrase_weights=None, passage_node_weight: float = 0.05,
                       damping: float = 0.5, tol: float = 1e-12, max_iter: int = 200) -> np.ndarray:
    """The fused path for one query: doc_scores[i] = pagerank[vertex of passage row i], with the DPR scores scattered into
    the reset vector on the device.  `phrase_weights`: dense [n_vertices] array (only its non-zero entries are shipped)
    or a (vertices, weights) pair.  `graph.set_passage_vertices(...)` must map every row of `index`."""
    q = np.ascontiguousarray(np.asarray(query_embedding, dtype=np.float32).reshape(-1))
    if _host_branch(index):
        reset = _host_reset(graph, index.scores(q[None, :])[0], phrase_weights, passage_node_weight)
        return graph.ppr(reset, damping=damping, tol=tol, max_iter=max_iter)[graph.passage_vertices]
    sv, sw = _seed_arrays(phrase_weights)
    out = np.empty(graph.n_rows, dtype=np.float64)
    it = C.c_int32(0)
    L.check(L.lib().cmr_index_ppr(index._h, graph._h, q.ctypes.data_as(C.c_void_p), sv.ctypes.data_as(C.c_void_p), sw.ctypes.data_as(C.c_void_p),
                                  len(sv), float(passage_node_weight), float(damping), float(tol), int(max_iter),
                                  out.ctypes.data_as(C.c_void_p), C.byref(it)))
    return out


def ppr_passage_ranking(index, graph: DeviceGraph, query_embedding, phrase_weights=None, passage_node_weight: float = 0.05,
                        damping: float = 0.5) -> Tuple[np.ndarray, np.ndarray]:
    """(sorted_doc_ids, sorted_doc_scores) exactly as ComoRAG.run_ppr returns them (ComoRAG.py:1101-1105); from DEVICE_RANK_MIN_ROWS
    passage rows up the device ranks (`ppr_passage_ranked`: equal scores by ascending row)."""
    if _device_rank(graph, getattr(graph, "n_rows", 0)):
        return ppr_passage_ranked(index, graph, query_embedding, phrase_weights, passage_node_weight, damping)
    doc_scores = ppr_passage_scores(index, graph, query_embedding, phrase_weights, passage_node_weight, damping)
    sorted_doc_ids = np.argsort(doc_scores)[::-1]
    return sorted_doc_ids, doc_scores[sorted_doc_ids.tolist()]


def ppr_passage_scores_batch(index, graph, query_embeddings, phrase_weights: Optional[Sequence] = None, passage_node_weight: float = 0.05,
                             damping: float = 0.5, tol: float = 1e-12, max_iter: int = 200) -> np.ndarray:
    """`ppr_passage_scores` for B queries [B, d] -> [B, n_rows]; row b is the single call's result for (Q[b], phrase_weights[b]) bit for
    bit.  `phrase_weights`: None, or one entry per query (dense array | (vertices, weights) | None).  The B power iterations run as one
    (ComoRAG.try_answer issues up to 16 graph searches at once, ComoRAG.py:432-453); B above CMR_PPR_MAX_BATCH goes in chunks."""
    Q = np.ascontiguousarray(np.asarray(query_embeddings, dtype=np.float32))
    if Q.ndim != 2:
        raise ValueError("query_embeddings must be [B, d]")
    B = Q.shape[0]
    pws = [None] * B if phrase_weights is None else list(phrase_weights)
    if len(pws) != B:
        raise ValueError(f"{len(pws)} phrase-weight entries for {B} queries")
    if _host_branch(index):
        # the scores of all B queries in one call, the reset vector per row, ONE batched PageRank
        S = index.scores(Q) if B else np.empty((0, 0), np.float32)
        resets = np.zeros((B, graph.n_vertices), dtype=np.float64)
        for b in range(B):
            resets[b] = _host_reset(graph, S[b], pws[b], passage_node_weight)
        if B == 0:
            return np.empty((0, len(graph.passage_vertices)), dtype=np.float64)
        return np.ascontiguousarray(_graph_ppr_batch(graph, resets, damping, tol, max_iter)[:, graph.passage_vertices])
    out = np.empty((B, graph.n_rows), dtype=np.float64)
    it = C.c_int32(0)
    for b0 in range(0, B, L.CMR_PPR_MAX_BATCH):
        nb = min(L.CMR_PPR_MAX_BATCH, B - b0)
        seeds = [_seed_arrays(pw) for pw in pws[b0:b0 + nb]]
        off = np.zeros(nb + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(v) for v, _ in seeds])
        sv = np.ascontiguousarray(np.concatenate([v for v, _ in seeds]), dtype=np.int32)
        sw = np.ascontiguousarray(np.concatenate([w for _, w in seeds]), dtype=np.float64)
        L.check(L.lib().cmr_index_ppr_batch(index._h, graph._h, Q[b0:b0 + nb].ctypes.data_as(C.c_void_p), nb, off.ctypes.data_as(C.c_void_p),
                                            sv.ctypes.data_as(C.c_void_p), sw.ctypes.data_as(C.c_void_p), float(passage_node_weight), float(damping),
                                            float(tol), int(max_iter), out[b0:b0 + nb].ctypes.data_as(C.c_void_p), C.byref(it)))
    return out


def _graph_ppr_batch(graph, resets: np.ndarray, damping: float, tol: float, max_iter: int) -> np.ndarray:
    """graph.ppr_batch, or — a custom graph object without it — its `ppr` row by row."""
    if hasattr(graph, "ppr_batch"):
        return np.asarray(graph.ppr_batch(resets, damping=damping, tol=tol, max_iter=max_iter))
    return np.stack([np.asarray(graph.ppr(r, damping=damping, tol=tol, max_iter=max_iter)) for r in resets])


def ppr_passage_ranking_batch(index, graph, query_embeddings, phrase_weights: Optional[Sequence] = None, passage_node_weight: float = 0.05,
                              damping: float = 0.5) -> list:
    """[(sorted_doc_ids, sorted_doc_scores)] per query, each exactly as ComoRAG.run_ppr returns them (ComoRAG.py:1101-1105); from
    DEVICE_RANK_MIN_ROWS passage rows up the device ranks (`ppr_passage_ranked_batch`)."""
    if _device_rank(graph, getattr(graph, "n_rows", 0)):
        ids, sc = ppr_passage_ranked_batch(index, graph, query_embeddings, phrase_weights, passage_node_weight, damping)
        return [(ids[b], sc[b]) for b in range(len(ids))]
    out = []
    for doc_scores in ppr_passage_scores_batch(index, graph, query_embeddings, phrase_weights, passage_node_weight, damping):
        sorted_doc_ids = np.argsort(doc_scores)[::-1]
        out.append((sorted_doc_ids, doc_scores[sorted_doc_ids.tolist()]))
    return out


def ppr_passage_ranked_batch(index, graph, query_embeddings, phrase_weights: Optional[Sequence] = None, passage_node_weight: float = 0.05,
                             damping: float = 0.5, n_out: Optional[int] = None, tol: float = 1e-12, max_iter: int = 200) -> Tuple[np.ndarray, np.ndarray]:
    """`ppr_passage_scores_batch` with the ranking on the device (ComoRAG.py:1101-1105): (ids [B, n_out] int64 passage rows, scores
    [B, n_out] float64) by descending score, equal scores by ascending row; n_out = None: all n_rows.  ids[b] = np.argsort(-doc, kind="stable")
    [:n_out] and scores[b] = doc[ids[b]] bit for bit, doc = ppr_passage_scores(Q[b], phrase_weights[b]).  A row-sharded index builds the reset
    vectors on the host as `ppr_passage_scores_batch` does and ranks through `graph.ppr_ranked_batch`."""
    Q = np.ascontiguousarray(np.asarray(query_embeddings, dtype=np.float32))
    if Q.ndim != 2:
        raise ValueError("query_embeddings must be [B, d]")
    B = Q.shape[0]
    pws = [None] * B if phrase_weights is None else list(phrase_weights)
    if len(pws) != B:
        raise ValueError(f"{len(pws)} phrase-weight entries for {B} queries")
    n = _n_out(n_out, graph.n_rows)
    if B == 0:
        return np.empty((0, n), np.int64), np.empty((0, n), np.float64)
    if _host_branch(index):
        S = index.scores(Q)
        resets = np.zeros((B, graph.n_vertices), dtype=np.float64)
        for b in range(B):
            resets[b] = _host_reset(graph, S[b], pws[b], passage_node_weight)
        return graph.ppr_ranked_batch(resets, n_out=n, damping=damping, tol=tol, max_iter=max_iter)
    ids = np.empty((B, n), dtype=np.int64)
    sc = np.empty((B, n), dtype=np.float64)
    it = C.c_int32(0)
    for b0 in range(0, B, L.CMR_PPR_MAX_BATCH):
        nb = min(L.CMR_PPR_MAX_BATCH, B - b0)
        seeds = [_seed_arrays(pw) for pw in pws[b0:b0 + nb]]
        off = np.zeros(nb + 1, dtype=np.int32)
        off[1:] = np.cumsum([len(v) for v, _ in seeds])
        sv = np.ascontiguousarray(np.concatenate([v for v, _ in seeds]), dtype=np.int32)
        sw = np.ascontiguousarray(np.concatenate([w for _, w in seeds]), dtype=np.float64)
        L.check(L.lib().cmr_index_ppr_ranked_batch(index._h, graph._h, Q[b0:b0 + nb].ctypes.data_as(C.c_void_p), nb, off.ctypes.data_as(C.c_void_p),
                                                   sv.ctypes.data_as(C.c_void_p), sw.ctypes.data_as(C.c_void_p), float(passage_node_weight), float(damping),
                                                   float(tol), int(max_iter), n, ids[b0:b0 + nb].ctypes.data_as(C.c_void_p),
                                                   sc[b0:b0 + nb].ctypes.data_as(C.c_void_p), C.byref(it)))
        graph.last_iters = it.value
    return ids, sc


def ppr_passage_ranked(index, graph, query_embedding, phrase_weights=None, passage_node_weight: float = 0.05, damping: float = 0.5,
                       n_out: Optional[int] = None, tol: float = 1e-12, max_iter: int = 200) -> Tuple[np.ndarray, np.ndarray]:
    """`ppr_passage_ranked_batch` for one query: (ids [n_out] int64, scores [n_out] float64).  On a device index this is
    cmr_index_ppr_ranked, which joins the index's combine queue as cmr_index_ppr does."""
    q = np.ascontiguousarray(np.asarray(query_embedding, dtype=np.float32).reshape(-1))
    if _host_branch(index):
        ids, sc = ppr_passage_ranked_batch(index, graph, q[None, :], [phrase_weights], passage_node_weight, damping, n_out, tol, max_iter)
        return ids[0], sc[0]
    n = _n_out(n_out, graph.n_rows)
    sv, sw = _seed_arrays(phrase_weights)
    ids = np.empty(n, dtype=np.int64)
    sc = np.empty(n, dtype=np.float64)
    it = C.c_int32(0)
    L.check(L.lib().cmr_index_ppr_ranked(index._h, graph._h, q.ctypes.data_as(C.c_void_p), sv.ctypes.data_as(C.c_void_p), sw.ctypes.data_as(C.c_void_p),
                                         len(sv), float(passage_node_weight), float(damping), float(tol), int(max_iter), n,
                                         ids.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), C.byref(it)))
    graph.last_iters = it.value
    return ids, sc
