"""DenseIndex — Python handle on one HBM-resident shard (`cmr_index_t`).

Host-side mirror of the numeric half of ComoRAG's retrieval path: where the
reference keeps `np.array(store.get_embeddings(keys))` matrices on the host
(src/comorag/ComoRAG.py:896-900) and runs np.dot + argsort per query (:937-967),
this keeps the matrix in HBM (MFMA-fragment-major panels) and asks the HIP library
for top-k / full scores.  numpy in, numpy out; torch tensors (device) accepted by
the *_dev methods.
"""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Optional, Tuple

import numpy as np

from . import _lib as L


def _f32c(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a: np.ndarray) -> int:
    # the array's address as an int (c_void_p parameters take one): `a.ctypes.data_as(...)` builds a ctypes helper object
    # per call, 2 us each — a third of a 35 us single-query search went into marshalling five arrays
    return a.__array_interface__["data"][0]


def pack_row_mask(n_rows: int, allow=None, exclude=None) -> np.ndarray:
    """Allow bitmap of a filtered search (`DenseIndex.search_filtered`, cmr_index_search_masked): uint32 [ceil(n_rows / 32)],
    bit (r & 31) of word (r >> 5) set when local row r is kept; bits at or beyond n_rows are zero.
    `allow`: a bool array [n_rows], or an iterable of row ids to keep; `exclude`: row ids to drop from an all-ones mask; neither:
    every row.  Giving both is an error; ids outside [0, n_rows) raise ValueError.  Pure numpy."""
    n_rows = int(n_rows)
    if n_rows < 0:
        raise ValueError(f"n_rows = {n_rows} < 0")
    if allow is not None and exclude is not None:
        raise ValueError("give allow or exclude, not both")

    def _ids(a) -> np.ndarray:
        ids = np.asarray(a if isinstance(a, np.ndarray) else list(a))
        if ids.size == 0:
            return np.empty(0, dtype=np.int64)
        if ids.ndim != 1 or ids.dtype.kind not in "iu":
            raise ValueError("row ids must be a 1-d sequence of integers")
        ids = ids.astype(np.int64)
        if ids.min() < 0 or ids.max() >= n_rows:
            raise ValueError(f"row id outside [0, {n_rows})")
        return ids

    if isinstance(allow, np.ndarray) and allow.dtype == np.bool_:
        if allow.shape != (n_rows,):
            raise ValueError(f"a bool allow array must be [{n_rows}], got {allow.shape}")
        keep = allow
    elif allow is not None:
        keep = np.zeros(n_rows, dtype=bool)
        keep[_ids(allow)] = True
    else:
        keep = np.ones(n_rows, dtype=bool)
        if exclude is not None:
            keep[_ids(exclude)] = False
    n_words = (n_rows + 31) // 32
    bits = np.zeros(n_words * 32, dtype=np.uint8)
    bits[:n_rows] = keep
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32, copy=False)


def pack_row_masks(n_rows: int, allow=None, exclude=None) -> np.ndarray:
    """Allow bitmaps of a per-query filtered search (`DenseIndex.search_filtered_each`, cmr_index_search_masked_each): uint32
    [nq, ceil(n_rows / 32)], row i exactly `pack_row_mask(n_rows, allow=allow[i])` (or `exclude=exclude[i]`).  `allow` / `exclude`: a
    sequence with one entry per query, each whatever `pack_row_mask` takes (a 2-d bool array [nq, n_rows] is a sequence of bool rows).
    Exactly one of the two must be given: the number of queries comes from its length."""
    if (allow is None) == (exclude is None):
        raise ValueError("give allow or exclude (one entry per query), not both and not neither")
    per_query = allow if allow is not None else exclude
    if isinstance(per_query, (str, bytes)) or not hasattr(per_query, "__len__"):
        raise ValueError("allow / exclude must be a sequence with one entry per query")
    n_words = (int(n_rows) + 31) // 32
    out = np.zeros((len(per_query), n_words), dtype=np.uint32)
    for i, entry in enumerate(per_query):
        out[i] = pack_row_mask(n_rows, allow=entry) if allow is not None else pack_row_mask(n_rows, exclude=entry)
    return out


def pack_id_lists(allow=None, exclude=None) -> Tuple[Optional[np.ndarray], np.ndarray]:
    """Row-id lists of `search_filtered_ids` (cmr_index_search_ids) as CSR: → (offsets int64 [nq + 1] | None, ids int64 [n_ids]).
    A 1-d integer array or a flat sequence of ints is ONE list shared by every query (offsets None).  A sequence with one entry per
    query — each a 1-d integer array or a flat sequence of ints, empty entries allowed; a 2-d integer array such as the ids an earlier
    search returned counts as one row per query — gives per-query lists: query i owns ids[offsets[i]:offsets[i + 1]].  The ids are not
    range-checked here: the device ignores negative ids (-1 padding) and ids the index does not hold.  Exactly one of `allow` /
    `exclude` must be given; anything else raises ValueError.  Pure numpy."""
    if (allow is None) == (exclude is None):
        raise ValueError("give allow or exclude, not both and not neither")
    lists = allow if allow is not None else exclude

    def _flat(a) -> np.ndarray:
        ids = np.asarray(a)
        if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
            raise ValueError("a row-id list must be a 1-d sequence of integers")
        return ids.astype(np.int64)

    if isinstance(lists, np.ndarray):
        if lists.dtype.kind not in "iu" or lists.ndim not in (1, 2):
            raise ValueError("row ids must be a 1-d (shared) or 2-d (one row per query) integer array")
        ids = np.ascontiguousarray(lists, dtype=np.int64)
        if ids.ndim == 1:
            return None, ids
        return np.arange(ids.shape[0] + 1, dtype=np.int64) * ids.shape[1], ids.reshape(-1)
    if isinstance(lists, (str, bytes)) or not hasattr(lists, "__len__") or not hasattr(lists, "__iter__"):
        raise ValueError("allow / exclude must be an integer array or a sequence")
    entries = list(lists)
    if all(isinstance(e, (int, np.integer)) and not isinstance(e, (bool, np.bool_)) for e in entries):
        return None, np.asarray(entries, dtype=np.int64).reshape(-1)      # (an empty sequence: one shared, empty list)
    if any(isinstance(e, (int, float, complex, bool, np.generic, str, bytes)) or not hasattr(e, "__len__") for e in entries):
        raise ValueError("allow / exclude must be a flat sequence of ints or a sequence with one list of ints per query")
    per_query = [_flat(e) for e in entries]
    offsets = np.zeros(len(per_query) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in per_query], out=offsets[1:])
    return offsets, (np.concatenate(per_query) if per_query else np.empty(0, dtype=np.int64))


def _ids_mode(mode) -> int:
    if mode in ("exclude", L.CMR_IDS_EXCLUDE):
        return L.CMR_IDS_EXCLUDE
    if mode in ("allow", L.CMR_IDS_ALLOW):
        return L.CMR_IDS_ALLOW
    raise ValueError(f"mode must be 'exclude' or 'allow', got {mode!r}")


def _mask_popcount(words: np.ndarray, n_rows: int) -> int:
    """Set bits among the first n_rows of an allow bitmap (bits at or beyond n_rows do not count)."""
    if len(words) == 0:
        return 0
    count = (lambda w: int(np.bitwise_count(w).sum())) if hasattr(np, "bitwise_count") else (lambda w: int(np.unpackbits(w.view(np.uint8)).sum()))
    total = count(words)
    if n_rows % 32:
        total -= count(words[-1:] & np.uint32(~((1 << (n_rows % 32)) - 1) & 0xFFFFFFFF))
    return total


def renumber_after_removal(ids, removed) -> np.ndarray:
    """Row ids held outside an index (cached result ids, a graph's vertex_of_row, the ids behind prepacked mask words) in the numbering
    after `remove_ids(removed)`: int64 array of the shape of `ids`, each entry its new id — id minus the distinct removed ids below it —
    or -1 where the entry itself was removed; negative entries (-1 padding) stay -1.  `removed`: the ids that were REMOVED, in the old
    numbering (what `remove_ids` was given, restricted to ids the index held; negative entries and duplicates are ignored).  Pure numpy."""
    ids = np.asarray(ids, dtype=np.int64)
    gone = np.unique(np.asarray(removed, dtype=np.int64).ravel())
    gone = gone[gone >= 0]
    below = np.searchsorted(gone, ids, side="left")
    hit = np.zeros(ids.shape, dtype=bool)
    if len(gone):
        hit = gone[np.minimum(below, len(gone) - 1)] == ids
    return np.where((ids < 0) | hit, np.int64(-1), ids - below).astype(np.int64)


# the calls whose host-array marshalling `DenseIndex` (cmr_index_*) and `MultiDeviceIndex` (cmr_mindex_*) share
_HOST_CALLS = ("destroy", "size", "info", "append", "search", "search_exact", "search_min_score", "scores", "sorted_scores",
               "rescore", "get_rows", "search_ids", "remove_ids", "update_rows", "range_count", "range_search", "search_min_score_ids",
               "range_count_ids", "range_search_ids", "pair_scores", "mmr_select", "search_mmr")
_bound = {}


def _host_calls(prefix: str) -> SimpleNamespace:
    """The library's `prefix` + name functions, resolved once per prefix: a call then costs two attribute reads."""
    c = _bound.get(prefix)
    if c is None:
        lib = L.lib()
        c = _bound[prefix] = SimpleNamespace(**{n: getattr(lib, prefix + n) for n in _HOST_CALLS})
    return c


class HostArrayIndex:
    """numpy in, numpy out: the call surface `DenseIndex` and `MultiDeviceIndex` have in common.  A subclass names the prefix of
    its C functions (`_PREFIX`), sets `self._c = _host_calls(self._PREFIX)` before it creates `self._h`, and has `dim`."""
    _PREFIX = ""

    # -- lifetime
    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            if not getattr(self, "_borrowed", False):
                self._c.destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        n = C.c_int64(0)
        L.check(self._c.size(self._h, C.byref(n)))
        return n.value

    @property
    def device_bytes(self) -> int:
        b = C.c_int64(0)
        L.check(self._c.info(self._h, None, None, None, C.byref(b)))
        return b.value

    def _queries(self, q) -> np.ndarray:
        q = _f32c(q)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self.dim:
            raise ValueError(f"q must be [nq,{self.dim}], got {q.shape}")
        return q

    # -- append
    def append(self, rows) -> None:
        rows = _f32c(rows)
        if rows.ndim == 1:
            rows = rows[None, :]
        if rows.shape[0] == 0:
            return
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n,{self.dim}], got {rows.shape}")
        L.check(self._c.append(self._h, _ptr(rows), rows.shape[0]))

    # -- remove (cmr_index_remove_ids / cmr_mindex_remove_ids)
    def remove_ids(self, ids) -> int:
        """Remove the listed rows (FAISS `IndexFlat.remove_ids`): survivors keep their order and are renumbered densely — row r becomes
        r minus the removed rows below it — and the index then answers every call bit for bit like a fresh one built from the surviving
        rows.  `ids`: anything `np.asarray(..., int64)` takes, row ids AS THE SEARCHES RETURN THEM (id base applied; `MultiDeviceIndex`:
        global ids); -1 padding, other negative ids, ids the index does not hold and duplicates are ignored, so a padded 2-d result of
        an earlier search goes in as it is.  → rows actually removed.  Row numbers held outside the index are stale afterwards
        (`renumber_after_removal`).  Exclusive like `append`; waits for everything in flight on the device."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64)).reshape(-1)
        n = C.c_int64(0)
        L.check(self._c.remove_ids(self._h, _ptr(ids) if len(ids) else None, len(ids), C.byref(n)))
        return n.value

    # -- update in place (cmr_index_update_rows / cmr_mindex_update_rows)
    def _update_args(self, ids, n_rows: int) -> np.ndarray:
        ids = np.asarray(ids)
        if ids.ndim == 0:
            ids = ids.reshape(1)
        if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
            raise ValueError("ids must be a 1-d sequence of integer row ids")
        if len(ids) != n_rows:
            raise ValueError(f"{len(ids)} ids for {n_rows} rows")
        return np.ascontiguousarray(ids, dtype=np.int64)

    def update_rows(self, ids, rows) -> int:
        """Replace the content of the listed rows in place: row count, row ids, capacity and id base / block tables stay, and the index
        then answers every call bit for bit like a fresh one built by appending the final row contents in order.  `ids` [n]: row ids AS
        THE SEARCHES RETURN THEM (`MultiDeviceIndex`: global ids), entry i paired with fp32 row i of `rows` [n, dim]; a scalar id with a
        1-d row is accepted.  Negative ids and ids the index does not hold are ignored with their rows; of an id that occurs several
        times the last occurrence wins.  → distinct rows replaced.  All or nothing: a NaN / Inf row, or one that rounds to Inf in the
        index dtype, among the rows that would be written raises `CmrError` (CMR_ERR_NONFINITE) with the index unchanged.  Exclusive
        like `remove_ids`; waits for everything in flight on the device."""
        rows = _f32c(rows)
        if rows.ndim == 1 and np.ndim(ids) == 0:
            rows = rows[None, :]
        if rows.ndim != 2 or rows.shape[1] != self.dim:
            raise ValueError(f"rows must be [n,{self.dim}], got {rows.shape}")
        ids = self._update_args(ids, rows.shape[0])
        n = C.c_int64(0)
        L.check(self._c.update_rows(self._h, _ptr(ids) if len(ids) else None, _ptr(rows) if len(ids) else None, len(ids), C.byref(n)))
        return n.value

    # -- search
    def search(self, q, k: int, with_minmax: bool = True
               ) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:
        """q [nq,dim] → (ids int64 [nq,k'], raw scores fp32 [nq,k'], min [nq], max [nq]) with
        k' = min(k, len(self)); order: score desc, row asc."""
        q = self._queries(q)
        nq = q.shape[0]
        ids = np.empty((nq, k), dtype=np.int64)
        sc = np.empty((nq, k), dtype=np.float32)
        mn = np.empty(nq, dtype=np.float32) if with_minmax else None
        mx = np.empty(nq, dtype=np.float32) if with_minmax else None
        L.check(self._c.search(self._h, _ptr(q), nq, k, _ptr(ids), _ptr(sc),
                               _ptr(mn) if with_minmax else None, _ptr(mx) if with_minmax else None))
        kk = min(k, len(self))
        return ids[:, :kk], sc[:, :kk], mn, mx

    # -- filtered search from row-id lists (cmr_index_search_ids / cmr_mindex_search_ids)
    def search_filtered_ids(self, q, k: int, *, allow=None, exclude=None, with_minmax: bool = True
                            ) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:
        """`search` among the rows the id lists leave: `exclude` = every row except the listed ones, `allow` = only the listed rows.  The
        ids are row ids AS THE SEARCHES RETURN THEM (id base / block table applied; over a `MultiDeviceIndex`: global ids), so what an
        earlier search returned — -1 padding included — goes straight back in: tri_retrieve's pool dedup (ComoRAG.py:499-505, 515-522,
        535-540) without a bitmap.  Lists as `pack_id_lists` takes them: one shared list, or one entry per query.  The device builds the
        allow words next to the corpus; nothing of the size of the corpus is packed or uploaded.  k <= 128.
        → (ids [nq,k], raw scores [nq,k], min [nq], max [nq]): always k columns, -1 / -inf padded, bit for bit what
        `DenseIndex.search_filtered_each` returns on the masks of the same rows; min / max over a query's allowed rows (+inf / -inf when
        it allows none)."""
        offsets, lst = pack_id_lists(allow=allow, exclude=exclude)
        q = self._queries(q)
        nq = q.shape[0]
        if offsets is not None and len(offsets) != nq + 1:
            raise ValueError(f"{len(offsets) - 1} id lists for {nq} queries")
        ids = np.empty((nq, k), dtype=np.int64)
        sc = np.empty((nq, k), dtype=np.float32)
        mn = np.empty(nq, dtype=np.float32) if with_minmax else None
        mx = np.empty(nq, dtype=np.float32) if with_minmax else None
        L.check(self._c.search_ids(self._h, _ptr(q), nq, k, L.CMR_IDS_ALLOW if allow is not None else L.CMR_IDS_EXCLUDE,
                                   _ptr(offsets) if offsets is not None else None, _ptr(lst) if len(lst) else None, len(lst),
                                   _ptr(ids), _ptr(sc), _ptr(mn) if with_minmax else None, _ptr(mx) if with_minmax else None))
        return ids, sc, mn, mx

    def search_min_score(self, q, k: int, min_score: float) -> Tuple[np.ndarray, np.ndarray]:
        """The k best rows among those with raw score >= min_score: (ids [nq,k], scores [nq,k]), -1 / -inf padded."""
        q = self._queries(q)
        nq = q.shape[0]
        ids = np.empty((nq, k), dtype=np.int64)
        sc = np.empty((nq, k), dtype=np.float32)
        L.check(self._c.search_min_score(self._h, _ptr(q), nq, k, float(min_score), _ptr(ids), _ptr(sc)))
        return ids, sc

    # -- range search (cmr_index_range_search / cmr_mindex_range_search)
    def range_search(self, q, min_score: float, max_total: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """EVERY row with raw score >= min_score, per query (FAISS `range_search`): (lims int64 [nq + 1], ids int64 [lims[nq]], scores fp32
        [lims[nq]]) — query i owns ids[lims[i]:lims[i + 1]], best first (score descending, then row id ascending): the head of row i of
        `sorted_scores`, as long as the scores stay at or above the bound.  The comparison is `search_min_score`'s (a row that attains the
        bound is in; -0.0 and +0.0 are one value), a row's score bits are those `scores` returns for it, ids are as the searches return
        them.  +inf: empty lists; -inf: every row; NaN: `CmrError` (CMR_ERR_INVALID).  `max_total` (None: 2^31 - 1): a batch with more hits
        in all raises `CmrError` (CMR_ERR_UNSUPPORTED, the total in the message) before anything is compacted, sorted or allocated —
        `range_count` sizes a request.  The arrays are numpy copies: the library's result is gone when this returns."""
        q = self._queries(q)
        nq = q.shape[0]
        res = C.c_void_p()
        L.check(self._c.range_search(self._h, _ptr(q), nq, float(min_score), int(max_total) if max_total is not None else 0, C.byref(res)))
        return self._range_lists(res, nq)

    @staticmethod
    def _range_lists(res, nq: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """numpy copies of a cmr_range_result_t, which is destroyed"""
        try:
            n, lims_p, ids_p, sc_p = C.c_int32(0), C.c_void_p(), C.c_void_p(), C.c_void_p()
            L.check(L.lib().cmr_range_result_view(res, C.byref(n), C.byref(lims_p), C.byref(ids_p), C.byref(sc_p)))
            lims = np.ctypeslib.as_array(C.cast(lims_p, C.POINTER(C.c_int64)), shape=(nq + 1,)).copy()
            total = int(lims[nq])
            if total:
                ids = np.ctypeslib.as_array(C.cast(ids_p, C.POINTER(C.c_int64)), shape=(total,)).copy()
                sc = np.ctypeslib.as_array(C.cast(sc_p, C.POINTER(C.c_float)), shape=(total,)).copy()
            else:
                ids, sc = np.empty(0, dtype=np.int64), np.empty(0, dtype=np.float32)
        finally:
            L.lib().cmr_range_result_destroy(res)
        return lims, ids, sc

    def range_count(self, q, min_score: float) -> np.ndarray:
        """Rows with raw score >= min_score per query, int64 [nq]: `np.diff(lims)` of `range_search` without the lists, and without its
        limit on the total."""
        q = self._queries(q)
        out = np.empty(q.shape[0], dtype=np.int64)
        L.check(self._c.range_count(self._h, _ptr(q), q.shape[0], float(min_score), _ptr(out)))
        return out

    # -- the score-bound searches among the rows id lists leave (cmr_index_*_ids / cmr_mindex_*_ids)
    def _id_list_args(self, q, allow, exclude):
        """→ (q [nq, dim], nq, (mode, offsets pointer | None, ids pointer | None, n_ids), the arrays behind the pointers)"""
        offsets, lst = pack_id_lists(allow=allow, exclude=exclude)
        q = self._queries(q)
        nq = q.shape[0]
        if offsets is not None and len(offsets) != nq + 1:
            raise ValueError(f"{len(offsets) - 1} id lists for {nq} queries")
        return q, nq, (L.CMR_IDS_ALLOW if allow is not None else L.CMR_IDS_EXCLUDE, _ptr(offsets) if offsets is not None else None,
                       _ptr(lst) if len(lst) else None, len(lst)), (offsets, lst)

    def search_min_score_filtered_ids(self, q, k: int, min_score: float, *, allow=None, exclude=None) -> Tuple[np.ndarray, np.ndarray]:
        """`search_min_score` among the rows the id lists leave (lists as `search_filtered_ids` takes them): row i of
        `search_filtered_ids(q, k, ...)` with every entry whose score is below the bound replaced by -1 / -inf padding, bit for bit.
        → (ids [nq,k], scores [nq,k]); k <= 128."""
        q, nq, lists, _keep = self._id_list_args(q, allow, exclude)
        ids = np.empty((nq, k), dtype=np.int64)
        sc = np.empty((nq, k), dtype=np.float32)
        L.check(self._c.search_min_score_ids(self._h, _ptr(q), nq, k, float(min_score), *lists, _ptr(ids), _ptr(sc)))
        return ids, sc

    def range_search_filtered_ids(self, q, min_score: float, *, allow=None, exclude=None, max_total: Optional[int] = None
                                  ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`range_search` among the rows the id lists leave: list i is list i of `range_search` with the entries of disallowed rows
        removed, bit for bit (order, ids, score words) — every row of a namespace at or above a similarity, or tri_retrieve's neighbours
        down to a bound with the question's pool kept out.  Lists as `search_filtered_ids` takes them (ids as the searches return them;
        `MultiDeviceIndex`: global ids; -1 padding is ignored).  -inf: the complete ranking of the allowed rows.  `max_total` is judged on
        the filtered total.  A query that allows nothing gets an empty list.  → (lims [nq + 1], ids, scores)."""
        q, nq, lists, _keep = self._id_list_args(q, allow, exclude)
        res = C.c_void_p()
        L.check(self._c.range_search_ids(self._h, _ptr(q), nq, float(min_score), int(max_total) if max_total is not None else 0, *lists, C.byref(res)))
        return self._range_lists(res, nq)

    def range_count_filtered_ids(self, q, min_score: float, *, allow=None, exclude=None) -> np.ndarray:
        """`np.diff(lims)` of `range_search_filtered_ids` without the lists and without its limit: int64 [nq]."""
        q, nq, lists, _keep = self._id_list_args(q, allow, exclude)
        out = np.empty(nq, dtype=np.int64)
        L.check(self._c.range_count_ids(self._h, _ptr(q), nq, float(min_score), *lists, _ptr(out)))
        return out

    # -- exact fp32 top-k (a 16-bit index created with keep_f32=True; an f32 index is exact already)
    def search_exact(self, q, k: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The ids / scores of the reference's fp32 np.dot + argsort (ComoRAG.py:958-966) from a bf16 / f16 index:
        (ids int64 [nq,k'], fp32 scores [nq,k'], exact bool [nq]) with k' = min(k, len(self)), k <= 64.  exact[i] is True only
        when the certificate proves the list is the fp32 top-k (cmr_index_search_exact; over the shards of a
        `MultiDeviceIndex` each shard certifies its top-k, the host merges, exact[i] = AND over the shards)."""
        q = self._queries(q)
        nq = q.shape[0]
        ids = np.empty((nq, k), dtype=np.int64)
        sc = np.empty((nq, k), dtype=np.float32)
        ex = np.empty(nq, dtype=np.int32)
        L.check(self._c.search_exact(self._h, _ptr(q), nq, k, _ptr(ids), _ptr(sc), _ptr(ex)))
        kk = min(k, len(self))
        return ids[:, :kk], sc[:, :kk], ex.astype(bool)

    def scores(self, q) -> np.ndarray:
        """All raw scores [nq, N] (fp32)."""
        q = _f32c(q)
        if q.ndim == 1:
            q = q[None, :]
        n = len(self)
        out = np.empty((q.shape[0], n), dtype=np.float32)
        if n:
            L.check(self._c.scores(self._h, _ptr(q), q.shape[0], _ptr(out), n))
        return out

    def sorted_scores(self, q):
        """Complete ranking: (ids int64 [nq,N], raw scores fp32 [nq,N] descending, min [nq], max [nq])."""
        q = _f32c(q)
        if q.ndim == 1:
            q = q[None, :]
        n, nq = len(self), q.shape[0]
        ids = np.empty((nq, n), dtype=np.int64)
        sc = np.empty((nq, n), dtype=np.float32)
        mn = np.empty(nq, dtype=np.float32)
        mx = np.empty(nq, dtype=np.float32)
        if n:
            L.check(self._c.sorted_scores(self._h, _ptr(q), nq, _ptr(ids), _ptr(sc), _ptr(mn), _ptr(mx)))
        return ids, sc, mn, mx

    def rescore(self, q, cand, k: int) -> Tuple[np.ndarray, np.ndarray]:
        q = _f32c(q)
        if q.ndim == 1:
            q = q[None, :]
        cand = np.ascontiguousarray(cand, dtype=np.int64)
        if cand.ndim == 1:
            cand = cand[None, :]
        nq, nc = cand.shape
        k = min(k, nc)
        ids = np.empty((nq, k), dtype=np.int64)
        sc = np.empty((nq, k), dtype=np.float32)
        L.check(self._c.rescore(self._h, _ptr(q), nq, _ptr(cand), nc, k, _ptr(ids), _ptr(sc)))
        return ids, sc

    def get_rows(self, ids) -> np.ndarray:
        ids = np.ascontiguousarray(ids, dtype=np.int64).ravel()
        out = np.empty((len(ids), self.dim), dtype=np.float32)
        if len(ids):
            L.check(self._c.get_rows(self._h, _ptr(ids), len(ids), _ptr(out)))
        return out

    # -- diversified top-k: maximal marginal relevance (cmr_index_search_mmr / cmr_mindex_search_mmr)
    @staticmethod
    def default_fetch_k(k: int) -> int:
        return min(L.CMR_MAX_K, max(4 * int(k), 20))

    def search_mmr(self, q, k: int, fetch_k: Optional[int] = None, lambda_mult: float = 0.5, *, allow=None, exclude=None
                   ) -> Tuple[np.ndarray, np.ndarray]:
        """MMR re-ranked top-k (LangChain's `max_marginal_relevance_search`): the `fetch_k` most relevant rows are fetched by the ordinary
        search, then k of them are picked greedily, each maximising lambda_mult * relevance - (1 - lambda_mult) * (largest pair score with
        a row picked before), in fp32 on the device (include/comorag_hip.h states the arithmetic; it is reproducible bit for bit).
        → (ids [nq,k'], scores [nq,k']) in PICK order, k' = min(k, len(self)); scores are the raw relevance scores of the picked rows,
        -1 / -inf behind the last pick.  `fetch_k` defaults to min(128, max(4 k, 20)) and is raised to k; 1 <= k <= fetch_k <= 128.
        lambda_mult = 1 is exactly `search(q, k)`; on L2-normalised rows the pair scores are cosines, MMR's usual form.
        One call and one host round trip.  With `allow` / `exclude` id lists (as `search_filtered_ids` takes them) it is TWO calls:
        `search_filtered_ids(q, fetch_k, ...)` followed by `mmr_select`."""
        q = self._queries(q)
        nq, k = q.shape[0], int(k)
        fetch_k = max(k, self.default_fetch_k(k) if fetch_k is None else int(fetch_k))
        kk = min(k, len(self))
        if allow is not None or exclude is not None:
            cid, csc, _, _ = self.search_filtered_ids(q, fetch_k, allow=allow, exclude=exclude, with_minmax=False)
            ids, sc = self.mmr_select(cid, csc, k, lambda_mult)
            return ids[:, :kk], sc[:, :kk]
        ids = np.empty((nq, k), dtype=np.int64)
        sc = np.empty((nq, k), dtype=np.float32)
        L.check(self._c.search_mmr(self._h, _ptr(q), nq, k, fetch_k, float(lambda_mult), _ptr(ids), _ptr(sc)))
        return ids[:, :kk], sc[:, :kk]

    def mmr_select(self, cand_ids, cand_scores, k: int, lambda_mult: float = 0.5) -> Tuple[np.ndarray, np.ndarray]:
        """The MMR selection of `search_mmr` over candidates of ANY earlier search: `cand_ids` / `cand_scores` [nq, F] (or [F]) as a search
        returned them — -1 / -inf padding, ids the index does not hold and repeated ids are skipped.  → (ids [nq,k], scores [nq,k]) in pick
        order, -1 / -inf padded; k <= F <= 128."""
        cand_ids = np.ascontiguousarray(cand_ids, dtype=np.int64)
        cand_scores = _f32c(cand_scores)
        if cand_ids.ndim == 1:
            cand_ids, cand_scores = cand_ids[None, :], cand_scores.reshape(1, -1)
        if cand_ids.ndim != 2 or cand_ids.shape != cand_scores.shape:
            raise ValueError(f"cand_ids {cand_ids.shape} and cand_scores {cand_scores.shape} must be [nq, F] both")
        nq, f = cand_ids.shape
        k = int(k)
        ids = np.empty((nq, k), dtype=np.int64)
        sc = np.empty((nq, k), dtype=np.float32)
        L.check(self._c.mmr_select(self._h, _ptr(cand_ids), _ptr(cand_scores), nq, f, k, float(lambda_mult), _ptr(ids), _ptr(sc)))
        return ids, sc

    def pair_scores(self, ids) -> np.ndarray:
        """Scores of stored rows against stored rows: ids [F] → [F, F], ids [nq, F] → [nq, F, F]; out[..., s, c] has the bits
        `scores(get_rows([ids[s]]))[0, ids[c]]` returns.  Rows and columns of negative ids, ids the index does not hold and ids repeated
        from an earlier position are -inf.  F <= 128."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        one = ids.ndim == 1
        if one:
            ids = ids[None, :]
        if ids.ndim != 2:
            raise ValueError(f"ids must be [F] or [nq, F], got {ids.shape}")
        nq, f = ids.shape
        out = np.empty((nq, f, f), dtype=np.float32)
        L.check(self._c.pair_scores(self._h, _ptr(ids), nq, f, _ptr(out)))
        return out[0] if one else out


class DenseIndex(HostArrayIndex):
    _PREFIX = "cmr_index_"

    def __init__(self, dim: int, dtype: str = "bf16", device: int = 0, capacity_hint: int = 0,
                 keep_f32: bool = False, options: Optional[dict] = None):
        self._c = _host_calls(self._PREFIX)
        self._h = C.c_void_p()
        self.dim = int(dim)
        self.dtype = dtype
        self.device = int(device)
        self.keep_f32 = bool(keep_f32)
        L.check(L.lib().cmr_index_create(self.device, self.dim, L.DTYPES[dtype], int(capacity_hint),
                                         L.CMR_FLAG_KEEP_F32 if keep_f32 else 0, C.byref(self._h)))
        for name, value in (options or {}).items():
            self.set_option(name, value)

    @classmethod
    def _borrow(cls, handle, dim: int, dtype: str, device: int, owner=None) -> "DenseIndex":
        """A view of a cmr_index_t somebody else owns (a shard of a MultiDeviceIndex): never destroyed from here."""
        self = cls.__new__(cls)
        self._c = _host_calls(cls._PREFIX)
        self._h, self.dim, self.dtype, self.device, self.keep_f32 = handle, int(dim), dtype, int(device), False
        self._borrowed, self._owner = True, owner
        return self

    def set_option(self, name: str, value: int) -> None:
        """Route selector (cmr_index_set_option): picks between implementations that return the same results."""
        L.check(L.lib().cmr_index_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        """Readable options (cmr_index_get_option): "last_route" (which path served the last call: CMR_ROUTE_* and the bits beside it in
        include/comorag_hip.h), "pipe_dual_scan_active", "pipe_cu_mask_active", "pipe_scan_cus", "exact_cand", "combine",
        "combine_wait_us", the combiner's counters (`combine_stats`), "prefilter" and, of the last pipelined call, "prefilter_active",
        "prefilter_rows", "prefilter_bytes" and — these wait for the pipeline — "prefilter_candidates", "prefilter_pairs",
        "prefilter_pair_overflow", "prefilter_wave_overflow"; "prefilter_tighten", "prefilter_pair_cap", "prefilter_wave_cap"; the int8
        sample's "prefilter_sample", "prefilter_sample_panels", "prefilter_sample_run", "prefilter_sample_wave_cap",
        "prefilter_sample_level0", "prefilter_sample_active" and — waiting for the pipeline — "prefilter_sample_pairs",
        "prefilter_sample_overflow"."""
        v = C.c_int64(0)
        L.check(L.lib().cmr_index_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def combine_stats(self) -> dict:
        """Counters of the combiner (option "combine" = 2..16: concurrent single search / scores / PPR calls of this index's callers share
        one batched call; with "combine_filtered" = 1 the filtered searches too): device calls made for combined work, queries served by them, the widest batch so far."""
        return {name: self.get_option("combine_" + name) for name in ("batches", "queries", "max_width")}

    def append_dev(self, rows_t, stream: Optional[int] = None) -> None:
        """rows_t: torch float32 CUDA tensor [n, dim], contiguous, on this index's device."""
        import torch
        assert rows_t.is_cuda and rows_t.dtype == torch.float32 and rows_t.is_contiguous()
        if rows_t.device.index != self.device:
            # the encoder may live on another GPU than the index (cfg.device vs the store's index device): a foreign
            # device pointer must not reach cmr_index_append_dev — go through the host
            self.append(rows_t.cpu().numpy())
            return
        if stream is None:
            stream = torch.cuda.current_stream(rows_t.device).cuda_stream
        L.check(L.lib().cmr_index_append_dev(self._h, C.c_void_p(rows_t.data_ptr()), rows_t.shape[0], C.c_void_p(stream)))

    def update_rows_dev(self, ids, rows_t, stream: Optional[int] = None) -> int:
        """`update_rows` with the rows in a torch float32 CUDA tensor [n, dim], contiguous (an encoder's output); the ids stay on the
        host.  A tensor on another device than the index goes through the host, as in `append_dev`.  Synchronous."""
        import torch
        assert rows_t.is_cuda and rows_t.dtype == torch.float32 and rows_t.is_contiguous()
        if rows_t.ndim != 2 or rows_t.shape[1] != self.dim:
            raise ValueError(f"rows must be [n,{self.dim}], got {tuple(rows_t.shape)}")
        if rows_t.device.index != self.device:
            return self.update_rows(ids, rows_t.cpu().numpy())
        ids = self._update_args(ids, rows_t.shape[0])
        if stream is None:
            stream = torch.cuda.current_stream(rows_t.device).cuda_stream
        n = C.c_int64(0)
        if len(ids):
            L.check(L.lib().cmr_index_update_rows_dev(self._h, _ptr(ids), C.c_void_p(rows_t.data_ptr()), len(ids), C.c_void_p(stream), C.byref(n)))
        return n.value

    def search_min_score_dev(self, q_t, k: int, min_score: float, out_ids=None, out_scores=None, stream: Optional[int] = None):
        """`search_min_score` on torch CUDA tensors, enqueued on torch's current stream without synchronising."""
        import torch
        assert q_t.is_cuda and q_t.dtype == torch.float32 and q_t.is_contiguous() and q_t.shape[1] == self.dim
        nq, dev = q_t.shape[0], q_t.device
        if out_ids is None:
            out_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
        if out_scores is None:
            out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.lib().cmr_index_search_min_score_dev(self._h, C.c_void_p(q_t.data_ptr()), nq, k, float(min_score),
                                                       C.c_void_p(out_ids.data_ptr()), C.c_void_p(out_scores.data_ptr()), C.c_void_p(stream)))
        return out_ids, out_scores

    def range_count_dev(self, q_t, min_score: float, out=None, stream: Optional[int] = None):
        """`range_count` on torch CUDA tensors (q_t float32 [nq, dim] → int64 [nq]), enqueued on torch's current stream without synchronising."""
        import torch
        assert q_t.is_cuda and q_t.dtype == torch.float32 and q_t.is_contiguous() and q_t.shape[1] == self.dim
        if out is None:
            out = torch.empty((q_t.shape[0],), dtype=torch.int64, device=q_t.device)
        assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.shape[0] == q_t.shape[0]
        if stream is None:
            stream = torch.cuda.current_stream(q_t.device).cuda_stream
        L.check(L.lib().cmr_index_range_count_dev(self._h, C.c_void_p(q_t.data_ptr()), q_t.shape[0], float(min_score), C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(stream)))
        return out

    def search_min_score_pipelined(self, q_t, k: int, min_score: float, out_ids, out_scores, wait_event=None):
        """`search_min_score` in throughput mode (the index's own streams; packing, scan and candidate merge of consecutive blocks
        overlap): returns the done-event handle of this block — `sync(handle)` of the LAST block covers every earlier one."""
        import torch
        assert q_t.is_cuda and q_t.dtype == torch.float32 and q_t.is_contiguous() and q_t.shape[1] == self.dim
        done = C.c_void_p()
        we = C.c_void_p(wait_event.cuda_event) if wait_event is not None else None
        L.check(L.lib().cmr_index_search_min_score_pipelined(self._h, C.c_void_p(q_t.data_ptr()), q_t.shape[0], k, float(min_score),
                                                             C.c_void_p(out_ids.data_ptr()), C.c_void_p(out_scores.data_ptr()), we, C.byref(done)))
        return done

    def search_dev(self, q_t, k: int, out_ids=None, out_scores=None, out_min=None, out_max=None,
                   stream: Optional[int] = None):
        """Asynchronous search on torch CUDA tensors, enqueued on torch's current stream (also when that is the default
        stream, handle 0): ordered after the kernels that produced `q_t`, before later readers of the outputs."""
        import torch
        assert q_t.is_cuda and q_t.dtype == torch.float32 and q_t.is_contiguous() and q_t.shape[1] == self.dim
        nq = q_t.shape[0]
        dev = q_t.device
        if out_ids is None:
            out_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
        if out_scores is None:
            out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.lib().cmr_index_search_dev(
            self._h, C.c_void_p(q_t.data_ptr()), nq, k, C.c_void_p(out_ids.data_ptr()), C.c_void_p(out_scores.data_ptr()),
            C.c_void_p(out_min.data_ptr()) if out_min is not None else None,
            C.c_void_p(out_max.data_ptr()) if out_max is not None else None, C.c_void_p(stream)))
        return out_ids, out_scores

    def search_mmr_dev(self, q_t, k: int, fetch_k: Optional[int] = None, lambda_mult: float = 0.5, out_ids=None, out_scores=None,
                       stream: Optional[int] = None):
        """`search_mmr` on torch CUDA tensors, enqueued on torch's current stream like `search_dev`: (ids [nq,k], scores [nq,k]), always k
        columns, -1 / -inf padded."""
        import torch
        assert q_t.is_cuda and q_t.dtype == torch.float32 and q_t.is_contiguous() and q_t.shape[1] == self.dim
        nq, k, dev = q_t.shape[0], int(k), q_t.device
        fetch_k = max(k, self.default_fetch_k(k) if fetch_k is None else int(fetch_k))
        if out_ids is None:
            out_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
        if out_scores is None:
            out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.lib().cmr_index_search_mmr_dev(self._h, C.c_void_p(q_t.data_ptr()), nq, k, fetch_k, float(lambda_mult),
                                                 C.c_void_p(out_ids.data_ptr()), C.c_void_p(out_scores.data_ptr()), C.c_void_p(stream)))
        return out_ids, out_scores

    def mmr_select_dev(self, cand_ids_t, cand_scores_t, k: int, lambda_mult: float = 0.5, out_ids=None, out_scores=None,
                       stream: Optional[int] = None):
        """`mmr_select` on torch CUDA tensors (int64 / float32 [nq, F], contiguous), enqueued on torch's current stream."""
        import torch
        assert cand_ids_t.is_cuda and cand_ids_t.dtype == torch.int64 and cand_ids_t.is_contiguous() and cand_ids_t.ndim == 2
        assert cand_scores_t.is_cuda and cand_scores_t.dtype == torch.float32 and cand_scores_t.is_contiguous() and cand_scores_t.shape == cand_ids_t.shape
        (nq, f), k, dev = cand_ids_t.shape, int(k), cand_ids_t.device
        if out_ids is None:
            out_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
        if out_scores is None:
            out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.lib().cmr_index_mmr_select_dev(self._h, C.c_void_p(cand_ids_t.data_ptr()), C.c_void_p(cand_scores_t.data_ptr()), nq, f, k,
                                                 float(lambda_mult), C.c_void_p(out_ids.data_ptr()), C.c_void_p(out_scores.data_ptr()),
                                                 C.c_void_p(stream)))
        return out_ids, out_scores

    # -- filtered search (cmr_index_search_masked*): top-k among the rows an allow bitmap keeps
    def search_filtered(self, q, k: int, mask=None, *, allow=None, exclude=None, with_minmax: bool = True
                        ) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:
        """`search` among the allowed LOCAL rows only (row r = the r-th appended row; returned ids carry the id base / block table as
        ever): what `search` returns on an index that holds just those rows, ids mapped back — the filter that tri_retrieve's pool dedup
        (ComoRAG.py:499-505, 515-522, 535-540) applies after its top-k, applied inside it.  `mask`: uint32 words of `pack_row_mask`
        ([ceil(len / 32)]), or give `allow` / `exclude` as `pack_row_mask` takes them.  One mask serves every query; k <= 128.
        → (ids [nq,k'], raw scores [nq,k'], min [nq], max [nq]) with k' = min(k, allowed rows); min / max over the allowed rows
        (+inf / -inf when there is none)."""
        n = len(self)
        if mask is None:
            mask = pack_row_mask(n, allow=allow, exclude=exclude)
        elif allow is not None or exclude is not None:
            raise ValueError("give mask or allow / exclude, not both")
        mask = np.ascontiguousarray(mask, dtype=np.uint32)
        if mask.ndim != 1:
            raise ValueError("mask must be a 1-d uint32 array")
        q = self._queries(q)
        nq = q.shape[0]
        ids = np.empty((nq, k), dtype=np.int64)
        sc = np.empty((nq, k), dtype=np.float32)
        mn = np.empty(nq, dtype=np.float32) if with_minmax else None
        mx = np.empty(nq, dtype=np.float32) if with_minmax else None
        L.check(L.lib().cmr_index_search_masked(self._h, _ptr(q), nq, k, _ptr(mask), mask.shape[0], _ptr(ids), _ptr(sc),
                                                _ptr(mn) if with_minmax else None, _ptr(mx) if with_minmax else None))
        kk = min(k, _mask_popcount(mask, n))
        return ids[:, :kk], sc[:, :kk], mn, mx

    # -- the score-bound searches among the rows allow bitmaps keep (cmr_index_search_min_score_masked, cmr_index_range_*_masked)
    def _mask_words_args(self, q, masks, allow, exclude):
        """→ (q [nq, dim], nq, masks uint32 [n_words] (shared) or [nq, n_words] (per query))"""
        n = len(self)
        q = self._queries(q)
        nq = q.shape[0]
        if masks is None:
            masks = pack_row_mask(n, allow=allow, exclude=exclude)
        elif allow is not None or exclude is not None:
            raise ValueError("give masks or allow / exclude, not both")
        masks = np.ascontiguousarray(masks, dtype=np.uint32)
        nw = (n + 31) // 32
        if masks.shape != (nw,) and masks.shape != (nq, nw):
            raise ValueError(f"masks must be uint32 [{nw}] (shared) or [{nq}, {nw}] (one row of pack_row_mask words per query), got {masks.shape}")
        return q, nq, masks

    def search_min_score_filtered(self, q, k: int, min_score: float, masks=None, *, allow=None, exclude=None) -> Tuple[np.ndarray, np.ndarray]:
        """`search_min_score` among the allowed LOCAL rows: row i of `search_filtered` (shared `masks` [n_words], or `allow` / `exclude` as
        `pack_row_mask` takes them) or `search_filtered_each` (`masks` [nq, n_words] as `pack_row_masks` lays them out) with every entry
        whose score is below the bound replaced by -1 / -inf padding, bit for bit.  → (ids [nq,k], scores [nq,k]); k <= 128."""
        q, nq, masks = self._mask_words_args(q, masks, allow, exclude)
        ids = np.empty((nq, k), dtype=np.int64)
        sc = np.empty((nq, k), dtype=np.float32)
        L.check(L.lib().cmr_index_search_min_score_masked(self._h, _ptr(q), nq, k, float(min_score), _ptr(masks), masks.shape[-1],
                                                          1 if masks.ndim == 1 else nq, _ptr(ids), _ptr(sc)))
        return ids, sc

    def range_search_filtered(self, q, min_score: float, masks=None, *, allow=None, exclude=None, max_total: Optional[int] = None
                              ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """`range_search` among the allowed LOCAL rows: list i is list i of `range_search` with the entries of disallowed rows removed, bit
        for bit — every row of one namespace or level at or above a similarity; with -inf the complete ranking of the namespace.  `masks`:
        uint32 [n_words] (one mask for every query) or [nq, n_words] (per query, `pack_row_masks`), or give `allow` / `exclude` as
        `pack_row_mask` takes them (shared).  `max_total` is judged on the filtered total; a query that allows nothing gets an empty list.
        → (lims [nq + 1], ids, scores) as `range_search`."""
        q, nq, masks = self._mask_words_args(q, masks, allow, exclude)
        res = C.c_void_p()
        L.check(L.lib().cmr_index_range_search_masked(self._h, _ptr(q), nq, float(min_score), int(max_total) if max_total is not None else 0,
                                                      _ptr(masks), masks.shape[-1], 1 if masks.ndim == 1 else nq, C.byref(res)))
        return self._range_lists(res, nq)

    def range_count_filtered(self, q, min_score: float, masks=None, *, allow=None, exclude=None) -> np.ndarray:
        """`np.diff(lims)` of `range_search_filtered` without the lists and without its limit: int64 [nq]."""
        q, nq, masks = self._mask_words_args(q, masks, allow, exclude)
        out = np.empty(nq, dtype=np.int64)
        L.check(L.lib().cmr_index_range_count_masked(self._h, _ptr(q), nq, float(min_score), _ptr(masks), masks.shape[-1],
                                                     1 if masks.ndim == 1 else nq, _ptr(out)))
        return out

    def search_filtered_dev(self, q_t, k: int, mask_t, out_ids=None, out_scores=None, out_min=None, out_max=None,
                            stream: Optional[int] = None):
        """`search_filtered` on torch CUDA tensors, enqueued on torch's current stream without synchronising (as `search_dev`).
        mask_t: the words of `pack_row_mask` on the device — int32 (torch has no uint32 arithmetic: `torch.from_numpy(words.view(np.int32))`)
        or uint32, contiguous, [ceil(len / 32)], read in place: upload a mask once and reuse it.  → (out_ids [nq,k], out_scores [nq,k]),
        -1 / -inf padded when fewer than k rows are allowed."""
        import torch
        assert q_t.is_cuda and q_t.dtype == torch.float32 and q_t.is_contiguous() and q_t.shape[1] == self.dim
        assert mask_t.is_cuda and mask_t.element_size() == 4 and not mask_t.dtype.is_floating_point and mask_t.is_contiguous() and mask_t.dim() == 1
        nq, dev = q_t.shape[0], q_t.device
        if out_ids is None:
            out_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
        if out_scores is None:
            out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.lib().cmr_index_search_masked_dev(
            self._h, C.c_void_p(q_t.data_ptr()), nq, k, C.c_void_p(mask_t.data_ptr()), mask_t.shape[0],
            C.c_void_p(out_ids.data_ptr()), C.c_void_p(out_scores.data_ptr()),
            C.c_void_p(out_min.data_ptr()) if out_min is not None else None,
            C.c_void_p(out_max.data_ptr()) if out_max is not None else None, C.c_void_p(stream)))
        return out_ids, out_scores

    # -- filtered search with a mask per query (cmr_index_search_masked_each*)
    def search_filtered_each(self, q, k: int, masks=None, *, allow=None, exclude=None, with_minmax: bool = True
                             ) -> Tuple[np.ndarray, np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:
        """`search_filtered` with an allow bitmap of its own for every query, in ONE corpus pass: row i is bit for bit what
        `search_filtered(q[i:i+1], k, mask=masks[i])` returns — every question of a ComoRAG batch (ComoRAG.try_answer, ComoRAG.py:432-453)
        has its own memory pool to keep out of tri_retrieve's top-k; so have the namespaces of one serving index.  `masks`: uint32
        [nq, ceil(len / 32)] as `pack_row_masks` lays them out, or give `allow` / `exclude` with one entry per query.  k <= 128.
        → (ids [nq,k], raw scores [nq,k], min [nq], max [nq]): always k columns, -1 / -inf padded behind a query's allowed rows (the
        counts differ per query); min / max over that query's allowed rows (+inf / -inf when it allows none)."""
        n = len(self)
        q = self._queries(q)
        nq = q.shape[0]
        if masks is None:
            masks = pack_row_masks(n, allow=allow, exclude=exclude)
        elif allow is not None or exclude is not None:
            raise ValueError("give masks or allow / exclude, not both")
        masks = np.ascontiguousarray(masks, dtype=np.uint32)
        if masks.ndim != 2 or masks.shape != (nq, (n + 31) // 32):
            raise ValueError(f"masks must be uint32 [{nq}, {(n + 31) // 32}] (one row of pack_row_mask words per query), got {masks.shape}")
        ids = np.empty((nq, k), dtype=np.int64)
        sc = np.empty((nq, k), dtype=np.float32)
        mn = np.empty(nq, dtype=np.float32) if with_minmax else None
        mx = np.empty(nq, dtype=np.float32) if with_minmax else None
        L.check(L.lib().cmr_index_search_masked_each(self._h, _ptr(q), nq, k, _ptr(masks), masks.shape[1], _ptr(ids), _ptr(sc),
                                                     _ptr(mn) if with_minmax else None, _ptr(mx) if with_minmax else None))
        return ids, sc, mn, mx

    def search_filtered_each_dev(self, q_t, k: int, masks_t, out_ids=None, out_scores=None, out_min=None, out_max=None,
                                 stream: Optional[int] = None):
        """`search_filtered_each` on torch CUDA tensors, enqueued on torch's current stream without synchronising (as
        `search_filtered_dev`).  masks_t: the words of `pack_row_masks` on the device — int32 or uint32, contiguous,
        [nq, ceil(len / 32)], read in place.  → (out_ids [nq,k], out_scores [nq,k]), -1 / -inf padded."""
        import torch
        assert q_t.is_cuda and q_t.dtype == torch.float32 and q_t.is_contiguous() and q_t.shape[1] == self.dim
        assert masks_t.is_cuda and masks_t.element_size() == 4 and not masks_t.dtype.is_floating_point and masks_t.is_contiguous()
        nq, dev = q_t.shape[0], q_t.device
        if masks_t.dim() != 2 or masks_t.shape[0] != nq:
            raise ValueError(f"masks_t must be [{nq}, n_words], got {tuple(masks_t.shape)}")
        if out_ids is None:
            out_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
        if out_scores is None:
            out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.lib().cmr_index_search_masked_each_dev(
            self._h, C.c_void_p(q_t.data_ptr()), nq, k, C.c_void_p(masks_t.data_ptr()), masks_t.shape[1],
            C.c_void_p(out_ids.data_ptr()), C.c_void_p(out_scores.data_ptr()),
            C.c_void_p(out_min.data_ptr()) if out_min is not None else None,
            C.c_void_p(out_max.data_ptr()) if out_max is not None else None, C.c_void_p(stream)))
        return out_ids, out_scores

    # -- filtered search from row-id lists on device tensors (cmr_index_row_masks_dev, cmr_index_search_ids_dev)
    @staticmethod
    def _id_list_tensors(ids_t, offsets_t):
        import torch
        assert ids_t.is_cuda and ids_t.dtype == torch.int64 and ids_t.is_contiguous() and ids_t.dim() == 1
        if offsets_t is not None:
            assert offsets_t.is_cuda and offsets_t.dtype == torch.int64 and offsets_t.is_contiguous() and offsets_t.dim() == 1
            assert offsets_t.device == ids_t.device

    def row_masks_dev(self, ids_t, offsets_t=None, nq: int = 1, mode="exclude", out=None, stream: Optional[int] = None):
        """The allow words `search_filtered_dev` / `search_filtered_each_dev` take, built on the device from row ids (as the searches
        return them; torch int64 CUDA tensor [n_ids]) — build once, search many times.  offsets_t: int64 [nq + 1] CSR offsets on the
        device (query i owns ids_t[offsets_t[i]:offsets_t[i + 1]]) → words int32 [nq, ceil(len / 32)]; None: one shared list → words
        [ceil(len / 32)].  Exactly the words of `pack_row_masks` / `pack_row_mask` on the local rows of the lists.  Enqueued on torch's
        current stream without synchronising."""
        import torch
        self._id_list_tensors(ids_t, offsets_t)
        n_words = (len(self) + 31) // 32
        if offsets_t is not None:
            nq = offsets_t.shape[0] - 1
        shape = (nq, n_words) if offsets_t is not None else (n_words,)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=ids_t.device)
        assert out.is_cuda and out.element_size() == 4 and out.is_contiguous() and tuple(out.shape) == shape
        if stream is None:
            stream = torch.cuda.current_stream(ids_t.device).cuda_stream
        L.check(L.lib().cmr_index_row_masks_dev(
            self._h, _ids_mode(mode), nq if offsets_t is not None else 1, C.c_void_p(offsets_t.data_ptr()) if offsets_t is not None else None,
            C.c_void_p(ids_t.data_ptr()) if ids_t.shape[0] else None, ids_t.shape[0], C.c_void_p(out.data_ptr()), n_words, C.c_void_p(stream)))
        return out

    def search_filtered_ids_dev(self, q_t, k: int, ids_t, offsets_t=None, mode="exclude", out_ids=None, out_scores=None, out_min=None,
                                out_max=None, stream: Optional[int] = None):
        """`search_filtered_ids` on torch CUDA tensors, enqueued on torch's current stream without synchronising: ids_t int64 [n_ids],
        offsets_t int64 [nq + 1] or None (one shared list), mode "exclude" | "allow".  The words are built into scratch of this stream's
        workspace.  → (out_ids [nq,k], out_scores [nq,k]), -1 / -inf padded."""
        import torch
        assert q_t.is_cuda and q_t.dtype == torch.float32 and q_t.is_contiguous() and q_t.shape[1] == self.dim
        self._id_list_tensors(ids_t, offsets_t)
        nq, dev = q_t.shape[0], q_t.device
        if offsets_t is not None and offsets_t.shape[0] != nq + 1:
            raise ValueError(f"offsets_t must be [{nq + 1}], got {tuple(offsets_t.shape)}")
        if out_ids is None:
            out_ids = torch.empty((nq, k), dtype=torch.int64, device=dev)
        if out_scores is None:
            out_scores = torch.empty((nq, k), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        L.check(L.lib().cmr_index_search_ids_dev(
            self._h, C.c_void_p(q_t.data_ptr()), nq, k, _ids_mode(mode), C.c_void_p(offsets_t.data_ptr()) if offsets_t is not None else None,
            C.c_void_p(ids_t.data_ptr()) if ids_t.shape[0] else None, ids_t.shape[0],
            C.c_void_p(out_ids.data_ptr()), C.c_void_p(out_scores.data_ptr()),
            C.c_void_p(out_min.data_ptr()) if out_min is not None else None,
            C.c_void_p(out_max.data_ptr()) if out_max is not None else None, C.c_void_p(stream)))
        return out_ids, out_scores

    def search_pipelined(self, q_t, k: int, out_ids, out_scores, out_min=None, out_max=None, wait_event=None):
        """Throughput mode (cmr_index_search_pipelined): enqueue on the index's own two streams and
        return an opaque done-event handle.  `wait_event`: a torch.cuda.Event (inputs ready) or None.
        Use `wait(handle, stream)` / `sync(handle)` before reading the outputs."""
        import torch
        assert q_t.is_cuda and q_t.dtype == torch.float32 and q_t.is_contiguous() and q_t.shape[1] == self.dim
        done = C.c_void_p()
        we = C.c_void_p(wait_event.cuda_event) if wait_event is not None else None
        L.check(L.lib().cmr_index_search_pipelined(
            self._h, C.c_void_p(q_t.data_ptr()), q_t.shape[0], k, C.c_void_p(out_ids.data_ptr()), C.c_void_p(out_scores.data_ptr()),
            C.c_void_p(out_min.data_ptr()) if out_min is not None else None,
            C.c_void_p(out_max.data_ptr()) if out_max is not None else None, we, C.byref(done)))
        return done

    def query_status(self) -> bool:
        """True if a `search_dev` / `search_pipelined` call since the last check saw a NaN/Inf query (those entry
        points cannot raise without a sync; this one synchronises their streams)."""
        f = C.c_int32(0)
        L.check(L.lib().cmr_index_query_status(self._h, C.byref(f)))
        return bool(f.value)

    def set_id_base(self, base: int) -> None:
        """Offset added to every returned row id (global id of local row 0 of a row shard)."""
        L.check(L.lib().cmr_index_set_id_base(self._h, int(base)))

    def set_id_blocks(self, local_starts, global_starts) -> None:
        """Block table of a shard that took incremental appends: local rows [local_starts[b], local_starts[b+1]) carry the
        global ids global_starts[b] + 0, 1, ... (cmr_index_set_id_blocks)."""
        ls = np.ascontiguousarray(local_starts, dtype=np.int64)
        gs = np.ascontiguousarray(global_starts, dtype=np.int64)
        if ls.shape != gs.shape or ls.ndim != 1 or len(ls) == 0:
            raise ValueError("local_starts / global_starts must be equally long, non-empty 1-d arrays")
        L.check(L.lib().cmr_index_set_id_blocks(self._h, len(ls), _ptr(ls), _ptr(gs)))

    def pipeline_stream(self, which: int = 2):
        """The pipeline's pre / scan / post stream as a torch.cuda.ExternalStream."""
        import torch
        s = C.c_void_p()
        L.check(L.lib().cmr_index_pipeline_stream(self._h, which, C.byref(s)))
        return torch.cuda.ExternalStream(s.value, device=torch.device("cuda", self.device))

    @staticmethod
    def wait(done_handle, torch_stream) -> None:
        """Make a torch stream wait for a pipelined search's outputs."""
        L.check(L.lib().cmr_stream_wait_event(C.c_void_p(torch_stream.cuda_stream), done_handle))

    @staticmethod
    def sync(done_handle) -> None:
        L.check(L.lib().cmr_event_synchronize(done_handle))

    def scores_dev(self, q_t, out=None, stream: Optional[int] = None):
        import torch
        assert q_t.is_cuda and q_t.dtype == torch.float32 and q_t.is_contiguous()
        n = len(self)
        if out is None:
            out = torch.empty((q_t.shape[0], n), dtype=torch.float32, device=q_t.device)
        if stream is None:
            stream = torch.cuda.current_stream(q_t.device).cuda_stream
        L.check(L.lib().cmr_index_scores_dev(self._h, C.c_void_p(q_t.data_ptr()), q_t.shape[0],
                                             C.c_void_p(out.data_ptr()), out.stride(0), C.c_void_p(stream)))
        return out

    def search_exact_pipelined(self, q_t, k: int, out_ids, out_scores, out_exact, wait_event=None):
        """`search_exact` stage 1 in throughput mode (cmr_index_search_exact_pipelined): torch CUDA tensors out_ids int64 [nq,k],
        out_scores fp32 [nq,k], out_exact int32 [nq]; returns the done-event handle (`wait` / `sync`).  Queries with
        out_exact == 0 may be asked again through `search_exact`."""
        import torch
        assert q_t.is_cuda and q_t.dtype == torch.float32 and q_t.is_contiguous() and q_t.shape[1] == self.dim
        assert out_exact.dtype == torch.int32 and out_exact.is_contiguous()
        done = C.c_void_p()
        we = C.c_void_p(wait_event.cuda_event) if wait_event is not None else None
        L.check(L.lib().cmr_index_search_exact_pipelined(
            self._h, C.c_void_p(q_t.data_ptr()), q_t.shape[0], k, C.c_void_p(out_ids.data_ptr()), C.c_void_p(out_scores.data_ptr()),
            C.c_void_p(out_exact.data_ptr()), we, C.byref(done)))
        return done

    def round_stats(self) -> Tuple[float, float]:
        """(max ||round(x)||, max ||round(x) - x||) over the appended rows: the maxima the exact search's certificate uses."""
        a, b = C.c_float(0), C.c_float(0)
        L.check(L.lib().cmr_index_round_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def prefilter_stats(self) -> Tuple[float, float]:
        """(max ||x||, max ||x - a m||) over the rows of the int8 companion (option "prefilter"): the maxima the pre-filter's bound uses."""
        a, b = C.c_float(0), C.c_float(0)
        L.check(L.lib().cmr_index_prefilter_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- measurement
    def profile(self, on) -> None:
        """HIP-event timing of the main scans: True / 1 = every scan, N > 1 = every N-th scan, False / 0 = off."""
        L.check(L.lib().cmr_profile_enable(self._h, int(on)))

    def profile_collect(self) -> dict:
        n, ms, b = C.c_int64(0), C.c_double(0), C.c_double(0)
        L.check(L.lib().cmr_profile_collect(self._h, C.byref(n), C.byref(ms), C.byref(b)))
        return {"launches": n.value, "total_ms": ms.value, "bytes_per_launch": b.value}


def merge_topk(ids: np.ndarray, scores: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Host-side final merge of per-shard candidates [S,nq,k] → [nq,k] (same tie rule)."""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    S, nq, k = ids.shape
    oi = np.empty((nq, k), dtype=np.int64)
    os_ = np.empty((nq, k), dtype=np.float32)
    L.check(L.lib().cmr_merge_topk(_ptr(ids), _ptr(scores), S, nq, k, _ptr(oi), _ptr(os_)))
    return oi, os_
