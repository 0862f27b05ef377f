/*
 * comorag_hip.h — C-ABI of libcomorag_hip.so, the MI355X (gfx950) dense-retrieval engine
 * behind ComoRAG's EmbeddingModel / EmbeddingStore Python API.
 *
 * The reference (EternityJune25/ComoRAG @ 2025-08-29) has no FFI: its boundary for this path is
 * duck-typed Python.  Each entry point below names the reference code whose
 * numeric work it replaces (paths relative to src/comorag/).  The Python host side
 * (comorag_amd/) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - every function returns int32 status: 0 = CMR_OK, < 0 = error; cmr_last_error() returns a
 *    thread-local NUL-terminated message valid until the next call on that thread.
 *  - host buffers are caller-owned, C-contiguous, never retained after return.
 *  - "_dev" variants take DEVICE pointers (e.g. torch tensors' data_ptr()) and a hipStream_t
 *    passed as void* (NULL = the legacy default stream, which is what torch's default stream
 *    handle is); they enqueue work on THAT stream and return without synchronising, so the work
 *    is ordered after the caller's earlier kernels on the stream and before its later ones.
 *    Calls on one stream must not be issued concurrently from several threads.
 *    Non-finite queries are reported (CMR_ERR_NONFINITE) by the synchronous host-buffer calls;
 *    the _dev and pipelined calls cannot report them without a sync: their outputs are then
 *    unspecified and cmr_index_query_status() tells, after the fact, that it happened.
 *  - handles are opaque; destroy(NULL) is a no-op.  All functions are thread-safe: searches on
 *    one index run concurrently (shared lock), append/destroy are exclusive; concurrent
 *    cmr_graph_ppr / cmr_index_ppr calls on one graph each take their own scratch vectors.
 *  - there is NO CPU fallback: without a visible gfx950 device every compute call fails with
 *    CMR_ERR_NO_DEVICE.
 *
 * Result order (exported tie rule): score descending, then row index ascending.  (Deviation from the reference, by
 * necessity: ComoRAG ranks with np.argsort(scores)[::-1] (ComoRAG.py:964), numpy's default introsort — not stable, so rows with
 * EQUAL scores, i.e. duplicated chunks, come out in an order numpy does not specify and that changes with the array around them.
 * The Python layer runs that very line on the GPU scores for corpora below 28672 rows and takes this library's order above;
 * tests/test_dropin_gpu.py pins both sides of the threshold.)  Scores on the
 * wire are RAW inner products; ComoRAG's min-max normalisation (utils/misc_utils.py:141-150) is
 * applied by the Python layer from out_min/out_max so its formula stays textually the
 * reference's.  Inputs must be finite IN THE INDEX DTYPE (checked: CMR_ERR_NONFINITE): NaN / Inf, and for a bf16 / f16 index also a
 * finite fp32 value that rounds to an infinity there (|v| >= 65520 in f16, |v| >= 2^127 (2 - 2^-8) ~ 3.39e38 in bf16), are refused in
 * appended rows (the index is unchanged) and in queries alike; an fp32 index takes every finite value.
 * f16 subnormals (|v| < 2^-14 after rounding) are stored and multiplied as they are: the gfx950 matrix instructions do not flush
 * them (tests/test_value_domain_gpu.py pins it).
 *
 * Encoder stages (cmr_encoder_*): the library computes the model's own functions — softmax attention, fp32 LayerNorm statistics, masked
 * mean-pool + L2 normalisation; the FFN's GELU runs in PyTorch, by default in the model's exact (erf) form.  The Python layer can OPT IN (`embedding_gelu = "epilogue"`) to hipBLASLt's bias + GELU GEMM epilogue,
 * whose GELU is the TANH form (<= 4.8e-4 per activation from the erf form: a different function from BGEEmbedding.py:120's, inside the
 * 1e-3 bar on the tested weights, never the default).
 *
 * Synchronous host-buffer calls (cmr_index_search, cmr_index_search_min_score, cmr_index_scores, and cmr_mindex_* on top of them) return
 * as soon as the results are in the caller's buffers: where the search's last kernel can report it, the host polls a word that kernel
 * stores behind its results in a pinned, device-mapped buffer instead of waiting for the stream (option sync_poll, default 1; ~5 us per
 * call).  The stream itself may still be finishing that kernel's epilogue when the call returns — invisible to the caller: every later
 * call on the index is ordered behind it.
 */
#ifndef COMORAG_HIP_H
#define COMORAG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMR_ABI_VERSION 2

enum cmr_status {
    CMR_OK = 0,
    CMR_ERR_INVALID = -1,     /* bad argument */
    CMR_ERR_NO_DEVICE = -2,   /* no usable HIP device / wrong arch */
    CMR_ERR_HIP = -3,         /* a HIP runtime call failed (message has the call) */
    CMR_ERR_OOM = -4,
    CMR_ERR_NONFINITE = -5,   /* NaN/Inf in rows or queries, or a value that rounds to Inf in the index dtype */
    CMR_ERR_UNSUPPORTED = -6  /* e.g. k above CMR_MAX_K */
};

enum cmr_dtype { CMR_F32 = 0, CMR_BF16 = 1, CMR_F16 = 2 };

/* index flags */
#define CMR_FLAG_KEEP_F32 1u /* also keep a row-major fp32 shadow (exact re-score, C5) */

#define CMR_MAX_K 128        /* largest k served by the fused scan+top-k kernel */
#define CMR_MAX_K_2PASS 4096 /* largest k overall: above CMR_MAX_K the scores of a query block are
                                materialised in HBM and selected per row (retrieve_knn's k = 2047) */

typedef struct cmr_index cmr_index_t;

/* ---- library --------------------------------------------------------------------------- */
int32_t cmr_abi_version(void);
const char* cmr_last_error(void);
/* number of visible HIP devices (0 on a CPU-only host; never an error there) */
int32_t cmr_device_count(int32_t* n);
/* name / arch / CU count / HBM bytes of a device — bench.py prints this next to the roofline */
int32_t cmr_device_info(int32_t device_id, char* name, int32_t name_len, int32_t* n_cu,
                        int64_t* hbm_bytes);

/* ---- index lifecycle -------------------------------------------------------------------
 * Replaces the dense matrices ComoRAG.prepare_retrieval_objects materialises on the host
 * (ComoRAG.py:896-900: np.array(store.get_embeddings(keys)) x3-4) and
 * EmbeddingStore.get_embeddings' per-call N x D copy (embedding_store.py:150-157).
 * Storage: HBM-resident, MFMA-fragment-major panels of 32 rows; dim is padded
 * to a multiple of 128 with zeros.  capacity grows x2 (device-to-device hipMemcpyAsync).      */
int32_t cmr_index_create(int32_t device_id, int32_t dim, int32_t dtype, int64_t capacity_hint,
                         uint32_t flags, cmr_index_t** out);
int32_t cmr_index_destroy(cmr_index_t* idx);
int32_t cmr_index_size(cmr_index_t* idx, int64_t* n_rows);
int32_t cmr_index_info(cmr_index_t* idx, int32_t* dim, int32_t* dtype, int64_t* capacity_rows,
                       int64_t* device_bytes);

/* Append n rows (fp32, row-major [n, dim]); converted round-to-nearest-even to the index dtype
 * on the device.  Row ids are assigned densely in append order (id = previous size + i) — the
 * same order EmbeddingStore._upsert extends its lists (embedding_store.py:122-128), so
 * hash_id_to_idx stays valid as the row id.  The memory-pool appends of the probe loop
 * (utils/memory_utils.py:176,297-300) use this too (BASELINE config 4).                        */
int32_t cmr_index_append(cmr_index_t* idx, const float* rows_f32, int64_t n);
int32_t cmr_index_append_dev(cmr_index_t* idx, const float* rows_f32_dev, int64_t n, void* stream);

/* ---- search ----------------------------------------------------------------------------
 * Fused scan + per-query top-k + global min/max of the raw scores.
 * Replaces np.dot + min_max_normalize + argsort in ComoRAG.dense_passage_retrieval
 * (ComoRAG.py:950-967), get_fact_scores + link_top_k argsort (ComoRAG.py:937-948,1073),
 * get_similar_summaries (utils/embed_utils.py:152-158), the python-loop cosine of
 * MemoryPool.retrieve_similar_nodes (utils/memory_utils.py:213-227) and each
 * torch.mm + torch.topk block of retrieve_knn (utils/embed_utils.py:52-78); k <= CMR_MAX_K_2PASS.
 *   q        [nq, dim] fp32 (rounded to the index dtype for bf16/f16 indexes, as BASELINE.md §2)
 *   out_ids  [nq, k] int64 row ids, -1 padded when the index has < k rows
 *   out_scores [nq, k] fp32 raw inner products, descending, -inf padded
 *   out_min/out_max [nq] fp32 over ALL rows (NULL allowed)                                     */
int32_t cmr_index_search(cmr_index_t* idx, const float* q_f32, int32_t nq, int32_t k,
                         int64_t* out_ids, float* out_scores, float* out_min, float* out_max);
/* Threshold search: the k best rows among those with raw score >= min_score (-1 / -inf padded) — the fused kernel's
 * running threshold simply starts at min_score, so nothing below it is ever pushed, merged or written.  This is what
 * the synonymy self-join consumes: ComoRAG.add_synonymy_edges (ComoRAG.py:670-712) asks retrieve_knn for 2047 neighbours
 * of every entity and then stops at the first score < synonymy_edge_sim_threshold (0.8) or after 101 accepted ones
 * (:696-699), i.e. it reads ~1/20 of what the reference materialises.  k <= CMR_MAX_K.                                  */
int32_t cmr_index_search_min_score(cmr_index_t* idx, const float* q_f32, int32_t nq, int32_t k, float min_score,
                                   int64_t* out_ids, float* out_scores);
/* The same on device buffers, enqueued on `stream` without synchronising: the self-join issues one call per query block
 * (queries uploaded once, results downloaded once) instead of an upload, a sync and a download per block.                 */
int32_t cmr_index_search_min_score_dev(cmr_index_t* idx, const float* q_f32_dev, int32_t nq, int32_t k, float min_score,
                                       int64_t* out_ids_dev, float* out_scores_dev, void* stream);
/* The threshold search in throughput mode (as cmr_index_search_pipelined below: the index's own streams, packing of block i + 1
 * and the candidate merge of block i - 1 run beside the scan of block i) — the synonymy self-join enqueues all its query blocks
 * this way and waits for the last *done_event (every merge runs on one in-order stream).                                  */
int32_t cmr_index_search_min_score_pipelined(cmr_index_t* idx, const float* q_f32_dev, int32_t nq, int32_t k, float min_score,
                                             int64_t* out_ids_dev, float* out_scores_dev, void* wait_event, void** done_event);
int32_t cmr_index_search_dev(cmr_index_t* idx, const float* q_f32_dev, int32_t nq, int32_t k,
                             int64_t* out_ids_dev, float* out_scores_dev, float* out_min_dev,
                             float* out_max_dev, void* stream);

/* Filtered search: the k best among the rows an allow bitmap keeps ("top-k among the rows not excluded").  Serves tri_retrieve's
 * memory-pool dedup (ComoRAG.py:499-505, 515-522, 535-540: the top qa_*_top_k chunks / summaries / episodes, less the ones whose hash
 * is already in the question's pool — the reference filters AFTER the top-k and so returns fewer than k; here the excluded rows never
 * compete) and one index that holds several levels or namespaces with a mask each (get_similar_summaries, utils/embed_utils.py:152-158).
 *   allow_words  one uint32 per 32-row panel over the LOCAL rows of this index (row r = the r-th appended row, before
 *                cmr_index_set_id_base / the block table): bit (r & 31) of word (r >> 5) keeps row r.  n_words == ceil(size / 32)
 *                exactly; bits at or beyond size are ignored.  One mask serves every query of the call.
 *   result       exactly what cmr_index_search returns on an index that holds only the allowed rows in their original order, every id
 *                mapped back to the original row and then translated by the id base / block table: score descending, then row id
 *                ascending; a row's score bits are those of the unfiltered search; out_min / out_max over the allowed rows only; fewer
 *                than k allowed rows: -1 / -inf padded; none: CMR_OK, all padding, min = +inf, max = -inf.
 *   k <= CMR_MAX_K (above: CMR_ERR_UNSUPPORTED), any nq >= 1 (more than 64 queries run as several narrow passes).  NULL mask / output,
 *   wrong n_words, k <= 0: CMR_ERR_INVALID, checked before any device call.  The synchronous form reports non-finite queries as
 *   cmr_index_search does; the _dev form as the other _dev calls do (cmr_index_query_status).
 * Route: always the narrow kernel's pack / [sample] / scan / merge chain on the masked variant of the scan — the panel's word stands
 * wherever the scan tests "row < rows" (min / max, threshold test, candidate push), the sampling passes read the same words, so their
 * thresholds are bounds among ALLOWED rows.  A filtered call joins a combined batch only where "combine_filtered" is set (see
 * "combine" below; by default never), never takes the int8 pre-filter, the single-launch paths or the finishing stage, and changes
 * nothing any other call returns.  last_route: CMR_ROUTE_CHAIN with CMR_ROUTE_FILTERED set.
 * The host form uploads the words into scratch of its own call (concurrent calls each have theirs); the _dev form reads the caller's
 * device words in place on `stream` — a caller that reuses one mask (a namespace, the pool's exclusion set) uploads it once.          */
int32_t cmr_index_search_masked(cmr_index_t* idx, const float* q_f32, int32_t nq, int32_t k,
                                const uint32_t* allow_words, int64_t n_words,
                                int64_t* out_ids, float* out_scores, float* out_min, float* out_max);
/* ComoRAG.py:499-505, 515-522, 535-540 on device buffers (see above): enqueued on `stream`, no synchronisation. */
int32_t cmr_index_search_masked_dev(cmr_index_t* idx, const float* q_f32_dev, int32_t nq, int32_t k,
                                    const uint32_t* allow_words_dev, int64_t n_words,
                                    int64_t* out_ids_dev, float* out_scores_dev,
                                    float* out_min_dev, float* out_max_dev, void* stream);

/* Filtered search with an allow bitmap PER QUERY: ComoRAG answers up to 16 questions at once (ComoRAG.try_answer,
 * ComoRAG.py:432-453), every question with a memory pool of its own, so the rows to keep out of tri_retrieve's top-k differ per query; a
 * serving process with several namespaces in one index has the same shape.  One corpus pass serves the batch where B one-query
 * cmr_index_search_masked calls read the corpus B times.
 *   allow_words  [nq][n_words], query-major and contiguous: query i's words at allow_words + i * n_words, each block exactly one
 *                cmr_index_search_masked bitmap (n_words == ceil(size / 32)).
 *   result       row i is bit for bit what cmr_index_search_masked(q + i * dim, 1, k, allow_words + i * n_words, ...) returns: ids, score
 *                bits, out_min[i] / out_max[i] over the rows query i allows, -1 / -inf padding.  A query that allows nothing gets all
 *                padding, min = +inf, max = -inf (the call still returns CMR_OK) and does not disturb its neighbours.
 *   Argument rules, non-finite queries and the _dev form's conventions are those of cmr_index_search_masked; any nq >= 1 (batches above
 *   the narrow kernel's width run as several passes, each on its own queries' words).
 * Route: the same chain on the per-query variant of the masked scan — in the scan's epilogue a lane owns one query column of the score
 * tile and loads that query's word of the panel; sampling passes read the same words, so each query's threshold is a bound among ITS
 * allowed rows.  last_route: CMR_ROUTE_CHAIN | CMR_ROUTE_FILTERED | CMR_ROUTE_FILTERED_EACH.
 * The host form uploads all nq blocks into scratch of its own call; the _dev form reads the caller's device words in place.
 * Filtered besides the top-k calls: the threshold search, the range search and the range count ("filtered score-bound searches" below, host
 * forms).  Not filtered: the pipelined, exact, sorted and all-scores calls, the _dev forms of the score-bound searches, PageRank; of
 * cmr_mindex_* only the _ids calls filter.                                                                                            */
int32_t cmr_index_search_masked_each(cmr_index_t* idx, const float* q_f32, int32_t nq, int32_t k,
                                     const uint32_t* allow_words, int64_t n_words,
                                     int64_t* out_ids, float* out_scores, float* out_min, float* out_max);
int32_t cmr_index_search_masked_each_dev(cmr_index_t* idx, const float* q_f32_dev, int32_t nq, int32_t k,
                                         const uint32_t* allow_words_dev, int64_t n_words,
                                         int64_t* out_ids_dev, float* out_scores_dev,
                                         float* out_min_dev, float* out_max_dev, void* stream);

/* Filtered search from ROW-ID LISTS: tri_retrieve's pool dedup has the rows to keep out as the ids earlier searches
 * returned, not as a bitmap, and a bitmap over local rows cannot cross the shards of a multi-device index.  The caller hands over ids;
 * the device builds the allow words next to the corpus (two small launches) and the masked scans above run on them unchanged.
 *   mode        CMR_IDS_EXCLUDE: every row except the listed ones; CMR_IDS_ALLOW: only the listed rows.
 *   ids         int64 row ids AS THE SEARCH ENTRY POINTS RETURN THEM (id base / block table applied), so a -1 padded result of an earlier
 *               search can be passed as it is; negative ids and ids this index does not hold are ignored; duplicates are harmless.
 *   id_offsets  int64 [nq + 1], CSR: query i owns ids[id_offsets[i] .. id_offsets[i+1]); NULL = ONE list of n_ids entries shared by
 *               every query.
 * cmr_index_row_masks_dev writes exactly the words cmr_index_search_masked(_each)_dev takes — [nq][n_words] with offsets, [n_words] without
 * (nq is then not used beyond nq >= 1), n_words == ceil(size / 32), bits at or beyond size zero — on `stream`, without synchronising: build
 * once, search many times.  Device offsets cannot be checked: malformed ones give unspecified words, never an access out of bounds.
 * cmr_index_search_ids returns, bit for bit, what cmr_index_search_masked_each returns on those words (with id_offsets == NULL:
 * cmr_index_search_masked on the one mask, on the shared-mask scan): ids, score bits, min / max over the allowed rows, -1 / -inf padding to
 * k columns; a query that allows nothing gets all padding, min = +inf, max = -inf, and CMR_OK.  n_ids == 0 is legal (exclude: every row
 * competes; allow: all padding).  k <= CMR_MAX_K (above: CMR_ERR_UNSUPPORTED), any nq >= 1.
 * CMR_ERR_INVALID, before any device call: a NULL handle, query or output; NULL ids with n_ids > 0; n_ids < 0; a mode other than 0 / 1;
 * nq or k <= 0; wrong n_words in the builder; in the host forms also id_offsets[0] != 0, decreasing offsets, id_offsets[nq] != n_ids.
 * Non-finite queries are reported as the masked calls report them.
 * Scratch: the words live in the call's own workspace (concurrent calls each have theirs) and never exceed 64 queries' worth: a larger
 * batch builds and scans group by group on one stream.  The host form uploads ids and offsets through the pinned buffer, like the
 * queries.  last_route: the masked route's bits plus CMR_ROUTE_FILTERED_IDS.  These calls are never combined (see "combine").
 * cmr_mindex_search_ids takes GLOBAL ids: every non-empty shard gets the whole list and keeps the ids it holds (no host-side split), the
 * search begins on every shard before it finishes on any, the host merges as cmr_mindex_search does; min / max over the shards (a shard
 * with nothing allowed contributes +inf / -inf); no active shard: all padding.                                                        */
#define CMR_IDS_EXCLUDE 0   /* every row except the listed ones */
#define CMR_IDS_ALLOW   1   /* only the listed rows */
int32_t cmr_index_row_masks_dev(cmr_index_t* idx, int32_t mode, int32_t nq, const int64_t* id_offsets_dev, const int64_t* ids_dev,
                                int64_t n_ids, uint32_t* words_dev /* [nq or 1][n_words] */, int64_t n_words, void* stream);
int32_t cmr_index_search_ids(cmr_index_t* idx, const float* q_f32, int32_t nq, int32_t k, int32_t mode, const int64_t* id_offsets,
                             const int64_t* ids, int64_t n_ids, int64_t* out_ids, float* out_scores, float* out_min, float* out_max);
int32_t cmr_index_search_ids_dev(cmr_index_t* idx, const float* q_f32_dev, int32_t nq, int32_t k, int32_t mode,
                                 const int64_t* id_offsets_dev, const int64_t* ids_dev, int64_t n_ids, int64_t* out_ids_dev,
                                 float* out_scores_dev, float* out_min_dev, float* out_max_dev, void* stream);

/* ROW REMOVAL by stable in-place compaction on the device (FAISS IndexFlat.remove_ids).  The listed rows go, the
 * survivors keep their relative order and are renumbered densely: local row r becomes r - #{removed rows < r}.  Afterwards the index IS
 * the shorter index — every entry point returns, bit for bit, what a fresh index built by appending the surviving rows in their old order
 * returns (ids, score bits, min / max, complete rankings, get_rows, the exact search's flags), on every route.  Two things may differ from
 * that fresh index: the index-wide maxima behind cmr_index_round_stats / cmr_index_prefilter_stats / the exact search's certificate may
 * stay at their old, larger values (still valid upper bounds: certified results do not change), and device_bytes does not shrink
 * (capacity is kept).  Row numbers held outside the index — prepacked mask words, a graph's vertex_of_row, cached result ids — are stale
 * afterwards; the caller renumbers them.
 *   ids        int64 row ids AS THE SEARCH ENTRY POINTS RETURN THEM (id base applied; cmr_mindex_remove_ids: global ids), by the rules of
 *              the id-list searches above: -1 padding, other negative ids, ids the index does not hold and duplicates are ignored, so a
 *              padded [nq, k] result of an earlier search goes in as it is.  An id base stays as it is.
 *   n_removed  (may be NULL) rows actually removed.  Removing nothing is legal and changes nothing; removing every row leaves an empty
 *              index that accepts appends.
 * Synchronous and exclusive, like an append: it waits for the searches that hold the index and then for EVERYTHING this process has
 * enqueued on the device (a device synchronise: removal is a maintenance call), so the results of _dev / pipelined calls issued before
 * the removal are complete when it returns, and calls issued after it see the shorter index.
 * CMR_ERR_INVALID, before any device call: a NULL handle, NULL ids with n_ids > 0, n_ids < 0.  CMR_ERR_UNSUPPORTED, index untouched: a
 * user-set block table of more than one block (cmr_index_set_id_blocks) — its owner removes (cmr_mindex_remove_ids).  Out of memory for
 * the scratch or the staging buffer is reported before any row moves (index untouched); after a HIP error from the copy launches the
 * rows are unspecified (the int8 companion is already marked stale from the first removed row on).
 * How: the keep words by the builder of the id-list searches, a one-workgroup prefix sum over their popcounts, then — unless nothing
 * goes or only a tail goes (a truncate) — the 16-byte slots of the panels from the first removed row's on move chunk by chunk through a
 * bounded staging buffer (the append's), ordered by one stream; the fp32 shadow of a CMR_FLAG_KEEP_F32 index likewise row by row.  The
 * int8 companion of the pre-filter is not compacted: the next pre-filtered call quantises again from the first removed row's panel.
 * Route selector "remove_stage_panels": panels the staging buffer holds (0 = default: 64 MiB worth; at least 2; never more than the
 * affected panels + 1); a chunk is that many source panels less one, because its destination rows may straddle one panel more.  Results
 * never depend on it.  Read-only "remove_chunks_last": chunks the corpus pass of the last removal ran (0: nothing moved).              */
int32_t cmr_index_remove_ids(cmr_index_t* idx, const int64_t* ids, int64_t n_ids, int64_t* n_removed /* may be NULL */);

/* IN-PLACE ROW UPDATE: the listed rows get new contents; row count, row ids, capacity, id base and block tables stay.
 * Afterwards every entry point returns, bit for bit, what a fresh index built by appending the final row contents in order returns, on
 * every route (a row's 16-byte slots are a function of that row alone).  As after a removal, two things may differ from that fresh
 * index: the index-wide maxima behind cmr_index_round_stats / the exact search's certificate, and those of the int8 companion
 * (cmr_index_prefilter_stats), are folded with an atomic max, not recomputed — they may stay larger and remain valid upper bounds.
 *   ids        int64 row ids AS THE SEARCH ENTRY POINTS RETURN THEM (id base / block table applied; cmr_mindex_update_rows: global ids),
 *              entry i paired with fp32 row i of rows [n, dim].  A negative id or an id the index does not hold is ignored together with
 *              its row; of an id that occurs several times the LAST occurrence wins and the id counts once.  A user-set block table of
 *              several blocks (cmr_index_set_id_blocks) is fine: nothing is renumbered.
 *   n_updated  (may be NULL) distinct rows replaced.  n == 0 returns 0 and touches nothing.
 * ALL OR NOTHING on bad input: a row that WOULD BE WRITTEN (the last occurrence of a held id) and is NaN / Inf or rounds to Inf in the
 * index dtype makes the call return CMR_ERR_NONFINITE with the index unchanged bit for bit — every row is checked before the first store
 * (an append may write first and check afterwards because it bumps the row count last; an update's rows are live).
 * Synchronous and exclusive, like cmr_index_remove_ids: it waits for the searches that hold the index, then for EVERYTHING this process
 * has enqueued on the device (_dev and pipelined calls hold the lock only while they enqueue: their kernels may still be reading), and
 * returns when the rows are in.  A search on another thread sees the index before or after the update, never in between.
 * CMR_ERR_INVALID, before any device call: a NULL handle, NULL ids or rows with n > 0, n < 0.
 * How: the host plans (cmr_mindex_plan_update, the only id parser: this index is its one-shard case), then three launches on one stream,
 * ordered by the stream alone — check (raises the call's flag where the packing would refuse a row), scatter (returns at once on a raised
 * flag; one lane packs and stores one 16-byte slot, 32 consecutive entries x 2 halves of one k-step per wave, plus its 8 floats of the
 * fp32 shadow on a CMR_FLAG_KEEP_F32 index; nothing outside the listed rows is written), maxima (over the winning rows).  Up to 128 KiB of
 * rows go through the append's pinned, device-mapped buffer; otherwise the rows are staged in chunks like an append's, and a call of
 * more than one chunk checks every chunk first and uploads again to write (twice the host-to-device traffic, for such calls only).
 * The int8 companion of the pre-filter is marked stale from the first updated row on before the first store is enqueued: the next
 * pre-filtered call quantises again from that row's panel and folds the new rows into the companion's maxima.
 * cmr_index_update_rows_dev: rows on the index's device (an encoder's output; `stream` = the stream that produced them, the launches go
 * there), ids on the HOST — they are few, and the host translates and orders them.  Synchronous like the host form.
 * Route selector "update_stage_rows": fp32 rows one staged chunk holds (0 = default: 256 MiB worth; a set value also keeps the call
 * off the mapped buffer).  Results never depend on it.  Read-only "update_chunks_last": chunks the last update wrote (0: nothing).   */
int32_t cmr_index_update_rows(cmr_index_t* idx, const int64_t* ids, const float* rows_f32, int64_t n, int64_t* n_updated /* may be NULL */);
int32_t cmr_index_update_rows_dev(cmr_index_t* idx, const int64_t* ids_host, const float* rows_f32_dev, int64_t n, void* stream,
                                  int64_t* n_updated /* may be NULL */);

/* Throughput mode for a stream of independent query batches (serving; bench.py).  Work is enqueued on streams owned by
 * the index: query packing + sampling passes of batch i+1 overlap the HBM-bound main scan of batch i.  On a 256-CU device
 * main scans shorter than ~1 ms (shards up to ~4 M x 768 bf16 rows) of batches of <= 64 queries run on a CU-masked pair of
 * streams (n_cu - 64 CUs; consecutive scans alternate between the two, so one scan's workgroups take over the CUs the previous
 * scan's workgroups leave) and their pre-phases on the other 64 CUs, wide batches likewise on n_cu - 32 / 32 CUs; longer scans
 * run on unmasked streams with a trimmed grid.  wait_event (hipEvent_t or NULL): inputs are ready when it
 * completes.  *done_event (hipEvent_t owned by the index): outputs are complete when it does; it is re-recorded three
 * pipelined calls later (the pipeline has three slots), so wait on it (hipStreamWaitEvent / hipEventSynchronize) before
 * then.  k <= CMR_MAX_K.  Results are identical to cmr_index_search_dev.                                               */
int32_t cmr_index_search_pipelined(cmr_index_t* idx, const float* q_f32_dev, int32_t nq, int32_t k,
                                   int64_t* out_ids_dev, float* out_scores_dev, float* out_min_dev,
                                   float* out_max_dev, void* wait_event, void** done_event);

/* Row-shard support: every row id returned by the search entry points is offset by `base` (the
 * global id of local row 0), so per-shard candidates can be all-gathered and merged as they are.  */
int32_t cmr_index_set_id_base(cmr_index_t* idx, int64_t base);
/* The same for a shard that takes INCREMENTAL appends (BASELINE config 4 at N > 1): global ids stay dense in append order
 * (embedding_store.py:122-128, utils/memory_utils.py:294-300), an append goes to the currently shortest shard, so a shard
 * holds several runs ("blocks") of consecutive global ids: local rows [local_start[b], local_start[b+1]) are global ids
 * global_start[b] + 0, 1, ...  (local_start[0] = 0; both arrays ascending; the last block is open-ended and grows with
 * cmr_index_append).  Every id the search entry points return is translated through the table (one extra tiny launch
 * when there is more than one block), cmr_index_rescore / cmr_index_get_rows translate the ids they are given.  Global
 * ids must stay < 2^32 - 1 (the packed candidate exchange carries 32-bit rows): checked here and by append.            */
int32_t cmr_index_set_id_blocks(cmr_index_t* idx, int32_t n_blocks, const int64_t* local_start, const int64_t* global_start);
/* Route selectors.  Each option picks between implementations that return the SAME results (the tests hold the routes
 * against each other bit for bit; tools A/B kernel decisions with them).  Nothing is read from the environment by the
 * shipped library.  Names: scan_ring (8 | 16), scan_asm_ring (0 | 1), scan_grid, scan_no_sample, scan_no_wide (batches of
 * more than 64 queries as narrow passes), scan_no_tiny / scan_no_small / small_max_panels / tiny_multi (single-launch
 * paths), zero_copy, sample_single, sample_single_max, sample_tau_in_scan, sample_div, sample_maxmul, scan_fin (0: small synchronous
 * batches run the sampling / scan / merge chain instead of the scan with the finishing stage) / scan_fin_queries (<= 16) /
 * scan_fin_dense / scan_fin_spin / scan_fin_suppliers / scan_fin_cap, sync_poll (0: synchronous calls wait for the stream), wide_mode (1: register-resident wide kernel | 2: query-split grid of the narrow kernel),
 * stream_nt, pipe_reserve_cus, pipe_slots (2..4), pipe_cu_mask (0: never | 1 | 2: every scan; default: scans shorter than ~1 ms) and
 * pipe_dual_scan (0 | 1; default: scans shorter than ~1 ms) — the pipelined search's streams with explicit CU masks (scans
 * of <= 64-query batches on n_cu - 64 CUs, their pre-phases on the other 64) and two alternating scan streams; both must
 * be set before the first pipelined call.
 * The certified int8 pre-filter of the pipelined 16-bit scan: prefilter (-1 auto | 0 | 1 | 2: the filter keeps every
 * row), prefilter_rescore_wgs, prefilter_tighten (1, the default: the k-th largest certified lower bound among a query's hits replaces
 * its sampling threshold in front of the re-score | 0: every hit is re-scored) and prefilter_pair_cap (hit records per query the
 * tightening selects from, 16 bytes each, clamped to [0, 2^20], default 16384; a query with more hits keeps the rest directly; 0:
 * as prefilter_tighten = 0) and prefilter_wave_cap (hit records per wave of the filter's grid, which writes them to an area of its own
 * before they are sorted into the queries' lists, 16 bytes each, clamped to [0, 2^20]; 0, the default: as many as the queries' lists
 * hold, spread over the waves and rounded up to a multiple of 64; a wave with more hits keeps the rest directly).
 * prefilter_sample (-1 auto, currently off | 0: the level-1 sampling threshold of a pre-filtered pass comes from the 16-bit panels, scan
 * + merge as on every other route | 1: from the int8 companion — the filter's loop over strided runs of panels, its records sorted by
 * query, the k-th largest certified lower bound as the threshold; only where the pass keeps record lists: prefilter = 1,
 * prefilter_tighten = 1, prefilter_pair_cap > 0, 4096 panels or more), with prefilter_sample_panels (0 auto: 8192; a forced value is
 * taken as it is, up to every panel), prefilter_sample_run (panels per wave, 0 auto: 16), prefilter_sample_wave_cap (records per wave
 * of the sample's grid, 0 auto; a hit beyond it is dropped) and prefilter_sample_level0 (panels of the 16-bit level 0 in front of it,
 * 0 auto: 64; at least k, at most 128).
 * cmr_index_get_option reads, of the last pre-filtered pass and waiting for the pipeline:
 * prefilter_candidates (rows handed to the re-score), prefilter_pairs (hit records stored, summed over the queries),
 * prefilter_pair_overflow (queries that had more hits than records) and prefilter_wave_overflow (waves that had more hits than records);
 * prefilter_sample_active (did the pass sample from the companion; does not wait), prefilter_sample_pairs and prefilter_sample_overflow
 * (records the sample stored, and queries whose sample list filled).
 * Unknown names: CMR_ERR_INVALID.
 * The wide-batch kernel exists for padded dims 768 (256 queries per pass) and 1024 (128 per pass) in bf16 / f16; any other
 * dim and every fp32 index run a batch of B > 64 queries on the query-split grid of the narrow kernel (up to four query tiles
 * per corpus pass) — same results.                                                                                           */
int32_t cmr_index_set_option(cmr_index_t* idx, const char* name, int64_t value);
/* Combining concurrent callers (comorag_amd/csrc/combine.h).  "combine" = 0 (default: off) or W in [2, 16]: single
 * calls that several threads issue on this index at the same time share ONE batched call of up to W queries and each caller gets the bits of
 * its own call —
 *   cmr_index_search  (same k, k <= CMR_MAX_K, nq < W),  cmr_index_scores  (nq < W),
 *   cmr_index_ppr     (same graph, passage_node_weight, damping, tol, max_iter; runs as cmr_index_ppr_batch),
 *   cmr_index_ppr_ranked  (the same and the same n_out; runs as cmr_index_ppr_ranked_batch).
 * "combine_wait_us" (default 0): the gather window — the first caller waits until W queries have joined or the window has passed; at 0
 * batches form only from calls that arrive while an earlier batch is on the device, and a caller alone runs its unchanged single call.
 * A call with a NaN / Inf query, or with arguments the call refuses, never joins a batch: it gets its own error.
 * Read-only: "combine_batches" (device calls made for combined work), "combine_queries" (queries they served), "combine_max_width".
 * "combine_filtered" = 0 (default) | 1: with "combine" on, cmr_index_search_masked and cmr_index_search_masked_each calls (same k, same
 * n_words, k <= CMR_MAX_K, nq < W) are combined too — with each other, never with unfiltered calls: the batch runs as ONE
 * cmr_index_search_masked_each over the participants' queries, every query with its caller's mask (a shared mask repeated per query), and
 * each caller gets the bits of its own call.  A participant whose n_words no longer fits the index when the batch runs (an append came in
 * between) gets its own CMR_ERR_INVALID; the others are served.  At 0 filtered calls never join a batch and never move the counters.
 * NOT combined: cmr_index_search_masked* unless "combine_filtered" is set, cmr_index_search_ids* and cmr_mindex_search_ids whether or not it is set, cmr_index_search_min_score, cmr_index_sorted_scores, cmr_index_range_search / _count, cmr_index_search_exact, cmr_graph_ppr, every _dev / pipelined call,
 * cmr_mindex_* (the option has no effect on searches issued through a multi-device handle).  The encoder is not combined HERE: concurrent
 * one-question encodes share one forward through the Python-level option `embedding_combine` (cmr_encoder_linear_rows* below).      */
/* Which path served the last call (read-only): "last_route", written by the host when a search or all-scores call on this index is
 * planned (for a batch of several corpus passes: its first pass); 0 before the first call.  Concurrent callers overwrite each other.
 *   bits 0..3   the path, CMR_ROUTE_*
 *   bits 4..5   sampling levels in front of the main scan (0, 1, 2)
 *   bit  6      the one sampling level's thresholds are derived inside the main scan (sample_tau_in_scan)
 *   bit  7      that level is the single 128-panel sample of a small batch (sample_single)
 *   bits 8..9   query tiles of 32 per workgroup (1, 2)
 *   bit  10     threshold search (cmr_index_search_min_score*)
 *   bit  11     the batch took more than one corpus pass: the bits above describe its first, later passes may be routed otherwise
 *   bit  12     filtered search (cmr_index_search_masked*): every scan of the pass is the masked variant
 *   bit  13     with bit 12: the per-query variant (cmr_index_search_masked_each*, or a combined batch of filtered calls)
 *   bit  14     with bit 12: the allow words were built on the device from row-id lists (cmr_index_search_ids*)
 *   bit  15     diversified top-k (cmr_index_search_mmr*): the bits below describe the candidate search in front of the selection   */
#define CMR_ROUTE_MORE_PASSES (1 << 11)
#define CMR_ROUTE_FILTERED (1 << 12)
#define CMR_ROUTE_FILTERED_EACH (1 << 13)
#define CMR_ROUTE_FILTERED_IDS (1 << 14)
#define CMR_ROUTE_MMR (1 << 15)
#define CMR_ROUTE_TINY 1          /* single launch, <= 1024 rows */
#define CMR_ROUTE_SMALL 2         /* single launch, hierarchical selection */
#define CMR_ROUTE_CHAIN 3         /* narrow kernel: pack / [sample] / scan / merge */
#define CMR_ROUTE_FIN 4           /* narrow kernel with the finishing stage */
#define CMR_ROUTE_WIDE 5          /* register-resident wide kernel */
#define CMR_ROUTE_QUERY_SPLIT 6   /* query-split grid of the narrow kernel */
#define CMR_ROUTE_LARGE_K 7       /* k > CMR_MAX_K: all scores, then per-row selection */
#define CMR_ROUTE_SCORES_SINGLE 8 /* cmr_index_scores, single launch */
#define CMR_ROUTE_SCORES 9        /* cmr_index_scores, general scan */
#define CMR_ROUTE_SORTED 10       /* cmr_index_sorted_scores: general scan + radix sort */
#define CMR_ROUTE_RANGE 11        /* cmr_index_range_search / _count: general scan + count / compaction / radix sort */
/* What the pipeline actually does (read-only): "pipe_dual_scan_active" / "pipe_dual_scan_wide_active" (the last pipelined <= 64-query / wide pass alternated between
 * the two scan streams: by default only scans shorter than ~1 ms do — launches that overlap have no per-launch duration, so a
 * caller that times kernels must know), "pipe_cu_mask_active", "pipe_scan_cus".                                            */
int32_t cmr_index_get_option(cmr_index_t* idx, const char* name, int64_t* value);
/* The pipeline's streams (which = 0 pre-phase and 1 first main-scan stream of the <= 64-query batches, 2 candidate merges /
 * outputs of every batch) as hipStream_t.  Work enqueued on stream 2 after a pipelined call is ordered after that call's
 * outputs and before the next use of the same output buffers (the RCCL exchange goes there).     */
int32_t cmr_index_pipeline_stream(cmr_index_t* idx, int32_t which, void** stream);

/* Did any _dev / pipelined search since the last call see a NaN/Inf query?  Synchronises the index's pipeline streams
 * and the streams used with the _dev API, reads and re-arms their flags.  *nonfinite = 0 / 1.                        */
int32_t cmr_index_query_status(cmr_index_t* idx, int32_t* nonfinite);

/* Helpers for callers that only hold opaque handles (e.g. a torch stream's cuda_stream):
 * make `stream` (hipStream_t) wait for `event` (hipEvent_t from *done_event), or block the host.  */
int32_t cmr_stream_wait_event(void* stream, void* event);
int32_t cmr_event_synchronize(void* event);

/* All N raw scores per query, out [nq, ld] fp32 (ld >= N; ld = N when 0).  For the callers that
 * consume every score: graph_search_with_fact_entities reads all (id, score) pairs of
 * dense_passage_retrieval (ComoRAG.py:1034-1042) and get_fact_scores returns the full vector
 * (ComoRAG.py:937-948).                                                                        */
int32_t cmr_index_scores(cmr_index_t* idx, const float* q_f32, int32_t nq, float* out, int64_t ld);
int32_t cmr_index_scores_dev(cmr_index_t* idx, const float* q_f32_dev, int32_t nq, float* out_dev,
                             int64_t ld, void* stream);

/* ALL N rows of each query by descending raw score (ties: ascending row id), out_ids / out_scores
 * [nq, N]; out_min / out_max [nq] (NULL allowed) are the last / first sorted score.  Replaces the
 * np.dot + full argsort of ComoRAG.dense_passage_retrieval (ComoRAG.py:958-966) for callers that
 * need the complete ranking: scan on MFMA, then a stable device radix sort.                       */
int32_t cmr_index_sorted_scores(cmr_index_t* idx, const float* q_f32, int32_t nq, int64_t* out_ids,
                                float* out_scores, float* out_min, float* out_max);

/* ---- range search ------------------------------------------------------------------------
 * EVERY row with raw score >= min_score, as per-query lists (FAISS range_search): what the synonymy join asks for when it reads
 * neighbours down to synonymy_edge_sim_threshold (ComoRAG.add_synonymy_edges, ComoRAG.py:670-712, over retrieve_knn,
 * utils/embed_utils.py:8-97) without the cap of CMR_MAX_K entries that cmr_index_search_min_score has and cannot report.
 *   list i     all rows r with score(i, r) >= min_score, compared as the threshold search compares (the order-preserving code of the
 *              fp32 bits, -0.0 and +0.0 one value): a row that attains the bound is in, the next fp32 value below is out.  Order: score
 *              descending, then row id ascending — the first c_i entries of row i of cmr_index_sorted_scores.  A row's score bits are
 *              those cmr_index_scores returns for it (gathered, never decoded from a key: a -0.0 stays -0.0); ids carry the id base /
 *              block table as every search's do.
 *   result     CSR: lims int64 [nq + 1] (lims[0] = 0), ids int64 [lims[nq]], scores fp32 [lims[nq]].  The library owns the arrays
 *              (their size is known only after the count): cmr_range_result_view's pointers are valid until cmr_range_result_destroy.
 *   bounds     +inf: empty lists; -inf and -FLT_MAX: every row; NaN: CMR_ERR_INVALID.  Empty index: nq empty lists, CMR_OK.
 *   max_total  <= 0: the library's limit, CMR_RANGE_MAX_TOTAL hits.  A batch whose total exceeds the limit: CMR_ERR_UNSUPPORTED with the
 *              total in the message, *out = NULL, nothing allocated for the result, no compaction or sort run.  cmr_index_range_count has
 *              no such limit: it is how a caller sizes a request.  cmr_index_range_count_dev enqueues on `stream` and never synchronises.
 * Any nq >= 1; rows < 2^32.  A NULL handle, query or output, nq <= 0 or a NaN bound: CMR_ERR_INVALID, before any device call.  A NaN / Inf
 * query: CMR_ERR_NONFINITE (the synchronous calls).  The calls take the shared lock like a search, use a workspace of their own and are
 * never combined, pipelined or filtered and never take the int8 pre-filter.  last_route: CMR_ROUTE_RANGE.
 * How: per block of queries (at most 2 GiB of scores; option "range_block_queries", 0 = that rule) the scan materialises the scores, a
 * count kernel counts the hits per (query, tile of CMR_RANGE_TILE rows) by wave ballots, one workgroup turns the counters into offsets
 * and per-query counts — the call's one small round trip per block —, a compaction kernel places every hit at its offset (no atomic
 * decides a position) with the key (query << 32 | complemented score code), a stable LSD radix sort orders them, a last kernel gathers
 * ids and score bits.  Option "range_scratch_hits" (0 = 1 GiB worth) bounds the hits compacted and sorted at once: a block with more is
 * done in groups of consecutive queries from the same scores, one query is never split.  Results never depend on the two options; read-only
 * "range_blocks_last" / "range_groups_last" tell how many blocks / groups the last call ran.
 * cmr_range_merge (pure host, no device): per-shard results of the same nq queries — each list in the exported order, ids disjoint —
 * merged per query by the exported tie rule; out_lims [nq + 1], out_ids / out_scores [sum of the shards' totals].                     */
#define CMR_RANGE_TILE 2048
#define CMR_RANGE_MAX_TOTAL 2147483647ll
typedef struct cmr_range_result cmr_range_result_t;
int32_t cmr_index_range_count(cmr_index_t* idx, const float* q_f32, int32_t nq, float min_score, int64_t* out_counts /*[nq]*/);
int32_t cmr_index_range_count_dev(cmr_index_t* idx, const float* q_f32_dev, int32_t nq, float min_score, int64_t* out_counts_dev,
                                  void* stream);
int32_t cmr_index_range_search(cmr_index_t* idx, const float* q_f32, int32_t nq, float min_score, int64_t max_total,
                               cmr_range_result_t** out);
int32_t cmr_range_result_view(const cmr_range_result_t* res, int32_t* nq, const int64_t** lims, const int64_t** ids, const float** scores);
int32_t cmr_range_result_destroy(cmr_range_result_t* res);      /* NULL is a no-op */
int32_t cmr_range_merge(int32_t n_shards, int32_t nq, const int64_t* const* lims, const int64_t* const* ids, const float* const* scores,
                        int64_t* out_lims, int64_t* out_ids, float* out_scores);

/* ---- filtered score-bound searches ------------------------------------------
 * The threshold search, the range search and the range count among the rows a filter keeps: every row of ONE namespace or level at or
 * above a similarity (get_similar_summaries over the level stores, utils/embed_utils.py:152-158; a serving index with several
 * namespaces), and tri_retrieve's searches that keep the question's memory pool out (ComoRAG.py:499-505, 515-522, 535-540) with the
 * synonymy join's score bound (ComoRAG.add_synonymy_edges, ComoRAG.py:670-712).  Host forms only.
 *   allow_words  exactly cmr_index_search_masked's bitmap: one uint32 per 32-row panel over the LOCAL rows, n_words == ceil(size / 32), bits
 *                at or beyond size ignored.  n_masks == 1: [n_words], one mask for every query; n_masks == nq: [nq][n_words], query i's
 *                words at allow_words + i * n_words.  Any other n_masks: CMR_ERR_INVALID.
 *   mode, id_offsets, ids, n_ids   exactly cmr_index_search_ids's lists: ids as the searches return them (id base / block table applied;
 *                cmr_mindex_*: global ids); negative ids, ids not held and duplicates are ignored; id_offsets == NULL: one shared list,
 *                otherwise CSR with nq + 1 offsets.
 * Range search / count: list i is list i of cmr_index_range_search on the same index with the entries of disallowed rows removed, bit for
 *   bit — order, ids, fp32 score words; the comparison with the bound is that call's (a row that attains it is in, -0.0 and +0.0 one
 *   value, NaN: CMR_ERR_INVALID); +inf: empty lists; -inf: every ALLOWED row, the complete ranking of a namespace.  out_counts[i] is the
 *   length of list i.  max_total is judged on the FILTERED total: above it CMR_ERR_UNSUPPORTED with that total in the message, *out = NULL,
 *   nothing compacted, sorted or allocated.  A query that allows nothing: an empty list, count 0, CMR_OK, its neighbours undisturbed.
 * Threshold search: row i is row i of cmr_index_search_masked / _masked_each / _ids with the same k and filter, every entry whose score is
 *   below the bound replaced by -1 / -inf padding, bit for bit.  k <= CMR_MAX_K (above: CMR_ERR_UNSUPPORTED); no min / max output, as
 *   cmr_index_search_min_score.
 * CMR_ERR_INVALID before any device call: a NULL handle, query or output; NULL words; n_words != ceil(size / 32); n_masks not 1 or nq; nq
 * or k <= 0; a NaN bound; a mode other than 0 / 1; NULL ids with n_ids > 0, n_ids < 0; id_offsets[0] != 0, decreasing offsets,
 * id_offsets[nq] != n_ids — every check but n_words before the handle is looked at.  Non-finite queries: as the unfiltered calls.
 * How: the range pipeline of cmr_index_range_search with masked variants of its count and compaction kernels — a hit is a row whose code is
 *   at or above the bound AND whose allow bit is set; a lane's four consecutive rows share one word of the query's mask, so it is one
 *   word load per lane and never a word at or beyond n_words; ranks still come from the ballots; offsets, sort and gather are the
 *   unfiltered call's.  The threshold search is the narrow masked chain of cmr_index_search_masked with the bound as every query's first
 *   threshold (no sampling passes).  The words live in the call's own workspace; the id forms build them there with the launches of
 *   cmr_index_row_masks_dev, never more than 64 queries' worth: per-query id lists run in blocks of at most 64 queries (which caps
 *   "range_block_queries" there).  Results never depend on the blocks or groups.  Never combined, never the int8 pre-filter, the
 *   single-launch paths or the finishing stage; nothing any other call returns changes.
 * last_route: CMR_ROUTE_RANGE, or CMR_ROUTE_CHAIN with the threshold bit, plus CMR_ROUTE_FILTERED, plus CMR_ROUTE_FILTERED_EACH where every
 *   query has words or a list of its own (n_masks > 1, id_offsets != NULL), plus CMR_ROUTE_FILTERED_IDS in the id forms.
 * cmr_mindex_*_ids (further down): every non-empty shard gets the whole lists and keeps the ids it holds, the work begins on every shard
 *   before it finishes on any, the host merges as the unfiltered calls do (cmr_range_merge / the top-k merge) — the result of one index
 *   holding the same rows, bit for bit; max_total is judged on the sum over the shards before any shard compacts.                        */
int32_t cmr_index_search_min_score_masked(cmr_index_t* idx, const float* q_f32, int32_t nq, int32_t k, float min_score,
                                          const uint32_t* allow_words, int64_t n_words, int32_t n_masks /* 1 | nq */, int64_t* out_ids,
                                          float* out_scores);
int32_t cmr_index_search_min_score_ids(cmr_index_t* idx, const float* q_f32, int32_t nq, int32_t k, float min_score, int32_t mode,
                                       const int64_t* id_offsets, const int64_t* ids, int64_t n_ids, int64_t* out_ids, float* out_scores);
int32_t cmr_index_range_count_masked(cmr_index_t* idx, const float* q_f32, int32_t nq, float min_score, const uint32_t* allow_words,
                                     int64_t n_words, int32_t n_masks /* 1 | nq */, int64_t* out_counts /*[nq]*/);
int32_t cmr_index_range_count_ids(cmr_index_t* idx, const float* q_f32, int32_t nq, float min_score, int32_t mode, const int64_t* id_offsets,
                                  const int64_t* ids, int64_t n_ids, int64_t* out_counts /*[nq]*/);
int32_t cmr_index_range_search_masked(cmr_index_t* idx, const float* q_f32, int32_t nq, float min_score, int64_t max_total,
                                      const uint32_t* allow_words, int64_t n_words, int32_t n_masks /* 1 | nq */, cmr_range_result_t** out);
int32_t cmr_index_range_search_ids(cmr_index_t* idx, const float* q_f32, int32_t nq, float min_score, int64_t max_total, int32_t mode,
                                   const int64_t* id_offsets, const int64_t* ids, int64_t n_ids, cmr_range_result_t** out);

/* Exact fp32 re-score of candidate rows (BASELINE config 5 "cross-scores on top-100").  The
 * reference's rerank.py is an LLM filter with no numeric scoring (rerank.py:100-123); this is
 * the numeric stage the engine adds behind the same (indices, items, {'confidence'}) shape.
 * Uses the fp32 shadow when the index was created with CMR_FLAG_KEEP_F32, otherwise the stored
 * (rounded) rows with fp32 queries.  cand [nq, n_cand] int64 row ids as the search entry points
 * return them (i.e. including the cmr_index_set_id_base offset; -1 = skip); out_ids likewise.   */
int32_t cmr_index_rescore(cmr_index_t* idx, const float* q_f32, int32_t nq, const int64_t* cand,
                          int32_t n_cand, int32_t k, int64_t* out_ids, float* out_scores);

/* Exact fp32 top-k from a 16-bit index (CMR_FLAG_KEEP_F32): the ids and scores of the reference's fp32 np.dot + argsort
 * (ComoRAG.py:958-966), with a per-query certificate.  Stage 1 takes the scan's top-kc (option exact_cand, default
 * CMR_MAX_K, > k) and re-scores them in fp32 from the shadow (a fixed-order fmaf chain: the same row gets the same score from every
 * call and shard layout).  Certificate: |scan - fp32| <= E_q = ||dq|| M_x + ||q|| M_dx + 2 dim 2^-23 ||q~|| M_x for every row, so
 * exact = 1 when the list holds every row or its last scan score is < (k-th scan score) - 2 E_q: then no row outside it can enter.
 *   k <= 64; out_ids / out_scores [nq, k] (score descending, then id ascending; -1 / -inf padded), out_exact [nq] int32 0 / 1.
 *   Synchronous call: queries stage 1 leaves uncertified run again on CMR_MAX_K_2PASS candidates of the two-pass search; a query
 *   still uncertified comes back with exact = 0 and the fp32 top-k of those candidates.  An fp32 index runs the plain search
 *   (exact by construction, every flag 1); a 16-bit index without the shadow: CMR_ERR_UNSUPPORTED.                            */
int32_t cmr_index_search_exact(cmr_index_t* idx, const float* q_f32, int32_t nq, int32_t k, int64_t* out_ids, float* out_scores,
                               int32_t* out_exact);
/* The exact search in throughput mode (ComoRAG.py:958-966): stage 1 only, on the pipeline of cmr_index_search_pipelined; the
 * re-score + certificate (as above: exact = 1 when nothing outside the kc candidates can beat the k-th by more than 2 E_q) runs
 * on the post stream (stream 2) and *done_event is recorded behind it.  Device buffers; exact_dev [nq] int32.  Queries with
 * exact = 0 may be asked again through cmr_index_search_exact.                                                                 */
int32_t cmr_index_search_exact_pipelined(cmr_index_t* idx, const float* q_f32_dev, int32_t nq, int32_t k, int64_t* ids_dev,
                                         float* scores_dev, int32_t* exact_dev, void* wait_event, void** done_event);
/* The certificate's index-wide maxima in use (ComoRAG.py:958-966 is what they make exact): M_x = max ||round(x)|| and
 * M_dx = max ||round(x) - x|| over every appended row, rounded up; 0 for an fp32 index (E_q = ||dq|| M_x + ||q|| M_dx + ...).   */
int32_t cmr_index_round_stats(cmr_index_t* idx, float* max_row_norm, float* max_round_err);
/* The int8 companion behind the option "prefilter" (certified int8 pre-filter of cmr_index_search_pipelined on a 16-bit index:
 * the main pass streams int8 rows, keeps the rows whose 16-bit score could still reach the threshold by a proven bound and scores
 * those again from the 16-bit rows — same ids, same score bits): the maxima its bound uses, M_x = max ||x|| and max ||x - a m||
 * (a, m: a stored row's scale and int8 values) over the rows quantised so far, rounded up; 0 while there is no companion.        */
int32_t cmr_index_prefilter_stats(cmr_index_t* idx, float* max_row_norm, float* max_quant_err);

/* Gather rows back to the host as fp32 (dequantised), out [n, dim]; ids as returned by search (with the id base). */
int32_t cmr_index_get_rows(cmr_index_t* idx, const int64_t* ids, int64_t n, float* out);

/* ---- diversified top-k: maximal marginal relevance ----------------------------------------------------
 * ComoRAG's corpora are near-duplicates by construction (overlapping chunks, summaries of sliding windows, fused notes) and
 * tri_retrieve removes exact hash matches only (ComoRAG.py:499-505, 515-522, 535-540).  These calls re-rank F candidates so that each
 * pick trades relevance against similarity to the rows already picked, on the device, bit for bit reproducible.
 *   Pair score  pair(a, b): the fp32 value cmr_index_scores returns for (query = stored row a as cmr_index_get_rows gives it, corpus
 *     row b) — stored (rounded) rows on both sides, also with CMR_FLAG_KEEP_F32.
 *   Selection, per query: positions 0 .. F-1 with ids, relevance rel (fp32) and G[s][c] = pair(id[s], id[c]).  A position is VOID when
 *     its id is negative, the index does not hold it, or an earlier position carries the same id; void positions are never picked and
 *     never penalise.  fp32 throughout, lam32 = (float)lam, oml = 1.0f - lam32.  Pick 1: the non-void position of largest rel.  Every later
 *     pick: the non-void unpicked position of largest (lam32 * rel[c]) - (oml * pen[c]), pen[c] = max of G[s][c] over the picked s — both
 *     products rounded to fp32, then one subtraction, no fused multiply-add.  IEEE comparisons (-0.0 == +0.0), ties to the lowest
 *     position; it stops after k picks or when no position is left.  Output in pick order: ids as given, scores = the rel bits of the
 *     picked positions, the rest -1 / -inf.  lam = 1 gives the first k non-void candidates in order — for cmr_index_search_mmr exactly
 *     cmr_index_search(q, k); scores are raw inner products (cosines on L2-normalised rows, MMR's usual form).
 *   Arguments, checked before the handle: NULL -> CMR_ERR_INVALID; nq >= 1, 1 <= k <= F (fetch_k), lam in [0, 1] and not NaN, else
 *     CMR_ERR_INVALID; F > CMR_MAX_K -> CMR_ERR_UNSUPPORTED.  The host forms refuse NaN among the candidate scores (CMR_ERR_INVALID).
 *   Never combined, pre-filtered or pipelined.
 * cmr_mmr_select: the selection alone on host arrays (no device; void = negative or repeated id).  rel [nq, F], gram [nq, F, F],
 *   ids [nq, F] -> out [nq, k].
 * cmr_index_pair_scores: out [nq, F, F], out[q][s][c] = pair(ids[q][s], ids[q][c]), -inf in the rows and columns of void positions.
 * cmr_index_mmr_select(_dev): the selection over candidates of ANY earlier search (padded results go straight in); _dev: device
 *   buffers, enqueued on `stream`.
 * cmr_index_search_mmr(_dev): the ordinary search for fetch_k on whichever route the plan picks, the pair scores and the selection on one
 *   stream; only [nq, k] goes to the host, in one round trip.  last_route: the candidate search's route with CMR_ROUTE_MMR set.
 * cmr_mindex_*: the same over global ids; every shard scores all candidate rows against the candidates it holds, the host assembles G
 *   and selects (cmr_mmr_select).  Results equal one index holding the same rows, bit for bit.                                      */
int32_t cmr_mmr_select(const float* rel, const float* gram, const int64_t* ids, int32_t nq, int32_t F, int32_t k, double lam,
                       int64_t* out_ids, float* out_scores);
int32_t cmr_index_pair_scores(cmr_index_t* idx, const int64_t* ids, int32_t nq, int32_t F, float* out);
int32_t cmr_index_mmr_select(cmr_index_t* idx, const int64_t* cand_ids, const float* cand_scores, int32_t nq, int32_t F, int32_t k,
                             double lam, int64_t* out_ids, float* out_scores);
int32_t cmr_index_mmr_select_dev(cmr_index_t* idx, const int64_t* cand_ids_dev, const float* cand_scores_dev, int32_t nq, int32_t F,
                                 int32_t k, double lam, int64_t* out_ids_dev, float* out_scores_dev, void* stream);
int32_t cmr_index_search_mmr(cmr_index_t* idx, const float* q_f32, int32_t nq, int32_t k, int32_t fetch_k, double lam, int64_t* out_ids,
                             float* out_scores);
int32_t cmr_index_search_mmr_dev(cmr_index_t* idx, const float* q_f32_dev, int32_t nq, int32_t k, int32_t fetch_k, double lam,
                                 int64_t* ids_dev, float* scores_dev, void* stream);

/* ---- multi-shard merge ------------------------------------------------------------------
 * Final merge of per-shard candidates after the RCCL all-gather (no reference counterpart;
 * SURVEY.md §8e).  ids/scores [n_shards, nq, k] (ids already global, -1 = empty); same tie rule,
 * so the result equals a single-shard search.  Host version and device version.               */
int32_t cmr_merge_topk(const int64_t* ids, const float* scores, int32_t n_shards, int32_t nq,
                       int32_t k, int64_t* out_ids, float* out_scores);
int32_t cmr_merge_topk_dev(int32_t device_id, const int64_t* ids_dev, const float* scores_dev,
                           int32_t n_shards, int32_t nq, int32_t k, int64_t* out_ids_dev,
                           float* out_scores_dev, void* stream);

/* ---- graph stage: DPR-seeded personalised PageRank --------------------------------------
 * Replaces the tail of ComoRAG.graph_search_with_fact_entities (ComoRAG.py:1034-1044: every (passage id, normalised
 * DPR score) pair copied to the host and scattered into `passage_weights`) and ComoRAG.run_ppr (:1086-1105: igraph /
 * prpack personalised PageRank — undirected, edge attribute 'weight', damping 0.5 — then pagerank[passage_node_idxs]).
 *   cmr_graph_create           undirected weighted edge list (igraph's get_edgelist() + es['weight']; weight NULL = 1)
 *                              -> symmetric CSR in HBM.  A vertex without edges jumps according to the reset vector.
 *   cmr_graph_set_passage_vertices   vertex of every passage ROW of the index (ComoRAG's passage_node_idxs)
 *   cmr_graph_ppr              run_ppr alone: reset [n_vertices] (negative / NaN -> 0, ComoRAG.py:1090) -> all scores
 *   cmr_index_ppr              the fused path for one query: scan -> min_max_normalize(scores) * passage_node_weight
 *                              scattered into the reset vector on the device, + the (few) phrase seeds (duplicate seed
 *                              vertices are SUMMED; ComoRAG's own loop assigns, last wins, :1019-1021 — resolve before the call) -> PPR ->
 *                              out_doc_scores [n_rows] = pagerank[vertex of row]; 8 * n_rows bytes come back instead of
 *                              the 12 * N of the full ranking.  The caller sorts (np.argsort(doc_scores)[::-1], :1102) — or calls
 *                              cmr_index_ppr_ranked below, which sorts on the device.
 * Power iteration in fp64, ceil(log(tol/2)/log(damping)) steps (<= max_iter; *iters = steps taken), fixed summation
 * order.  prpack solves the same linear system directly to ~1e-10.                                                     */
typedef struct cmr_graph cmr_graph_t;
int32_t cmr_graph_create(int32_t device_id, int64_t n_vertices, int64_t n_edges, const int32_t* src, const int32_t* dst,
                         const double* weight, cmr_graph_t** out);
int32_t cmr_graph_destroy(cmr_graph_t* g);
int32_t cmr_graph_set_passage_vertices(cmr_graph_t* g, const int32_t* vertex_of_row, int64_t n_rows);
int32_t cmr_graph_ppr(cmr_graph_t* g, const double* reset, double damping, double tol, int32_t max_iter, double* out_scores,
                      int32_t* iters);
int32_t cmr_index_ppr(cmr_index_t* idx, cmr_graph_t* g, const float* q_f32, const int32_t* seed_vertices,
                      const double* seed_weights, int32_t n_seeds, double passage_node_weight, double damping, double tol,
                      int32_t max_iter, double* out_doc_scores, int32_t* iters);
/* The same for nb <= CMR_PPR_MAX_BATCH queries per power iteration (ComoRAG.try_answer, ComoRAG.py:432-453, runs up to 16
 * graph searches at once, each ending in run_ppr :1086-1105): the graph is read once per step for all of them.  More than
 * CMR_PPR_MAX_BATCH: CMR_ERR_UNSUPPORTED (split the batch; comorag_amd/ppr.py does).  Arguments are checked before any
 * device call (CMR_ERR_INVALID).  One NaN / Inf query fails the whole batch (CMR_ERR_NONFINITE).
 *   cmr_graph_ppr_batch   run_ppr for nb reset vectors (:1086-1105 from each thread of :432-453): reset / out_scores
 *                         [nb, n_vertices] row-major, the caller's vertex order; row b equals cmr_graph_ppr(reset[b]) bit for bit.
 *   cmr_index_ppr_batch   cmr_index_ppr for nb queries (:1034-1044 + :1086-1105 each): q_f32 [nb, dim]; seeds in CSR form:
 *                         seed_offsets [nb + 1], seed_vertices / seed_weights [seed_offsets[nb]] (duplicates within one query
 *                         are summed in input order, as in cmr_index_ppr); out_doc_scores [nb, n_rows].  Row b equals
 *                         cmr_index_ppr(q[b], seeds of b) bit for bit.                                                       */
#define CMR_PPR_MAX_BATCH 16
int32_t cmr_graph_ppr_batch(cmr_graph_t* g, const double* reset, int32_t nb, double damping, double tol, int32_t max_iter,
                            double* out_scores, int32_t* iters);
int32_t cmr_index_ppr_batch(cmr_index_t* idx, cmr_graph_t* g, const float* q_f32, int32_t nb, const int32_t* seed_offsets,
                            const int32_t* seed_vertices, const double* seed_weights, double passage_node_weight,
                            double damping, double tol, int32_t max_iter, double* out_doc_scores, int32_t* iters);
/* The same calls with the ranking done on the device: every passage row by descending PageRank score — the reference's
 * `sorted_doc_ids = np.argsort(doc_scores)[::-1]` and `sorted_doc_scores = doc_scores[sorted_doc_ids.tolist()]` (ComoRAG.py:1101-1105),
 * which must cover every passage (`len(sorted_doc_ids) == len(passage_node_idxs)`).  A segmented stable radix sort of the fp64 scores
 *  runs behind the power iteration on the call's stream; the [nb, n_rows] doubles never reach the host unsorted.
 *   out_ids    [nb, n_out] int64 passage ROWS — positions in the unranked call's out_doc_scores, what np.argsort(doc_scores) indexes;
 *              neither cmr_index_set_id_base nor the id block table is applied.
 *   out_scores [nb, n_out] double, out_scores[b, r] = doc_scores[b, out_ids[b, r]] bit for bit (gathered, not recomputed).
 *   1 <= n_out <= n_rows; n_out = n_rows is the reference's full ranking, a smaller n_out shortens only the last kernel and the copy.
 * Order: score descending (-0.0 = +0.0; a NaN, which the iteration cannot produce, last), equal scores by ascending row — where numpy's
 * argsort leaves the order of equal scores unspecified.  Row b of a batch equals the single call bit for bit.
 *   cmr_index_ppr_ranked        cmr_index_ppr + ranking (ComoRAG.py:1034-1044, :1086-1105 with :1101-1105 on the device); combined like
 *                               cmr_index_ppr where the index's "combine" option is set (same n_out as well).
 *   cmr_index_ppr_ranked_batch  cmr_index_ppr_batch + ranking (:1101-1105 for each of the nb queries, one set of launches).
 *   cmr_graph_ppr_ranked_batch  cmr_graph_ppr_batch, then pagerank[vertex of row] ranked (:1101-1105): needs cmr_graph_set_passage_vertices;
 *                               nb = 1 is the single call.
 * Arguments are checked before any device call: NULL, n_out out of range, no passage map -> CMR_ERR_INVALID; nb > CMR_PPR_MAX_BATCH or
 * n_rows >= 2^32 -> CMR_ERR_UNSUPPORTED.                                                                                              
 * CMR_PPR_RANK_TILE: keys per workgroup of the sort (sizes around it are where its paths change).                                    */
#define CMR_PPR_RANK_TILE 2048
int32_t cmr_index_ppr_ranked(cmr_index_t* idx, cmr_graph_t* g, const float* q_f32, const int32_t* seed_vertices,
                             const double* seed_weights, int32_t n_seeds, double passage_node_weight, double damping, double tol,
                             int32_t max_iter, int64_t n_out, int64_t* out_ids, double* out_scores, int32_t* iters);
int32_t cmr_index_ppr_ranked_batch(cmr_index_t* idx, cmr_graph_t* g, const float* q_f32, int32_t nb, const int32_t* seed_offsets,
                                   const int32_t* seed_vertices, const double* seed_weights, double passage_node_weight,
                                   double damping, double tol, int32_t max_iter, int64_t n_out, int64_t* out_ids,
                                   double* out_scores, int32_t* iters);
int32_t cmr_graph_ppr_ranked_batch(cmr_graph_t* g, const double* reset, int32_t nb, double damping, double tol, int32_t max_iter,
                                   int64_t n_out, int64_t* out_ids, double* out_scores, int32_t* iters);

/* ---- row-shard exchange ------------------------------------------------------------------
 * One process per GPU, each with a row shard (cmr_index_set_id_base makes its searches return global ids).  Per query
 * batch every rank packs its [nq, k] candidates into ONE u64 each — the order-preserving score code in the high word,
 * ~(global row) in the low word, so unsigned order == the exported order; global rows must be < 2^32 - 1 — all-gathers
 * them with a single collective (nq*k*8 bytes per rank; latency-bound over xGMI) and merges world*k keys per query.
 * The result equals a single-shard search by construction.  (No reference counterpart)
 *
 * cmr_pack_candidates_dev / cmr_merge_keys_dev are the two kernels on their own, for hosts that bring their own
 * collective (comorag_amd/sharded.py runs torch.distributed's all_gather_into_tensor between them).
 * cmr_comm_* wrap RCCL itself (bound with dlopen at first use — the RCCL already in the process when there is one):
 * rank 0 calls cmr_comm_unique_id and ships the 128 bytes to the other ranks by any channel, every rank calls
 * cmr_comm_create (collective), then cmr_comm_allgather_merge per batch on a stream of its choice — the index
 * pipeline's post stream (cmr_index_pipeline_stream(idx, 2)) orders it after the batch's outputs.                     */
#define CMR_COMM_ID_BYTES 128
typedef struct cmr_comm cmr_comm_t;
int32_t cmr_pack_candidates_dev(const int64_t* ids_dev, const float* scores_dev, int64_t n, uint64_t* keys_dev, void* stream);
int32_t cmr_merge_keys_dev(const uint64_t* keys_dev /*[n_shards][nq][k]*/, int32_t n_shards, int32_t nq, int32_t k,
                           int64_t* out_ids_dev, float* out_scores_dev, void* stream);
int32_t cmr_comm_unique_id(uint8_t* out_id128);
int32_t cmr_comm_create(int32_t world, int32_t rank, const uint8_t* id128, int32_t device_id, cmr_comm_t** out);
int32_t cmr_comm_destroy(cmr_comm_t* comm);
/* what the communicator was created with, and the rank count RCCL itself reports (ncclCommCount; 0 if unavailable) —
 * bench.py prints it so a multi-GPU line shows that the collective really spanned N ranks                              */
int32_t cmr_comm_info(cmr_comm_t* comm, int32_t* world, int32_t* rank, int32_t* rccl_ranks);
int32_t cmr_comm_allgather_merge(cmr_comm_t* comm, const int64_t* ids_dev, const float* scores_dev, int32_t nq, int32_t k,
                                 int64_t* out_ids_dev, float* out_scores_dev, void* stream);

/* ---- one process, several devices --------------------------------------------------------------
 * ComoRAG runs ONE process whose 16-thread pool (ComoRAG.try_answer, ComoRAG.py:432-453) calls tri_retrieve (:456-554) at
 * LLM-dependent times; a row-sharded index it can sit on must therefore be driven from one process.  cmr_mindex_t owns
 * n_shards cmr_index_t row shards, shard s on device device_ids[s] (a device may appear several times: logical shards — how a
 * 1-GPU box rehearses the layout).  Same conventions as cmr_index_t: thread-safe (searches concurrent, append exclusive), host
 * buffers in / out, exported tie rule, global row ids dense in append order (embedding_store.py:122-128,
 * utils/memory_utils.py:294-300) — results are identical to ONE cmr_index_t holding the same rows.
 *   append      rows go to the shards in blocks: a block opens on the currently shortest shard and holds
 *               max(append_block_rows, ceil(n / n_shards)) rows — a bulk append lands as contiguous row blocks, a memory pool's
 *               25-row appends fill blocks of append_block_rows (default 65536: a corpus of a few thousand rows lives on ONE shard
 *               and is searched without multi-shard overhead) that go round the shards; each shard translates
 *               its rows through its block table (cmr_index_set_id_blocks).  All or nothing: a chunk that fails (NaN/Inf rows,
 *               out of memory) rolls the shards that already took theirs back.
 *   search      begins on every non-empty shard before it finishes on any (from three shards on the per-shard enqueues are
 *               issued by per-shard worker threads); every shard's merge kernel writes its [nq, k] candidates straight into
 *               pinned, device-mapped HOST memory (nq * k * 12 bytes per shard over PCIe: no peer access, no collective), the
 *               host does the final merge of the sorted lists — north_star's "host-side final merge"; min / max combine.
 *   scores / sorted_scores / rescore / get_rows   as on cmr_index_t, over global ids.
 *   search_pipelined + collect   throughput mode: q_dev[s] = the batch's queries on shard s's device (entries of empty shards are
 *               ignored); returns at once with a ticket, up to four tickets may be uncollected; collect waits for the shards,
 *               merges on the host and frees the ticket.  k <= CMR_MAX_K.
 *   set_option  "append_block_rows", "parallel_min_shards" (default 3), "force_peer_staging" (1: append_dev stages every chunk through
 *               hipMemcpyPeer even when source and shard share a device — how a one-GPU box executes the cross-device append path);
 *               anything else goes to every shard (cmr_index_set_option) with NO search in flight (exclusive over the handle).
 *   shard       borrow shard s (profiling, reading options, tests).  Do NOT append to it or re-base it directly, and set route
 *               selectors through cmr_mindex_set_option, not on the borrowed handle, while other threads search.
 * cmr_mindex_plan_append is the routing rule on its own (pure host arithmetic, no device): chunks (shard, rows) for m appended
 * rows given the shards' sizes and the open block (cur_shard, cur_room); n_chunks always returns the chunk count.            */
typedef struct cmr_mindex cmr_mindex_t;
int32_t cmr_mindex_create(int32_t n_shards, const int32_t* device_ids, int32_t dim, int32_t dtype, int64_t capacity_hint,
                          uint32_t flags, cmr_mindex_t** out);
int32_t cmr_mindex_destroy(cmr_mindex_t* m);
int32_t cmr_mindex_size(cmr_mindex_t* m, int64_t* n_rows);
int32_t cmr_mindex_info(cmr_mindex_t* m, int32_t* n_shards, int32_t* device_ids /*[n_shards] or NULL*/,
                        int64_t* shard_rows /*[n_shards] or NULL*/, int64_t* device_bytes);
int32_t cmr_mindex_shard(cmr_mindex_t* m, int32_t s, cmr_index_t** out);
int32_t cmr_mindex_set_option(cmr_mindex_t* m, const char* name, int64_t value);
int32_t cmr_mindex_append(cmr_mindex_t* m, const float* rows_f32, int64_t n);
/* rows on device src_device (e.g. an encoder's output tensor; `stream` = the stream that produced them): chunks of shards on
 * that device are appended in place, the others go device to device (hipMemcpyPeer) first.  Returns when the rows are in.  */
int32_t cmr_mindex_append_dev(cmr_mindex_t* m, const float* rows_f32_dev, int64_t n, int32_t src_device, void* stream);
int32_t cmr_mindex_search(cmr_mindex_t* m, const float* q_f32, int32_t nq, int32_t k, int64_t* out_ids, float* out_scores,
                          float* out_min, float* out_max);
int32_t cmr_mindex_search_ids(cmr_mindex_t* m, const float* q_f32, int32_t nq, int32_t k, int32_t mode, const int64_t* id_offsets,
                              const int64_t* ids /* GLOBAL row ids */, int64_t n_ids, int64_t* out_ids, float* out_scores, float* out_min,
                              float* out_max);
int32_t cmr_mindex_search_min_score(cmr_mindex_t* m, const float* q_f32, int32_t nq, int32_t k, float min_score,
                                    int64_t* out_ids, float* out_scores);
int32_t cmr_mindex_scores(cmr_mindex_t* m, const float* q_f32, int32_t nq, float* out, int64_t ld);
int32_t cmr_mindex_sorted_scores(cmr_mindex_t* m, const float* q_f32, int32_t nq, int64_t* out_ids, float* out_scores,
                                 float* out_min, float* out_max);
/* Range search over the shards (cmr_index_range_search above has the semantics): GLOBAL ids; the result equals ONE cmr_index_t holding the
 * same rows, bit for bit.  Every non-empty shard runs its own range search — all of them at once, on the shards' worker threads — and the
 * host merges per query with cmr_range_merge (a shard's list is in the exported order already: local row order is global id order inside
 * a shard).  max_total applies to the merged total: where the batch could exceed it, every shard's count runs before any shard's
 * compaction.                                                                                                                          */
int32_t cmr_mindex_range_count(cmr_mindex_t* m, const float* q_f32, int32_t nq, float min_score, int64_t* out_counts /*[nq]*/);
int32_t cmr_mindex_range_search(cmr_mindex_t* m, const float* q_f32, int32_t nq, float min_score, int64_t max_total,
                                cmr_range_result_t** out);
/* The filtered score-bound searches from GLOBAL row ids ("filtered score-bound searches" above has the semantics): the
 * result of ONE cmr_index_t holding the same rows, bit for bit.                                                                        */
int32_t cmr_mindex_search_min_score_ids(cmr_mindex_t* m, const float* q_f32, int32_t nq, int32_t k, float min_score, int32_t mode,
                                        const int64_t* id_offsets, const int64_t* ids /* GLOBAL row ids */, int64_t n_ids, int64_t* out_ids,
                                        float* out_scores);
int32_t cmr_mindex_range_count_ids(cmr_mindex_t* m, const float* q_f32, int32_t nq, float min_score, int32_t mode, const int64_t* id_offsets,
                                   const int64_t* ids /* GLOBAL row ids */, int64_t n_ids, int64_t* out_counts /*[nq]*/);
int32_t cmr_mindex_range_search_ids(cmr_mindex_t* m, const float* q_f32, int32_t nq, float min_score, int64_t max_total, int32_t mode,
                                    const int64_t* id_offsets, const int64_t* ids /* GLOBAL row ids */, int64_t n_ids,
                                    cmr_range_result_t** out);
int32_t cmr_mindex_rescore(cmr_mindex_t* m, const float* q_f32, int32_t nq, const int64_t* cand, int32_t n_cand, int32_t k,
                           int64_t* out_ids, float* out_scores);
int32_t cmr_mindex_get_rows(cmr_mindex_t* m, const int64_t* ids, int64_t n, float* out);
/* Diversified top-k over the shards (see cmr_index_search_mmr): global ids; bit for bit what one index holding the same rows returns. */
int32_t cmr_mindex_pair_scores(cmr_mindex_t* m, const int64_t* ids, int32_t nq, int32_t F, float* out);
int32_t cmr_mindex_mmr_select(cmr_mindex_t* m, const int64_t* cand_ids, const float* cand_scores, int32_t nq, int32_t F, int32_t k,
                              double lam, int64_t* out_ids, float* out_scores);
int32_t cmr_mindex_search_mmr(cmr_mindex_t* m, const float* q_f32, int32_t nq, int32_t k, int32_t fetch_k, double lam, int64_t* out_ids,
                              float* out_scores);
/* Exact fp32 top-k over every shard (ComoRAG.py:958-966): each shard certifies its local top-k (cmr_index_search_exact: exact when
 * no row outside its candidates can beat its k-th by more than 2 E_q), the host merges the fp32 lists with the exported tie rule,
 * out_exact = AND over the shards.                                                                                             */
int32_t cmr_mindex_search_exact(cmr_mindex_t* m, const float* q_f32, int32_t nq, int32_t k, int64_t* out_ids, float* out_scores,
                                int32_t* out_exact);
int32_t cmr_mindex_search_pipelined(cmr_mindex_t* m, const float* const* q_dev /*[n_shards]*/, int32_t nq, int32_t k, void** ticket);
int32_t cmr_mindex_collect(cmr_mindex_t* m, void* ticket, int64_t* out_ids, float* out_scores, float* out_min, float* out_max);
/* host-side cost of the throughput mode since the last reset: collected batches, mean microseconds a shard's enqueue job took
 * on its worker thread, mean microseconds collect waited for the shards' events, mean microseconds of the host merge          */
int32_t cmr_mindex_profile(cmr_mindex_t* m, int32_t reset, int64_t* n_batches, double* enqueue_us_per_shard, double* wait_us_per_batch,
                           double* merge_us_per_batch);
int32_t cmr_mindex_plan_append(const int64_t* shard_rows, int32_t n_shards, int32_t cur_shard, int64_t cur_room, int64_t m,
                               int64_t block_rows, int32_t max_chunks, int32_t* out_shard, int64_t* out_count, int32_t* n_chunks,
                               int32_t* new_cur, int64_t* new_room);
/* Row removal over the shards (cmr_index_remove_ids above has the semantics): GLOBAL ids in, global ids dense again in the old global
 * order afterwards — results equal ONE cmr_index_t that removed the same ids.  The new block tables are planned on the host first
 * (cmr_mindex_plan_remove), then every shard that loses rows compacts its own, all shards at once, then the tables, the shards' row
 * counts and the total are replaced; later appends keep global ids dense in append order (the open block stays open: an append continues
 * a shard's last run only while that run ends at the last global id).  Exclusive over the handle; uncollected tickets of
 * cmr_mindex_search_pipelined issued before stay collectable with the ids of before.
 * The only fallible step is a shard's compaction.  If one fails, the call returns its error, *n_removed = the rows that did go, and the
 * index is left CONSISTENT as if only the ids held by the shards that succeeded had been listed: those rows are gone, global ids are
 * dense, the failed shard's listed rows are all still there (out of memory: it is untouched) — the caller may call again with the same
 * list.  (After a HIP error inside a shard's copy launches that shard's rows are unspecified, as in cmr_index_remove_ids.)  One case is NOT
 * consistent: a shard that reports success but another number of removed rows than the host planned — CMR_ERR_HIP, the tables are left as
 * they were and no longer describe the shards; destroy the index.
 * cmr_mindex_plan_remove is the table arithmetic on its own (pure host, no device): the shards' tables — n_blocks[s] blocks each,
 * concatenated in shard order in local_start / global_start, block b of a shard holding local rows [local_start[b], next local start or
 * shard_rows[s]) = global ids global_start[b] + ... — and the ids to remove give the new row counts and tables (same layout; never more
 * blocks than came in; any output may be NULL).  skip_shards (NULL: none): ids held by a shard with a non-zero entry are ignored, as
 * if they had not been listed — the tables cmr_mindex_remove_ids installs when those shards' compaction failed.  A block's new global start is its old one minus the removed ids below it, its length
 * shrinks by the removed ids inside it, empty blocks are dropped, local starts are the running sum.                                  */
int32_t cmr_mindex_remove_ids(cmr_mindex_t* m, const int64_t* ids /* GLOBAL row ids */, int64_t n_ids, int64_t* n_removed /* may be NULL */);
int32_t cmr_mindex_plan_remove(int32_t n_shards, const int64_t* shard_rows, const int32_t* n_blocks /*[n_shards]*/, const int64_t* local_start,
                               const int64_t* global_start, const int64_t* ids, int64_t n_ids, const int32_t* skip_shards /*[n_shards] or NULL*/,
                               int64_t* new_shard_rows /*[n_shards]*/, int32_t* new_n_blocks /*[n_shards]*/, int64_t* new_local_start,
                               int64_t* new_global_start, int64_t* n_removed);
/* Row update over the shards (cmr_index_update_rows above has the semantics): GLOBAL ids in; results equal ONE cmr_index_t that took
 * the same update.  Planned once on the host, then the CHECK phase runs on every shard that has entries (on the shards' worker threads)
 * — if any check fails the error is returned with nothing written anywhere — then the WRITE phase on every such shard.  A HIP error in
 * the write phase is returned as it is; every row is then wholly old or wholly new.  Exclusive over the handle.
 * cmr_mindex_plan_update is the planning on its own (pure host, no device), tables as in cmr_mindex_plan_remove: ignored ids dropped,
 * the last occurrence of an id kept, the entries grouped by shard and, inside a shard, by ascending local row — entry j replaces
 * local row out_local[j] of shard out_shard[j] by input row out_src[j].  Each output holds n_ids entries, the first *n_updated valid;
 * out_count[s] (may be NULL) = entries of shard s.  One cmr_index_t is the one-shard case: its id base or block table is shard 0's.  */
int32_t cmr_mindex_update_rows(cmr_mindex_t* m, const int64_t* ids /* GLOBAL row ids */, const float* rows_f32, int64_t n, int64_t* n_updated /* may be NULL */);
int32_t cmr_mindex_plan_update(int32_t n_shards, const int64_t* shard_rows, const int32_t* n_blocks /*[n_shards]*/, const int64_t* local_start,
                               const int64_t* global_start, const int64_t* ids, int64_t n_ids, int32_t* out_shard, int64_t* out_local,
                               int64_t* out_src /* each [n_ids] */, int64_t* out_count /*[n_shards] or NULL*/, int64_t* n_updated);

/* ---- encoder tail -----------------------------------------------------------------------
 * Fused masked mean-pool + L2-normalise of the encoder's last hidden state; replaces
 * mean_pooling (embedding_model/BGEEmbedding.py:15-28) + F.normalize (:126-127, eps 1e-12).
 *   hidden_dev [b, l, d] of hidden_dtype (cmr_dtype), mask_dev [b, l] int64 (HF attention_mask),
 *   out_dev [b, d] fp32.  normalize = 0 gives the plain masked mean.                           */
int32_t cmr_pool_l2norm(int32_t device_id, const void* hidden_dev, int32_t hidden_dtype,
                        const int64_t* mask_dev, int32_t b, int32_t l, int32_t d, int32_t normalize,
                        float* out_dev, void* stream);

/* ---- encoder layer pieces -----------------------------------------------------------------
 * The two non-GEMM stages of a BERT layer inside `self.embedding_model(**inputs)` (embedding_model/BGEEmbedding.py:119; the
 * GEMMs stay PyTorch-ROCm / hipBLASLt as north_star prescribes).  They take device pointers of bf16, fp16 or fp32 tensors (dtype =
 * CMR_BF16, CMR_F16 or CMR_F32: every tensor of a call has that type) and run on `stream`.  CMR_F32 is fp32 end to end (fp32 in, exact
 * f32-input MFMA products, fp32 out, nothing rounded to 16 bits); its buffers must be 16-byte aligned in every entry point.
 *
 * cmr_encoder_attention: out[b*l, hidden] = softmax(Q K^T / sqrt(head_dim), keys >= lens[s] masked) V per sequence and head,
 *   with Q | K | V the three hidden-wide column groups of ONE packed projection qkv_dev[b*l, 3*hidden] (hidden = n_heads *
 *   head_dim, head h = columns h*head_dim.. of its group); lens_dev[b] int32 = real tokens of each right-padded sequence
 *   (transformers' BertSelfAttention + its additive mask).  head_dim must be 64 or 32 (BERT-base / -large heads; the 384-hidden
 *   small tier: bge-small, e5-small, MiniLM), any other width is CMR_ERR_INVALID.  Rows >= lens[s] of out are unspecified
 *   finite values (zeros where a whole 128-row block is padding): the pooling mask drops them.
 * cmr_encoder_embed_layernorm: out[t] = LayerNorm(word[ids[t]] + position[t mod l] + token_type[tt[t]]) for the rows = b*l tokens
 *   of a [b, l] mini-batch (transformers' BertEmbeddings with default position ids; token_type_dev NULL = type 0; ids outside a
 *   table are clamped into it).  position_offset: 0 for BERT; padding_idx + 1 for the RoBERTa family (XLM-R = bge-m3), whose
 *   position table starts there (RobertaEmbeddings.create_position_ids_from_input_ids on right-padded rows: token t of a sequence
 *   sits at position t + padding_idx + 1; the padded tail's embeddings are never used).
 * cmr_encoder_add_layernorm: out = LayerNorm(y + bias + residual) * gamma + beta over rows of d elements, fp32 statistics
 *   (BertSelfOutput / BertOutput after their dense GEMM); bias_dev / residual_dev may be NULL.                              */
/* The LAST layer's cmr_encoder_add_layernorm with the encoder tail folded in — mean_pooling over the tokens < lens[s]
 * (embedding_model/BGEEmbedding.py:15-28) and F.normalize (:126-127, eps 1e-12; normalize = 0: the plain masked mean) of the
 * [b, l, d] mini-batch it would have written: out_dev [b, d] fp32; the hidden state itself is never stored (a 16-token block per
 * workgroup -> one fp32 partial row, summed in block order by a small second launch; a 16-bit dtype's values are rounded to 16 bits before
 * they are added, as the stored hidden state would have been; CMR_F32 adds them as they are).  l % 16 == 0, d % 8 == 0, d <= 2048, 16-byte aligned buffers, right-padded
 * sequences (lens_dev [b] int32): CMR_ERR_UNSUPPORTED otherwise — callers then run add_layernorm + cmr_pool_l2norm.             */
int32_t cmr_encoder_add_layernorm_pool(int32_t device_id, const void* y_dev, const void* bias_dev, const void* residual_dev,
                                       const void* gamma_dev, const void* beta_dev, float eps, int32_t b, int32_t l, int32_t d,
                                       int32_t dtype, const int32_t* lens_dev, int32_t normalize, float* partial_dev /* scratch:
                                       b * (l / 16) * d floats, caller-owned so that a stream capture allocates nothing */,
                                       float* out_dev, void* stream);
int32_t cmr_encoder_embed_layernorm(int32_t device_id, const int64_t* ids_dev, const int64_t* token_type_dev,
                                    const void* word_dev, const void* pos_dev, const void* type_dev,
                                    const void* gamma_dev, const void* beta_dev, float eps, int64_t rows, int32_t l,
                                    int32_t d, int32_t vocab, int32_t n_positions, int32_t n_types, int32_t position_offset,
                                    int32_t dtype, void* out_dev, void* stream);
/* cmr_encoder_embed_layernorm from RAGGED token ids: ids32_dev holds the b sequences' tokens back to back (int32), offsets_dev[b + 1]
 * their starts; row (s, t) of the [b, l] mini-batch embeds token t of sequence s (token 0 behind its end: padding rows, masked
 * downstream), token type 0.  What the host ships per mini-batch is then ONE int32 array lens | offsets | ids — no padded id, mask
 * or token-type tensors (the tokenizer call of embedding_model/BGEEmbedding.py:112-118 pads on the host and uploads three).     */
int32_t cmr_encoder_embed_layernorm_ragged(int32_t device_id, const int32_t* ids32_dev, const int32_t* offsets_dev, const void* word_dev,
                                           const void* pos_dev, const void* type_dev, const void* gamma_dev, const void* beta_dev, float eps,
                                           int32_t b, int32_t l, int32_t d, int32_t vocab, int32_t n_positions, int32_t position_offset,
                                           int32_t dtype, void* out_dev, void* stream);
int32_t cmr_encoder_attention(int32_t device_id, const void* qkv_dev, int32_t dtype, const int32_t* lens_dev,
                              int32_t b, int32_t l, int32_t n_heads, int32_t head_dim, void* out_dev, void* stream);
int32_t cmr_encoder_add_layernorm(int32_t device_id, const void* y_dev, const void* bias_dev,
                                  const void* residual_dev, const void* gamma_dev, const void* beta_dev,
                                  float eps, int64_t rows, int32_t d, int32_t dtype, void* out_dev, void* stream);

/* ---- encoder: the linear layers of ONE SHORT QUERY (1 .. 128 token rows) -----------------------------------------------------
 * The four nn.Linear of the model's BertLayer inside `self.embedding_model(**inputs)` (embedding_model/BGEEmbedding.py:119) for a
 * mini-batch of m = b*l <= 128 token rows, where a library GEMM is all launch and latency: weight-streaming kernels over nn.Linear's
 * own row-major weight w_dev [n, k] (no packed copy), fp32 accumulation.  dtype = CMR_BF16 or CMR_F16 (every 16-bit tensor of a call has
 * that type); n % 16 == 0, k % 32 == 0, 16-byte aligned buffers.  Checked before any device call: NULL pointers, m / n / k <= 0 and an
 * unknown dtype are CMR_ERR_INVALID; m > 128, other n / k, CMR_F32 and misaligned buffers are CMR_ERR_UNSUPPORTED.  A token row's result
 * does not depend on m or on the other rows (the split and the order of every sum are functions of n and k).
 *
 * cmr_encoder_linear_small: out16_dev [m, n] = x_dev [m, k] w^T + bias (bias_dev [n] or NULL) summed in fp32 and rounded to the 16-bit
 *   type — BertSelfAttention's packed query | key | value projection (act = 0) — and, with act = 1, the model's exact erf GELU of that
 *   ROUNDED value, rounded again: BertIntermediate, F.gelu(F.linear(x, w, b)) in one launch.
 * cmr_encoder_linear_small_partials: the same product with K split over n_split workgroup slices (BertSelfOutput.dense, BertOutput.dense:
 *   k = hidden or intermediate): partials_dev [n_split, m, n] fp32, slice s of the sum in slab s, no bias, nothing rounded.  The slabs
 *   are combined by the NEXT launch, cmr_encoder_add_layernorm_partials — no workgroup waits on another one.
 * cmr_encoder_linear_small_split: n_split and the bytes of the slabs for (m, n, k, dtype), so that the caller can allocate.
 * cmr_encoder_add_layernorm_partials: out = LayerNorm(sum_s partials[s] + bias + residual) * gamma + beta over rows of d elements (the
 *   slabs added in slab order in fp32, then cmr_encoder_add_layernorm's body: BertSelfOutput / BertOutput after their dense GEMM);
 *   bias_dev / residual_dev may be NULL; d % 4 == 0, d <= 2048, slabs 16-byte and 16-bit buffers 8-byte aligned.
 * cmr_encoder_add_layernorm_partials_pool: the LAST layer's cmr_encoder_add_layernorm_partials with the encoder tail folded in — what
 *   cmr_encoder_add_layernorm_pool is to cmr_encoder_add_layernorm (mean_pooling, embedding_model/BGEEmbedding.py:15-28, and F.normalize,
 *   :126-127): the same kernel with the slabs as its input; out_dev [b, d] fp32, pool_partial_dev b * (l / 16) * d floats of scratch;
 *   l % 16 == 0, d % 8 == 0, d <= 2048, 16-byte aligned buffers, CMR_ERR_UNSUPPORTED otherwise.                                    */
int32_t cmr_encoder_linear_small(int32_t device_id, const void* x_dev, const void* w_dev, const void* bias_dev, int32_t m, int32_t n,
                                 int32_t k, int32_t dtype, int32_t act, void* out16_dev, void* stream);
int32_t cmr_encoder_linear_small_partials(int32_t device_id, const void* x_dev, const void* w_dev, int32_t m, int32_t n, int32_t k,
                                          int32_t dtype, float* partials_dev, void* stream);
int32_t cmr_encoder_linear_small_split(int32_t m, int32_t n, int32_t k, int32_t dtype, int32_t* n_split, int64_t* slab_bytes);
int32_t cmr_encoder_add_layernorm_partials(int32_t device_id, const float* partials_dev, int32_t n_split, const void* bias_dev,
                                           const void* residual_dev, const void* gamma_dev, const void* beta_dev, float eps,
                                           int64_t rows, int32_t d, int32_t dtype, void* out_dev, void* stream);
int32_t cmr_encoder_add_layernorm_partials_pool(int32_t device_id, const float* partials_dev, int32_t n_split, const void* bias_dev,
                                                const void* residual_dev, const void* gamma_dev, const void* beta_dev, float eps,
                                                int32_t b, int32_t l, int32_t d, int32_t dtype, const int32_t* lens_dev, int32_t normalize,
                                                float* pool_partial_dev, float* out_dev, void* stream);

/* ---- encoder: the same linear layers over MANY token rows (several short queries in one forward) ------------------------------
 * cmr_encoder_linear_rows / cmr_encoder_linear_rows_partials are cmr_encoder_linear_small / _partials for 1 <= m <= CMR_ENCODER_ROWS_MAX
 * token rows: the concatenated rows of up to 16 one-question forwards (embedding_combine).  Operands, alignment, act and
 * dtype rules, the checks and their order are those of the block above; only the row limit differs (m > CMR_ENCODER_ROWS_MAX is
 * CMR_ERR_UNSUPPORTED).  The partials form writes partials_dev [n_split, m, n] with the n_split cmr_encoder_linear_small_split reports
 * for (n, k, dtype) (ask it with any m <= 128: n_split does not depend on m; the slabs take n_split * m * n floats); the unchanged
 * cmr_encoder_add_layernorm_partials(_pool) consume them.
 * CONTRACT: for every row r the output bits are those cmr_encoder_linear_small(_partials) produces for that row in ANY call that contains
 * it — independent of m, of the row's position and of the other rows.  (The kernel is the same weight stream: m > 128 runs row tiles of
 * 128 over the grid's third dimension, each tile the sums of the one-query kernel in the same order; later tiles re-read the weights,
 * which no packed copy is made of.)                                                                                                    */
#define CMR_ENCODER_ROWS_MAX 2048   /* 16 questions x 128 token rows */
int32_t cmr_encoder_linear_rows(int32_t device_id, const void* x_dev, const void* w_dev, const void* bias_dev, int32_t m, int32_t n,
                                int32_t k, int32_t dtype, int32_t act, void* out16_dev, void* stream);
int32_t cmr_encoder_linear_rows_partials(int32_t device_id, const void* x_dev, const void* w_dev, int32_t m, int32_t n, int32_t k,
                                         int32_t dtype, float* partials_dev, void* stream);

/* ---- encoder: the tail of a CROSS-ENCODER (bge-reranker-*: an XLM-R / BERT encoder with a one-logit classification head) ------
 * Only token 0 of every sequence feeds the head, so the last layer needs every stage behind its K / V projection for b rows, not b*l.
 *
 * out[s, h*head_dim ..] = softmax(q K^T / sqrt(head_dim), keys >= lens[s] masked) V for the ONE query row q = token 0 of
 * sequence s, per head; qkv_dev is the packed projection [b*l, 3*hidden] of cmr_encoder_attention (same column groups),
 * lens_dev[b] int32 >= 1, out_dev [b, hidden] of `dtype` (CMR_BF16 / CMR_F16: fp32 arithmetic, rounded once on the store;
 * CMR_F32: nothing rounded).  head_dim 64 or 32.  Rows >= lens[s] of qkv are never read.  A sequence's result does not depend on the
 * other sequences or heads of the call.  NULL, b / l / n_heads <= 0, another head_dim or dtype and buffers that are not 16-byte aligned are
 * CMR_ERR_INVALID, checked before any device call (as cmr_encoder_attention).                                                    */
int32_t cmr_encoder_attention_cls(int32_t device_id, const void* qkv_dev, int32_t dtype, const int32_t* lens_dev,
                                  int32_t b, int32_t l, int32_t n_heads, int32_t head_dim, void* out_dev, void* stream);
/* out[s] = b2 + sum_j w2[j] * tanh(b1[j] + sum_i w1[j, i] * x[s*x_stride + i]),  s < b:  RobertaClassificationHead
 * (dense -> tanh -> out_proj, one label) and BertPooler + classifier are this same map.  w1 [d, d] row-major (nn.Linear's own
 * tensor), b1 [d] or NULL, w2 [d], b2 [1] or NULL, x rows x_stride elements apart (x_stride >= d: the CLS rows of a
 * [b*l, d] hidden state are read in place with x_stride = l*d).  All of `dtype`; fp32 arithmetic, tanhf, out_dev [b] fp32.
 * d % 8 == 0, d <= 2048, 16-byte aligned rows: CMR_ERR_UNSUPPORTED otherwise.  NULL x / w1 / w2 / out, b or d <= 0, x_stride < d and an
 * unknown dtype are CMR_ERR_INVALID; all of it is checked before any device call.  No atomics: partial sums meet in a fixed order, and a
 * row's bits do not depend on b or on the other rows.                                                                             */
int32_t cmr_encoder_cls_head(int32_t device_id, const void* x_dev, int64_t x_stride, const void* w1_dev, const void* b1_dev,
                             const void* w2_dev, const void* b2_dev, int32_t b, int32_t d, int32_t dtype, float* out_dev, void* stream);

/* ---- measurement ------------------------------------------------------------------------
 * HIP-event timing of the dominant kernel (the corpus scan) on the stream it is launched on.
 * enable → run searches → collect returns launches, summed kernel ms and the algorithmic bytes
 * one launch reads (N_pad*Dpad*sizeof(elem) + query/result bytes), then resets.
 * on = 1: every main scan is timed; on = N > 1: every N-th one (the two event packets around a
 * scan cost ~25 us on the scan stream, 9 % of a 1 M-row step: sampling keeps the measurement from
 * slowing what it measures); on = 0: off.                                                      */
int32_t cmr_profile_enable(cmr_index_t* idx, int32_t on);
int32_t cmr_profile_collect(cmr_index_t* idx, int64_t* n_launches, double* total_ms,
                            double* bytes_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* COMORAG_HIP_H */
