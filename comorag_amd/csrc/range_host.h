// Range search and count, among every row or among the rows a RowFilter keeps (the filter's checks and its view in
// the workspace: row_filter.h), the merge of shard results and the result handle.  Included by api.hip only, behind row_filter.h.
#pragma once

// ---- range search: every row at or above a score bound, per query.  Per block of queries: scores_enqueue, count + offsets
// (range_kernels.hip), ONE small round trip for the per-query counts, then per group of consecutive queries compaction, the stable sort of
// (query | complemented score code, row) pairs and the gather of ids and score bits — all on the workspace's one stream.
static int range_block_queries(const cmr_index* idx, int nq, long long ld) {
    long long b = std::max<long long>(1, std::min<long long>(nq, (1ll << 31) / std::max<long long>(ld * 4, 1)));      // <= 2 GiB of scores
    if (idx->range_block_queries > 0) b = std::min<long long>(b, idx->range_block_queries);
    return (int)b;
}
// the arguments of a range search or count that need neither an index nor a device.  The filtered forms: every check
// that needs no index comes first, the handle last (as cmr_index_search_ids).
int cmr_range_args_check(const void* idx, const void* q, const void* out, int nq, float min_score, const RowFilter& f) {
    if (f.kind == RowFilter::none) {
        if (!idx || !q || !out) return fail(CMR_ERR_INVALID, "NULL argument");
        if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
        return cmr_min_score_check(min_score);
    }
    if (!q || !out) return fail(CMR_ERR_INVALID, "NULL argument");
    int rc = cmr_filter_args_check(f, nq, 1);
    if (rc) return rc;
    if ((rc = cmr_min_score_check(min_score))) return rc;
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    return CMR_OK;
}
static int range_rows_check(const cmr_index* idx) {
    return idx->n < (1ll << 32) ? CMR_OK : fail(CMR_ERR_UNSUPPORTED, "range search needs fewer than 2^32 rows, the index holds %lld", idx->n);
}
// scores of nb queries into ws->d_out [nb][ld], the (query, tile) offsets into ws->r_cnt, the per-query counts to counts_dev [nb]
// mk: only the allowed rows count (the words of per-query lists are built here, behind the scores and in front of the count); the block's first query
// is query q0 of the call
static int range_count_enqueue(cmr_index* idx, Workspace* ws, const float* q_dev, int nb, long long ld, unsigned lo, long long* counts_dev,
                               const FilterView* mk = nullptr, int q0 = 0) {
    HIP_TRY(ws->d_out.ensure((size_t)nb * ld * 4));
    HIP_TRY(ws->r_cnt.ensure(cmr_range_counter_bytes(idx->n, nb)));
    int rc = scores_enqueue(idx, ws, q_dev, nb, (float*)ws->d_out.p, ld);
    if (rc) return rc;
    idx->last_route.store(route_code(CMR_ROUTE_RANGE) | (mk ? mk->route : 0), std::memory_order_relaxed);
    if (mk && (rc = filter_words_enqueue(idx, ws, *mk, q0, nb))) return rc;
    const CmrRangeMask km = mk ? mk->kernel(q0) : CmrRangeMask{};
    HIP_TRY(cmr_launch_range_count((const float*)ws->d_out.p, ld, idx->n, nb, lo, (unsigned*)ws->r_cnt.p, counts_dev, ws->stream, mk ? &km : nullptr));
    return CMR_OK;
}
// the counts of a block on the host (the block's round trip), with the non-finite flag of its queries
static int range_counts_to_host(Workspace* ws, int nb, int64_t* counts) {
    int flagged = 0;
    HIP_TRY(hipMemcpyAsync(counts, ws->r_counts.p, (size_t)nb * 8, hipMemcpyDeviceToHost, ws->stream));
    HIP_TRY(hipMemcpyAsync(&flagged, ws->flag_ptr, sizeof(int), hipMemcpyDeviceToHost, ws->stream));
    HIP_TRY(hipStreamSynchronize(ws->stream));
    if (flagged) {
        HIP_TRY(hipMemsetAsync(ws->flag_ptr, 0, sizeof(int), ws->stream));
        return fail(CMR_ERR_NONFINITE, "query contains NaN/Inf or a value that rounds to Inf in the index dtype");
    }
    return CMR_OK;
}
// queries [g0, g1) of the block whose scores and offsets the workspace holds -> their `hits` sorted entries at out_ids / out_scores (host)
static int range_group(cmr_index* idx, Workspace* ws, long long ld, unsigned lo, int g0, int g1, long long hits, int64_t* out_ids, float* out_scores,
                       const CmrRangeMask* km = nullptr) {
    if (hits == 0) return CMR_OK;
    hipStream_t const s = ws->stream;
    const size_t h = (size_t)hits;
    HIP_TRY(ws->r_hits.ensure(h * 24 + cmr_sort_keys64_hist_bytes(hits)));
    u64 *ka = (u64*)ws->r_hits.p, *kb = ka + h;
    unsigned *va = (unsigned*)(kb + h), *vb = va + h, *hist = vb + h;
    HIP_TRY(cmr_launch_range_compact((const float*)ws->d_out.p, ld, idx->n, lo, (const unsigned*)ws->r_cnt.p, g0, g1 - g0, hits, ka, va, s, km));
    // the four score digits first, then the query digits that can differ inside the group: equal scores keep ascending rows
    unsigned digits = 0x0Fu;
    for (unsigned span = (unsigned)(g1 - g0 - 1), p = 4; span; span >>= 8, ++p) digits |= 1u << p;
    u64* ks = nullptr;
    unsigned* vs = nullptr;
    HIP_TRY(cmr_launch_sort_keys64(ka, kb, va, vb, hist, hits, digits, &ks, &vs, s));
    // ids over the dead key buffer, scores over the dead row buffer
    int64_t* ids_dev = (int64_t*)(ks == ka ? kb : ka);
    float* sc_dev = (float*)(vs == va ? vb : va);
    HIP_TRY(cmr_launch_range_finish(ks, vs, hits, (const float*)ws->d_out.p, ld, g0, kernel_id_base(idx), ids_dev, sc_dev, s));
    int rc = remap_ids_enqueue(idx, ids_dev, hits, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out_ids, ids_dev, h * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_scores, sc_dev, h * 4, hipMemcpyDeviceToHost, s));
    return CMR_OK;
}

extern "C" int32_t cmr_index_range_count_dev(cmr_index_t* idx, const float* q_dev, int32_t nq, float min_score, int64_t* out_counts_dev, void* stream) {
    int rc = cmr_range_args_check(idx, q_dev, out_counts_dev, nq, min_score, RowFilter{});
    if (rc) return rc;
    DevCall call(idx);
    if ((rc = range_rows_check(idx))) return rc;
    if ((rc = call.open(stream))) return rc;
    if (idx->n == 0) { HIP_TRY(hipMemsetAsync(out_counts_dev, 0, (size_t)nq * 8, call.ws->stream)); return CMR_OK; }
    const long long ld = (idx->n + 3) / 4 * 4;
    const int blockq = range_block_queries(idx, nq, ld);
    const unsigned lo = cmr_range_bound_code(min_score);
    for (int q0 = 0; q0 < nq; q0 += blockq)
        if ((rc = range_count_enqueue(idx, call.ws, q_dev + (size_t)q0 * idx->dim, std::min(blockq, nq - q0), ld, lo, (long long*)out_counts_dev + q0))) return rc;
    return CMR_OK;
}

// the arguments are checked; f: the filtered forms (none: every row)
int cmr_index_range_count_host(cmr_index_t* idx, const float* q, int nq, float min_score, int64_t* out_counts, const RowFilter& f) {
    int rc;
    const bool filtered = f.kind != RowFilter::none;
    SyncCall call(idx);
    if ((rc = range_rows_check(idx))) return rc;
    if ((rc = filter_index_check(idx, f))) return rc;
    if (idx->n == 0) { std::fill(out_counts, out_counts + nq, (int64_t)0); return CMR_OK; }
    if ((rc = call.open())) return rc;
    Workspace* const ws = call.ws;
    const long long ld = (idx->n + 3) / 4 * 4;
    const int blockq = std::min(range_block_queries(idx, nq, ld), filter_group(f, nq));      // (per-query id lists: a block is at most one group of masks)
    const unsigned lo = cmr_range_bound_code(min_score);
    HIP_TRY(ws->d_q.ensure((size_t)nq * idx->dim * 4));
    HIP_TRY(ws->r_counts.ensure((size_t)nq * 8));
    HIP_TRY(hipMemcpyAsync(ws->d_q.p, q, (size_t)nq * idx->dim * 4, hipMemcpyHostToDevice, call.s));
    FilterView mk;
    if (filtered) rc = filter_open(idx, ws, f, nq, FilterBytes::host, &mk);
    for (int q0 = 0; q0 < nq && !rc; q0 += blockq)
        rc = range_count_enqueue(idx, ws, (const float*)ws->d_q.p + (size_t)q0 * idx->dim, std::min(blockq, nq - q0), ld, lo, (long long*)ws->r_counts.p + q0,
                                 filtered ? &mk : nullptr, q0);
    if (rc) { (void)hipStreamSynchronize(call.s); return rc; }
    return range_counts_to_host(ws, nq, out_counts);
}

// the arguments are checked, *out is NULL; f: the filtered forms (none: every row)
int cmr_index_range_search_host(cmr_index_t* idx, const float* q, int nq, float min_score, int64_t max_total, cmr_range_result_t** out, const RowFilter& f) {
    int rc;
    const long long limit = max_total > 0 ? max_total : CMR_RANGE_MAX_TOTAL;
    SyncCall call(idx);
    if ((rc = range_rows_check(idx))) return rc;
    if ((rc = filter_index_check(idx, f))) return rc;
    std::unique_ptr<cmr_range_result> res(new cmr_range_result());
    res->nq = nq;
    res->lims = new int64_t[(size_t)nq + 1]();
    if (idx->n == 0) { *out = res.release(); return CMR_OK; }
    if ((rc = call.open())) return rc;
    Workspace* const ws = call.ws;
    hipStream_t const s = call.s;
    const long long ld = (idx->n + 3) / 4 * 4;
    // (per-query id lists: a block is at most one group of masks)
    const int blockq = std::min(range_block_queries(idx, nq, ld), filter_group(f, nq));
    const int nblocks = (nq + blockq - 1) / blockq;
    const unsigned lo = cmr_range_bound_code(min_score);
    const long long cap_hits = idx->range_scratch_hits > 0 ? idx->range_scratch_hits : (1ll << 30) / 24;
    HIP_TRY(ws->d_q.ensure((size_t)nq * idx->dim * 4));
    HIP_TRY(ws->r_counts.ensure((size_t)blockq * 8));
    HIP_TRY(hipMemcpyAsync(ws->d_q.p, q, (size_t)nq * idx->dim * 4, hipMemcpyHostToDevice, s));
    std::vector<int64_t> counts((size_t)nq);
    long long groups = 0;
    FilterView mk;
    const FilterView* const mkp = f.kind != RowFilter::none ? &mk : nullptr;
    if (mkp && (rc = filter_open(idx, ws, f, nq, FilterBytes::host, &mk))) { (void)hipStreamSynchronize(s); return rc; }
    auto count_block = [&](int q0, int nb) -> int {
        int rc_ = range_count_enqueue(idx, ws, (const float*)ws->d_q.p + (size_t)q0 * idx->dim, nb, ld, lo, (long long*)ws->r_counts.p, mkp, q0);
        if (!rc_) rc_ = range_counts_to_host(ws, nb, counts.data() + q0);
        return rc_;
    };
    // the size of the result is known once every block is counted, and the limit is judged before anything is allocated, compacted or
    // sorted: a batch of one block counts once; a batch of several counts them all first and scans each block again for its lists
    auto body = [&]() -> int {
        for (int q0 = 0; q0 < nq; q0 += blockq) { int rc_ = count_block(q0, std::min(blockq, nq - q0)); if (rc_) return rc_; }
        long long total = 0;
        for (int i = 0; i < nq; ++i) { total += counts[i]; res->lims[i + 1] = total; }
        if (total > limit)
            return fail(CMR_ERR_UNSUPPORTED, "range search: the batch has %lld hits, above the limit of %lld (cmr_index_range_count sizes a request)", total, limit);
        res->ids = new int64_t[(size_t)std::max<long long>(total, 1)];
        res->scores = new float[(size_t)std::max<long long>(total, 1)];
        for (int q0 = 0; q0 < nq; q0 += blockq) {
            const int nb = std::min(blockq, nq - q0);
            if (res->lims[q0 + nb] == res->lims[q0]) continue;          // no hit in the block
            if (nblocks > 1) {      // the workspace holds the last block's scores (and words): this block's again (same launches, same bits)
                int rc_ = range_count_enqueue(idx, ws, (const float*)ws->d_q.p + (size_t)q0 * idx->dim, nb, ld, lo, (long long*)ws->r_counts.p, mkp, q0);
                if (rc_) return rc_;
            }
            const CmrRangeMask km = mkp ? mk.kernel(q0) : CmrRangeMask{};
            for (int g0 = 0; g0 < nb;) {      // groups of consecutive queries of at most cap_hits hits; a query is never split
                int g1 = g0 + 1;
                long long hits = counts[q0 + g0];
                while (g1 < nb && hits + counts[q0 + g1] <= cap_hits) hits += counts[q0 + g1++];
                if (hits) {
                    ++groups;
                    int rc_ = range_group(idx, ws, ld, lo, g0, g1, hits, res->ids + res->lims[q0 + g0], res->scores + res->lims[q0 + g0], mkp ? &km : nullptr);
                    if (rc_) return rc_;
                }
                g0 = g1;
            }
        }
        return CMR_OK;
    };
    rc = body();
    const hipError_t e = hipStreamSynchronize(s);
    if (rc) return rc;
    if (e != hipSuccess) return fail(CMR_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    idx->range_blocks_last.store(nblocks, std::memory_order_relaxed);
    idx->range_groups_last.store(groups, std::memory_order_relaxed);
    *out = res.release();
    return CMR_OK;
}

// ---- the entry points: range search / count among every row, or among the rows an allow bitmap or id lists keep
static int32_t range_count_entry(cmr_index_t* idx, const float* q, int32_t nq, float min_score, int64_t* out_counts, const RowFilter& f) {
    const int rc = cmr_range_args_check(idx, q, out_counts, nq, min_score, f);
    return rc ? rc : cmr_index_range_count_host(idx, q, nq, min_score, out_counts, f);
}
static int32_t range_search_entry(cmr_index_t* idx, const float* q, int32_t nq, float min_score, int64_t max_total, cmr_range_result_t** out, const RowFilter& f) {
    if (out) *out = nullptr;
    const int rc = cmr_range_args_check(idx, q, out, nq, min_score, f);
    return rc ? rc : cmr_index_range_search_host(idx, q, nq, min_score, max_total, out, f);
}

extern "C" {

int32_t cmr_index_range_count(cmr_index_t* idx, const float* q, int32_t nq, float min_score, int64_t* out_counts) {
    return range_count_entry(idx, q, nq, min_score, out_counts, RowFilter{});
}

int32_t cmr_index_range_search(cmr_index_t* idx, const float* q, int32_t nq, float min_score, int64_t max_total, cmr_range_result_t** out) {
    return range_search_entry(idx, q, nq, min_score, max_total, out, RowFilter{});
}

int32_t cmr_index_range_count_masked(cmr_index_t* idx, const float* q, int32_t nq, float min_score, const uint32_t* allow, int64_t n_words, int32_t n_masks,
                                     int64_t* out_counts) {
    return range_count_entry(idx, q, nq, min_score, out_counts, RowFilter::of_words(allow, n_words, n_masks, n_masks > 1));
}

int32_t cmr_index_range_count_ids(cmr_index_t* idx, const float* q, int32_t nq, float min_score, int32_t mode, const int64_t* id_offsets, const int64_t* ids,
                                  int64_t n_ids, int64_t* out_counts) {
    return range_count_entry(idx, q, nq, min_score, out_counts, RowFilter::of_ids(mode, id_offsets, ids, n_ids));
}

int32_t cmr_index_range_search_masked(cmr_index_t* idx, const float* q, int32_t nq, float min_score, int64_t max_total, const uint32_t* allow, int64_t n_words,
                                      int32_t n_masks, cmr_range_result_t** out) {
    return range_search_entry(idx, q, nq, min_score, max_total, out, RowFilter::of_words(allow, n_words, n_masks, n_masks > 1));
}

int32_t cmr_index_range_search_ids(cmr_index_t* idx, const float* q, int32_t nq, float min_score, int64_t max_total, int32_t mode, const int64_t* id_offsets,
                                   const int64_t* ids, int64_t n_ids, cmr_range_result_t** out) {
    return range_search_entry(idx, q, nq, min_score, max_total, out, RowFilter::of_ids(mode, id_offsets, ids, n_ids));
}

int32_t cmr_range_result_view(const cmr_range_result_t* res, int32_t* nq, const int64_t** lims, const int64_t** ids, const float** scores) {
    if (!res) return fail(CMR_ERR_INVALID, "NULL result");
    if (nq) *nq = res->nq;
    if (lims) *lims = res->lims;
    if (ids) *ids = res->ids;
    if (scores) *scores = res->scores;
    return CMR_OK;
}

int32_t cmr_range_result_destroy(cmr_range_result_t* res) {
    delete res;
    return CMR_OK;
}

// per query an S-way merge of lists that are each in the exported order (score descending through the canonical comparison, then id
// ascending); the scores keep their bits
int32_t cmr_range_merge(int32_t n_shards, int32_t nq, const int64_t* const* lims, const int64_t* const* ids, const float* const* scores, int64_t* out_lims,
                        int64_t* out_ids, float* out_scores) {
    if (n_shards <= 0 || nq <= 0) return fail(CMR_ERR_INVALID, "n_shards and nq must be > 0");
    if (!lims || !ids || !scores || !out_lims) return fail(CMR_ERR_INVALID, "NULL argument");
    long long total = 0;
    for (int a = 0; a < n_shards; ++a) {
        if (!lims[a]) return fail(CMR_ERR_INVALID, "NULL lims of shard %d", a);
        if (lims[a][nq] > 0 && (!ids[a] || !scores[a])) return fail(CMR_ERR_INVALID, "NULL lists of shard %d", a);
        total += lims[a][nq];
    }
    if (total > 0 && (!out_ids || !out_scores)) return fail(CMR_ERR_INVALID, "NULL output");
    std::vector<int64_t> head((size_t)n_shards);
    int64_t at = 0;
    out_lims[0] = 0;
    for (int qi = 0; qi < nq; ++qi) {
        for (int a = 0; a < n_shards; ++a) head[a] = lims[a][qi];
        for (;;) {
            int best = -1;
            float bs = 0.0f;
            int64_t bi = 0;
            for (int a = 0; a < n_shards; ++a) {
                if (head[a] >= lims[a][qi + 1]) continue;
                const float sc = scores[a][head[a]] + 0.0f;
                const int64_t id = ids[a][head[a]];
                if (best < 0 || sc > bs || (sc == bs && id < bi)) { best = a; bs = sc; bi = id; }
            }
            if (best < 0) break;
            out_ids[at] = bi;
            out_scores[at] = scores[best][head[best]];
            ++at;
            ++head[best];
        }
        out_lims[qi + 1] = at;
    }
    return CMR_OK;
}

}  // extern "C"
