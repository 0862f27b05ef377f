// The row filter of the filtered calls and nothing else: the checks of a RowFilter (the descriptor is in
// cmr_internal.h), its view in a call's workspace, the masked and id-list enqueue code, and the filtered top-k and threshold entry points.
// Range search and count take the same descriptor and the same view (range_host.h).  Included by api.hip only, behind the enqueue core,
// the packed round trip and the combined calls it builds on.
#pragma once

// ---- checks that need neither an index nor a device (declared in cmr_internal.h: multi.hip runs them in front of its own handle)
int cmr_min_score_check(float min_score) {
    return min_score == min_score ? CMR_OK : fail(CMR_ERR_INVALID, "min_score is NaN");
}

// the words forms (n_words against the index: filter_index_check, under its lock)
int cmr_words_args_check(const void* allow, int nq, int64_t n_words, int n_masks) {
    if (!allow) return fail(CMR_ERR_INVALID, "NULL allow words");
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    if (n_words < 0) return fail(CMR_ERR_INVALID, "n_words %lld < 0", (long long)n_words);
    if (n_masks != 1 && n_masks != nq) return fail(CMR_ERR_INVALID, "n_masks %d is neither 1 nor nq = %d", n_masks, nq);
    return CMR_OK;
}

// the id-list forms; off_host: CSR offsets the host can read (nullptr: a shared list, or device offsets, which the kernel clamps instead)
int cmr_ids_args_check(int mode, int nq, int k, const int64_t* off_host, const int64_t* ids, int64_t n_ids) {
    if (mode != CMR_IDS_EXCLUDE && mode != CMR_IDS_ALLOW) return fail(CMR_ERR_INVALID, "mode %d is neither CMR_IDS_EXCLUDE nor CMR_IDS_ALLOW", mode);
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    if (k <= 0) return fail(CMR_ERR_INVALID, "k must be > 0");
    if (n_ids < 0) return fail(CMR_ERR_INVALID, "n_ids %lld < 0", (long long)n_ids);
    if (n_ids > 0 && !ids) return fail(CMR_ERR_INVALID, "NULL ids with n_ids = %lld", (long long)n_ids);
    if (off_host) {
        if (off_host[0] != 0) return fail(CMR_ERR_INVALID, "id_offsets[0] = %lld, not 0", (long long)off_host[0]);
        for (int i = 0; i < nq; ++i)
            if (off_host[i + 1] < off_host[i]) return fail(CMR_ERR_INVALID, "id_offsets decrease at query %d (%lld after %lld)", i, (long long)off_host[i + 1], (long long)off_host[i]);
        if (off_host[nq] != n_ids) return fail(CMR_ERR_INVALID, "id_offsets[nq] = %lld, not n_ids = %lld", (long long)off_host[nq], (long long)n_ids);
    }
    if (k > CMR_MAX_K) return fail(CMR_ERR_UNSUPPORTED, "filtered search supports k <= %d", CMR_MAX_K);
    return CMR_OK;
}

// a filter whose pointers the host can read: the ladder of its form
int cmr_filter_args_check(const RowFilter& f, int nq, int k) {
    return f.kind == RowFilter::words_form ? cmr_words_args_check(f.words, nq, f.n_words, f.n_masks) : cmr_ids_args_check(f.mode, nq, k, f.off, f.ids, f.n_ids);
}

// ---- the filter's second check, the one that reads the index (under its lock; no device call)
static int words_check(const cmr_index* idx, int64_t n_words) {      // a mask is one word per 32-row panel
    if (n_words != panels_of(idx->n)) return fail(CMR_ERR_INVALID, "n_words %lld != ceil(%lld rows / 32) = %lld", (long long)n_words, idx->n, panels_of(idx->n));
    return CMR_OK;
}
static int filter_index_check(const cmr_index* idx, const RowFilter& f) {
    return f.kind == RowFilter::words_form ? words_check(idx, f.n_words) : CMR_OK;
}
static int masked_check(const cmr_index* idx, int nq, int k, const RowFilter& f) {
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    if (k <= 0) return fail(CMR_ERR_INVALID, "k must be > 0");
    if (int rc = filter_index_check(idx, f)) return rc;
    if (k > CMR_MAX_K) return fail(CMR_ERR_UNSUPPORTED, "filtered search supports k <= %d", CMR_MAX_K);
    return CMR_OK;
}

namespace {

// Filtered search (cmr_index_search_masked*): the best k among the local rows whose bit is set in allow_dev (one word per
// 32-row panel, on the device).  Narrow passes of the pack / [sample] / scan / merge chain on the masked scan variant, all on
// ws->stream; one mask serves every query.  k <= CMR_MAX_K (checked by the caller).
// mask_stride > 0 (cmr_index_search_masked_each*): allow_dev is [nq][mask_stride], query i's words at allow_dev + i * mask_stride;
// the pass that starts at query q0 gets the pointer advanced by q0 blocks, its kernel indexes the pass's own queries from 0.
// min_score (cmr_index_search_min_score_masked / _ids): the filtered threshold search — the bound is every query's initial
// threshold as in search_enqueue, so no sampling passes; the same masked scans, the same merge.
int search_masked_enqueue(cmr_index* idx, Workspace* ws, const float* q_dev, int nq, int k, const unsigned* allow_dev, int64_t* ids_dev,
                          float* scores_dev, float* min_dev, float* max_dev, long long mask_stride = 0, const float* min_score = nullptr) {
    const PassStreams st = PassStreams::one(ws->stream);
    const int per_pass = idx->narrow_width(nq);
    for (int q0 = 0; q0 < nq; q0 += per_pass) {
        const int nqp = std::min(per_pass, nq - q0);
        PassPlan plan;
        PassRequest rq = st.request(nqp, k, Route::narrow, min_score != nullptr, 0);
        rq.masked = true;
        rq.masked_each = mask_stride > 0;
        int rc = plan_pass(idx, rq, &plan);
        if (rc) return rc;
        if (q0 == 0) idx->last_route.store(route_code(plan, min_score != nullptr) | (nqp < nq ? CMR_ROUTE_MORE_PASSES : 0), std::memory_order_relaxed);
        rc = enqueue_pass(idx, ws, st, plan, q_dev + (size_t)q0 * idx->dim, min_score, ids_dev + (size_t)q0 * k, scores_dev + (size_t)q0 * k,
                          min_dev ? min_dev + q0 : nullptr, max_dev ? max_dev + q0 : nullptr, allow_dev + (size_t)q0 * (size_t)mask_stride, mask_stride);
        if (rc) return rc;
    }
    return CMR_OK;
}

// ---- filters from row-id lists (include/comorag_hip.h: cmr_index_row_masks_dev, cmr_index_search_ids*).  The
// caller hands over row ids in the domain the searches return; the device builds the allow words next to the corpus (aux_kernels.hip:
// row_mask_fill, row_mask_apply_ids) and the masked scans of 4.15 / 4.15b run on them unchanged.  Never combined.

constexpr int kIdsGroup = 64;      // queries whose words are built and scanned together: the scratch never holds more than this many masks

// words [nm][npanels] (nm = nq with offsets, 1 without) from the lists, on s
int row_masks_enqueue(cmr_index* idx, int mode, int nq, const int64_t* off_dev, const int64_t* ids_dev, int64_t n_ids, unsigned* words, hipStream_t s) {
    const int nm = off_dev ? nq : 1, nb = (int)idx->blk_local.size(), exclude = mode == CMR_IDS_EXCLUDE;
    HIP_TRY(cmr_launch_row_mask_fill(words, nm, idx->npanels(), idx->n, exclude, s));
    HIP_TRY(cmr_launch_row_mask_apply_ids(words, idx->npanels(), idx->n, exclude, (const long long*)off_dev, nm, (const long long*)ids_dev, n_ids,
                                          kernel_id_base(idx), nb > 1 ? idx->d_blk : nullptr, nb, s));
    return CMR_OK;
}

// ---- the filter in a call's workspace: the allow words the masked scans and the masked count / compaction kernels read.  Words forms and
// a shared id list: every mask of the call, laid down once.  Per-query id lists (off_dev): the words of ONE group of at most kIdsGroup
// queries, built into the same scratch (ws->d_mask) in front of the work that reads them and behind the previous group's (stream order) —
// the scratch never holds more than that many masks, and a query's row does not depend on the group it falls into.
struct FilterView {
    const unsigned* words = nullptr; long long stride = 0, route = 0;
    int mode = 0; const int64_t* off_dev = nullptr; const int64_t* ids_dev = nullptr; int64_t n_ids = 0;
    // the range kernels' view for the block whose first query is query q0 of the call
    CmrRangeMask kernel(int q0) const { return CmrRangeMask{words, stride, off_dev ? 0 : (long long)q0}; }
};
// where the filter's bytes are when the view opens: in the caller's device memory (the _dev calls), in the workspace where the packed round
// trip put them (filter_input), or on the host — then they go up here, by plain copies on ws->stream (range search and count)
enum class FilterBytes { device, packed, host };

// queries a call works on at once as far as the filter is concerned
int filter_group(const RowFilter& f, int nq) { return f.kind == RowFilter::ids_form && f.off ? kIdsGroup : nq; }
// ws->d_lists of a call with id lists is [offsets (nq + 1) | ids]: the bytes in front of the ids
size_t filter_off_bytes(const RowFilter& f, int nq) { return f.off ? ((size_t)nq + 1) * 8 : 0; }
// the filter's bytes as an input of the packed round trip
PackedInput filter_input(const RowFilter& f, int nq) {
    if (f.kind == RowFilter::words_form) return {&Workspace::d_mask, f.words, (size_t)f.n_words * 4 * (size_t)f.n_masks};
    return {&Workspace::d_lists, f.off, filter_off_bytes(f, nq), f.ids, (size_t)f.n_ids * 8};
}

// (under the index lock, filter_index_check passed) sizes ws->d_mask; a shared list's words are built here
int filter_open(cmr_index* idx, Workspace* ws, const RowFilter& f, int nq, FilterBytes at, FilterView* v) {
    hipStream_t const s = ws->stream;
    const size_t nw = (size_t)idx->npanels();
    v->stride = f.each ? (long long)nw : 0;
    v->route = CMR_ROUTE_FILTERED | (f.each ? CMR_ROUTE_FILTERED_EACH : 0);
    if (f.kind == RowFilter::words_form) {
        if (at == FilterBytes::host) {
            const size_t bytes = (size_t)f.n_masks * nw * 4;
            HIP_TRY(ws->d_mask.ensure(std::max<size_t>(bytes, 4)));
            HIP_TRY(hipMemcpyAsync(ws->d_mask.p, f.words, bytes, hipMemcpyHostToDevice, s));
        }
        v->words = at == FilterBytes::device ? f.words : (const unsigned*)ws->d_mask.p;
        return CMR_OK;
    }
    v->route |= CMR_ROUTE_FILTERED_IDS;
    const size_t off_bytes = filter_off_bytes(f, nq), ids_bytes = (size_t)f.n_ids * 8;
    if (at == FilterBytes::host) {
        HIP_TRY(ws->d_lists.ensure(std::max<size_t>(off_bytes + ids_bytes, 8)));
        if (off_bytes) HIP_TRY(hipMemcpyAsync(ws->d_lists.p, f.off, off_bytes, hipMemcpyHostToDevice, s));
        if (ids_bytes) HIP_TRY(hipMemcpyAsync((char*)ws->d_lists.p + off_bytes, f.ids, ids_bytes, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(ws->d_mask.ensure(std::max<size_t>((size_t)(f.off ? std::min(nq, kIdsGroup) : 1) * nw * 4, 4)));
    v->words = (const unsigned*)ws->d_mask.p;
    v->mode = f.mode; v->n_ids = f.n_ids;
    v->ids_dev = at == FilterBytes::device ? f.ids : (const int64_t*)((char*)ws->d_lists.p + off_bytes);
    if (f.off) { v->off_dev = at == FilterBytes::device ? f.off : (const int64_t*)ws->d_lists.p; return CMR_OK; }
    return row_masks_enqueue(idx, f.mode, 1, nullptr, v->ids_dev, f.n_ids, (unsigned*)ws->d_mask.p, s);
}
// the words of queries [q0, q0 + nb) from per-query lists, on ws->stream; nothing to do for the other forms
int filter_words_enqueue(cmr_index* idx, Workspace* ws, const FilterView& v, int q0, int nb) {
    return v.off_dev ? row_masks_enqueue(idx, v.mode, nb, v.off_dev + q0, v.ids_dev, v.n_ids, (unsigned*)ws->d_mask.p, ws->stream) : CMR_OK;
}

// The filtered top-k and threshold search on ws->stream, every form: the view opened, then group by group the words (per-query lists) and
// the masked scans — a shared mask or list on the shared-mask scan, per-query words or lists on the per-query variant.  Only per-query
// lists make more than one group, and every group's words start at v.words; search_masked_enqueue cuts a group into its passes.
int search_filtered_enqueue(cmr_index* idx, Workspace* ws, const float* q_dev, int nq, int k, const RowFilter& f, FilterBytes at, int64_t* ids_out,
                            float* scores_out, float* min_out, float* max_out, const float* min_score = nullptr) {
    FilterView v;
    int rc = filter_open(idx, ws, f, nq, at, &v);
    if (rc) return rc;
    const int group = filter_group(f, nq);
    long long route = 0;
    for (int q0 = 0; q0 < nq; q0 += group) {
        const int nqg = std::min(group, nq - q0);
        if ((rc = filter_words_enqueue(idx, ws, v, q0, nqg))) return rc;
        rc = search_masked_enqueue(idx, ws, q_dev + (size_t)q0 * idx->dim, nqg, k, v.words, ids_out + (size_t)q0 * k, scores_out + (size_t)q0 * k,
                                   min_out ? min_out + q0 : nullptr, max_out ? max_out + q0 : nullptr, v.stride, min_score);
        if (rc) return rc;
        if (q0 == 0) route = idx->last_route.load(std::memory_order_relaxed);
    }
    if (f.kind == RowFilter::ids_form)
        idx->last_route.store(route | CMR_ROUTE_FILTERED_IDS | (group < nq ? CMR_ROUTE_MORE_PASSES : 0), std::memory_order_relaxed);
    return CMR_OK;
}

}  // namespace

// A synchronous filtered top-k or threshold call in two halves, as cmr_index_search_begin (its name is the id-list call's, which was the
// first to need the halves; every form begins here): arguments checked by the caller; finished or abandoned through
// cmr_index_search_finish / _abandon.  The packed round trip (packed_begin) with two inputs: the queries, and the filter's bytes — the
// allow words into d_mask, or [offsets (nq + 1) | ids] as one block into d_lists.
int cmr_index_search_ids_begin(cmr_index_t* idx, const float* q, int nq, int k, const RowFilter& f, bool take_lock, CmrPending** out, const float* min_score) {
    if (!idx || !q || !out) return fail(CMR_ERR_INVALID, "NULL argument");
    *out = nullptr;
    const PackedInput in[] = {{&Workspace::d_q, q, (size_t)nq * idx->dim * 4}, filter_input(f, nq)};
    return packed_begin(idx, nq, k, take_lock, in, [&](Workspace* ws, int64_t* ids_out, float* sc, float* mn, float* mx) {
        return search_filtered_enqueue(idx, ws, (const float*)ws->d_q.p, nq, k, f, FilterBytes::packed, ids_out, sc, mn, mx, min_score);
    }, out);
}

// ---- filtered host calls.  With "combine" >= 2 AND "combine_filtered" = 1, concurrent cmr_index_search_masked /
// cmr_index_search_masked_each calls of one k and one word count share ONE per-query-mask search: the leader lays the participants'
// queries and masks out as one [total][n_words] block (a shared-mask participant's words once per query of its own) and scatters the
// rows, which hold the bits of each caller's solo call (4.15b's contract).  A batch of one is the caller's own call, unchanged.
// filter: the words form — shared: [n_words], one mask for every query; each: [nq][n_words]
// min_score: the filtered threshold search (cmr_index_search_min_score_masked), which never queues
struct CombinedMasked : CombinedSearch { RowFilter filter; const float* min_score = nullptr; };
static const CombinedMasked* masked_args(const cmr_combine::Request* r) { return static_cast<const CombinedMasked*>(search_args(r)); }

// The synchronous filtered search behind the filtered host calls: begin + finish.  The caller holds the index's shared lock and has
// checked the arguments under it (masked_check), so the pending call takes none.
static int masked_call(cmr_index* idx, const CombinedMasked& a) {
    CmrPending* p = nullptr;
    const int rc = cmr_index_search_ids_begin(idx, a.q, a.nq, a.k, a.filter, false, &p, a.min_score);
    return rc ? rc : cmr_index_search_finish(p, a.ids, a.scores, a.mn, a.mx);
}

static int masked_single(cmr_index* idx, const CombinedMasked& a) {
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    const int rc = masked_check(idx, a.nq, a.k, a.filter);
    return rc ? rc : masked_call(idx, a);
}

// one lock for the batch; every participant's word count is judged under it (an append may have come in since it queued) and a
// participant that fails is answered alone
static void combined_masked_run(void* ctx, cmr_combine::Request** reqs, int n) {
    cmr_index* const idx = (cmr_index*)ctx;
    if (n == 1) { combine_answer(reqs[0], masked_single(idx, *masked_args(reqs[0]))); return; }
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    cmr_combine::Request* live[cmr_combine::kMaxWidth];
    int nl = 0;
    for (int i = 0; i < n; ++i) {
        const CombinedMasked* a = masked_args(reqs[i]);
        const int rc = masked_check(idx, a->nq, a->k, a->filter);
        if (rc) { combine_answer(reqs[i], rc); continue; }
        live[nl++] = reqs[i];
    }
    if (nl == 0) return;
    if (nl == 1) { combine_answer(live[0], masked_call(idx, *masked_args(live[0]))); return; }
    const CombinedTopk b(live, nl, (size_t)idx->dim);
    const size_t nw = (size_t)masked_args(live[0])->filter.n_words;      // (k and the word count are part of the batch's key)
    std::vector<uint32_t> words((size_t)b.all.nq * nw);
    for (int i = 0, at = 0; i < nl; at += live[i++]->nq) {
        const RowFilter& f = masked_args(live[i])->filter;
        for (int qi = 0; qi < live[i]->nq; ++qi) memcpy(words.data() + (size_t)(at + qi) * nw, f.words + (f.each ? (size_t)qi * nw : 0), nw * 4);
    }
    b.answer(live, nl, masked_call(idx, CombinedMasked{b.all, RowFilter::of_words(words.data(), (int64_t)nw, b.all.nq, true)}));
}

static void threshold_padding(int nq, int k, int64_t* out_ids, float* out_scores) {
    std::fill(out_ids, out_ids + (size_t)nq * k, (int64_t)-1);
    std::fill(out_scores, out_scores + (size_t)nq * k, -INFINITY);
}

// ---- filtered threshold search: the masked / id-list searches with the bound as every query's initial threshold, behind the
// entry point's index-free checks.  Never combined: the words form is the single call whatever "combine_filtered" says.
static int filtered_threshold(cmr_index* idx, const float* q, int nq, int k, float min_score, const RowFilter& f, int64_t* out_ids, float* out_scores) {
    CombinedMasked a{{q, nq, k, out_ids, out_scores, nullptr, nullptr}, f};
    a.min_score = &min_score;
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (int rc = masked_check(idx, nq, k, f)) return rc;
    if (idx->n == 0) { threshold_padding(nq, k, out_ids, out_scores); return CMR_OK; }      // no row: no device call
    return masked_call(idx, a);
}

extern "C" {

// each = false: allow_dev is [n_words], one mask for every query; each = true: [nq][n_words].  Never pre-filtered; the _dev forms go
// straight to the enqueue code, the host forms through the combiner where "combine_filtered" is set.
static int32_t masked_dev(cmr_index_t* idx, const float* q_dev, int32_t nq, int32_t k, const uint32_t* allow_dev, int64_t n_words, bool each,
                          int64_t* ids_dev, float* scores_dev, float* min_dev, float* max_dev, void* stream) {
    if (!idx || !q_dev || !allow_dev || !ids_dev || !scores_dev) return fail(CMR_ERR_INVALID, "NULL argument");
    const RowFilter f = RowFilter::of_words(allow_dev, n_words, each ? nq : 1, each);
    DevCall call(idx);
    int rc = masked_check(idx, nq, k, f);
    if (rc) return rc;
    rc = call.open(stream);
    if (rc) return rc;
    return search_filtered_enqueue(idx, call.ws, q_dev, nq, k, f, FilterBytes::device, ids_dev, scores_dev, min_dev, max_dev);
}

int32_t cmr_index_search_masked_dev(cmr_index_t* idx, const float* q_dev, int32_t nq, int32_t k, const uint32_t* allow_dev, int64_t n_words,
                                    int64_t* ids_dev, float* scores_dev, float* min_dev, float* max_dev, void* stream) {
    return masked_dev(idx, q_dev, nq, k, allow_dev, n_words, false, ids_dev, scores_dev, min_dev, max_dev, stream);
}

int32_t cmr_index_search_masked_each_dev(cmr_index_t* idx, const float* q_dev, int32_t nq, int32_t k, const uint32_t* allow_dev, int64_t n_words,
                                         int64_t* ids_dev, float* scores_dev, float* min_dev, float* max_dev, void* stream) {
    return masked_dev(idx, q_dev, nq, k, allow_dev, n_words, true, ids_dev, scores_dev, min_dev, max_dev, stream);
}

int32_t cmr_index_row_masks_dev(cmr_index_t* idx, int32_t mode, int32_t nq, const int64_t* id_offsets_dev, const int64_t* ids_dev, int64_t n_ids,
                                uint32_t* words_dev, int64_t n_words, void* stream) {
    if (!words_dev) return fail(CMR_ERR_INVALID, "NULL argument");
    int rc = cmr_ids_args_check(mode, nq, 1, nullptr, ids_dev, n_ids);
    if (rc) return rc;
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    DevCall call(idx);
    rc = words_check(idx, n_words);
    if (rc) return rc;
    rc = call.open();      // (no workspace: the words are the caller's)
    if (rc) return rc;
    return row_masks_enqueue(idx, mode, nq, id_offsets_dev, ids_dev, n_ids, words_dev, (hipStream_t)stream);
}

int32_t cmr_index_search_ids_dev(cmr_index_t* idx, const float* q_dev, int32_t nq, int32_t k, int32_t mode, const int64_t* id_offsets_dev,
                                 const int64_t* ids_dev, int64_t n_ids, int64_t* ids_out_dev, float* scores_out_dev, float* min_dev, float* max_dev,
                                 void* stream) {
    if (!q_dev || !ids_out_dev || !scores_out_dev) return fail(CMR_ERR_INVALID, "NULL argument");
    int rc = cmr_ids_args_check(mode, nq, k, nullptr, ids_dev, n_ids);
    if (rc) return rc;
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    DevCall call(idx);
    rc = call.open(stream);
    if (rc) return rc;
    return search_filtered_enqueue(idx, call.ws, q_dev, nq, k, RowFilter::of_ids(mode, id_offsets_dev, ids_dev, n_ids), FilterBytes::device, ids_out_dev,
                                   scores_out_dev, min_dev, max_dev);
}

int32_t cmr_index_search_ids(cmr_index_t* idx, const float* q, int32_t nq, int32_t k, int32_t mode, const int64_t* id_offsets, const int64_t* ids,
                             int64_t n_ids, int64_t* out_ids, float* out_scores, float* out_min, float* out_max) {
    if (!q || !out_ids || !out_scores) return fail(CMR_ERR_INVALID, "NULL argument");
    int rc = cmr_ids_args_check(mode, nq, k, id_offsets, ids, n_ids);
    if (rc) return rc;
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    CmrPending* p = nullptr;
    rc = cmr_index_search_ids_begin(idx, q, nq, k, RowFilter::of_ids(mode, id_offsets, ids, n_ids), true, &p);
    if (rc) return rc;
    return cmr_index_search_finish(p, out_ids, out_scores, out_min, out_max);
}

static int32_t host_masked(cmr_index_t* idx, const float* q, int32_t nq, int32_t k, const uint32_t* allow, int64_t n_words, bool each,
                           int64_t* out_ids, float* out_scores, float* out_min, float* out_max) {
    if (!idx || !q || !allow || !out_ids || !out_scores) return fail(CMR_ERR_INVALID, "NULL argument");
    const CombinedMasked a{{q, nq, k, out_ids, out_scores, out_min, out_max}, RowFilter::of_words(allow, n_words, each ? nq : 1, each)};
    const int W = idx->combine_filtered.load(std::memory_order_relaxed) ? idx->combine.load(std::memory_order_relaxed) : 0;
    // joins a batch: as cmr_index_search — fewer queries than the batch holds, arguments that pass the checks which need no lock, finite queries
    // (the batch carries one non-finite flag); everything else takes the single call and gets its result or its error there
    if (!W || nq <= 0 || nq >= W || k <= 0 || k > CMR_MAX_K || n_words <= 0 || !cmr_combine::all_finite(q, (size_t)nq * idx->dim, idx->dtype))
        return masked_single(idx, a);
    {   // a word count the index refuses gets its error here, alone (the lock is let go before the call queues: a queued caller holds none)
        std::shared_lock<std::shared_mutex> lk(idx->mu);
        const int rc = masked_check(idx, nq, k, a.filter);
        if (rc) return rc;
    }
    cmr_combine::Request r;
    r.args = (void*)static_cast<const CombinedSearch*>(&a); r.nq = nq;      // (what search_args / masked_args read)
    cmr_combine::Key key;
    key.w[0] = 5; key.w[1] = (uint64_t)k; key.w[2] = (uint64_t)n_words;      // (one kind for both forms: they share batches; never with kind 1, the unfiltered search)
    idx->combiner.submit(key, &r, W, idx->combine_wait_us.load(std::memory_order_relaxed), combined_masked_run, idx);
    return combine_result(r);
}

int32_t cmr_index_search_masked(cmr_index_t* idx, const float* q, int32_t nq, int32_t k, const uint32_t* allow, int64_t n_words,
                                int64_t* out_ids, float* out_scores, float* out_min, float* out_max) {
    return host_masked(idx, q, nq, k, allow, n_words, false, out_ids, out_scores, out_min, out_max);
}

int32_t cmr_index_search_masked_each(cmr_index_t* idx, const float* q, int32_t nq, int32_t k, const uint32_t* allow, int64_t n_words,
                                     int64_t* out_ids, float* out_scores, float* out_min, float* out_max) {
    return host_masked(idx, q, nq, k, allow, n_words, true, out_ids, out_scores, out_min, out_max);
}

int32_t cmr_index_search_min_score_masked(cmr_index_t* idx, const float* q, int32_t nq, int32_t k, float min_score, const uint32_t* allow, int64_t n_words,
                                          int32_t n_masks, int64_t* out_ids, float* out_scores) {
    if (!q || !out_ids || !out_scores) return fail(CMR_ERR_INVALID, "NULL argument");
    int rc = cmr_words_args_check(allow, nq, n_words, n_masks);
    if (rc) return rc;
    if (k <= 0) return fail(CMR_ERR_INVALID, "k must be > 0");
    if ((rc = cmr_min_score_check(min_score))) return rc;
    if (k > CMR_MAX_K) return fail(CMR_ERR_UNSUPPORTED, "filtered threshold search supports k <= %d", CMR_MAX_K);
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    return filtered_threshold(idx, q, nq, k, min_score, RowFilter::of_words(allow, n_words, n_masks, n_masks > 1), out_ids, out_scores);
}

int32_t cmr_index_search_min_score_ids(cmr_index_t* idx, const float* q, int32_t nq, int32_t k, float min_score, int32_t mode, const int64_t* id_offsets,
                                       const int64_t* ids, int64_t n_ids, int64_t* out_ids, float* out_scores) {
    if (!q || !out_ids || !out_scores) return fail(CMR_ERR_INVALID, "NULL argument");
    int rc = cmr_ids_args_check(mode, nq, k, id_offsets, ids, n_ids);
    if (rc) return rc;
    if ((rc = cmr_min_score_check(min_score))) return rc;
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    return filtered_threshold(idx, q, nq, k, min_score, RowFilter::of_ids(mode, id_offsets, ids, n_ids), out_ids, out_scores);
}

}  // extern "C"
