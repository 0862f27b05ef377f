// Diversified top-k, maximal marginal relevance, and nothing else: the device path of one index and cmr_index_gram_rows for
// the shards of multi.hip.  The selection itself is mmr_select.h.  Included by api.hip only, behind the packed round trip it calls.
#pragma once

// ---- diversified top-k: maximal marginal relevance (include/comorag_hip.h: cmr_index_search_mmr, cmr_index_mmr_select,
// cmr_index_pair_scores).  Candidates [nq, F] of ANY search (global ids, -1 / -inf padded) -> their local rows (void
// positions -1) -> their pair scores with the scan's bits -> the greedy selection, all on the call's stream; only [nq, k] comes back.
// Never combined, pre-filtered or pipelined.
// (declared in cmr_internal.h: multi.hip runs the same check in front of its own handle)
int cmr_mmr_args_check(int nq, int F, int k, double lam) {
    const int bad = cmr_mmr::check_args(nq, F, k, lam, CMR_MAX_K);
    if (bad == 2) return fail(CMR_ERR_UNSUPPORTED, "fetch_k = %d above CMR_MAX_K = %d", F, CMR_MAX_K);
    if (bad) return fail(CMR_ERR_INVALID, "need nq >= 1, 1 <= k <= fetch_k and lambda in [0, 1] (nq %d, k %d, fetch_k %d, lambda %g)", nq, k, F, lam);
    return CMR_OK;
}

extern "C" {

// local rows and pair scores of the candidates ids_dev [nq, F] into ws->m_rows / ws->m_gram; qfrag: see cmr_launch_mmr_gram
static int mmr_gram_enqueue(cmr_index* idx, Workspace* ws, const int64_t* ids_dev, int nq, int F, const void* qfrag) {
    hipStream_t const s = ws->stream;
    const int nb = (int)idx->blk_local.size();
    HIP_TRY(ws->m_rows.ensure((size_t)nq * F * 8));
    HIP_TRY(ws->m_gram.ensure((size_t)nq * F * F * 4));
    HIP_TRY(cmr_launch_mmr_rows(ids_dev, nq, F, idx->n, kernel_id_base(idx), nb > 1 ? idx->d_blk : nullptr, nb, (long long*)ws->m_rows.p, s));
    HIP_TRY(cmr_launch_mmr_gram(idx->dtype, idx->corpus, qfrag, (const long long*)ws->m_rows.p, nq, F, idx->dpad, (float*)ws->m_gram.p, s));
    return CMR_OK;
}

static int mmr_select_enqueue(cmr_index* idx, Workspace* ws, const int64_t* ids_dev, const float* sc_dev, int nq, int F, int k, float lam32,
                              int64_t* out_ids_dev, float* out_scores_dev) {
    const int rc = mmr_gram_enqueue(idx, ws, ids_dev, nq, F, nullptr);
    if (rc) return rc;
    HIP_TRY(cmr_launch_mmr_select(ids_dev, sc_dev, (const long long*)ws->m_rows.p, (const float*)ws->m_gram.p, nq, F, k, lam32, out_ids_dev,
                                  out_scores_dev, ws->stream));
    return CMR_OK;
}

// the ordinary search for F candidates (whichever route the plan picks) into ws->m_ids / ws->m_sc, then the selection
static int search_mmr_enqueue(cmr_index* idx, Workspace* ws, const float* q_dev, int nq, int k, int F, float lam32, int64_t* out_ids_dev,
                              float* out_scores_dev) {
    HIP_TRY(ws->m_ids.ensure((size_t)nq * F * 8));
    HIP_TRY(ws->m_sc.ensure((size_t)nq * F * 4));
    if (idx->n > 0) {
        const int rc = search_enqueue(idx, ws, q_dev, nq, F, (int64_t*)ws->m_ids.p, (float*)ws->m_sc.p, nullptr, nullptr);
        if (rc) return rc;
        idx->last_route.fetch_or(CMR_ROUTE_MMR, std::memory_order_relaxed);
    } else {      // no rows: every candidate is padding (id -1; its score is never read)
        HIP_TRY(hipMemsetAsync(ws->m_ids.p, 0xFF, (size_t)nq * F * 8, ws->stream));
        HIP_TRY(hipMemsetAsync(ws->m_sc.p, 0, (size_t)nq * F * 4, ws->stream));
        idx->last_route.store(CMR_ROUTE_MMR, std::memory_order_relaxed);
    }
    return mmr_select_enqueue(idx, ws, (const int64_t*)ws->m_ids.p, (const float*)ws->m_sc.p, nq, F, k, lam32, out_ids_dev, out_scores_dev);
}

int32_t cmr_mmr_select(const float* rel, const float* gram, const int64_t* ids, int32_t nq, int32_t F, int32_t k, double lam, int64_t* out_ids,
                       float* out_scores) {
    if (!rel || !gram || !ids || !out_ids || !out_scores) return fail(CMR_ERR_INVALID, "NULL argument");
    { int rc_ = cmr_mmr_args_check(nq, F, k, lam); if (rc_) return rc_; }
    if (cmr_mmr::any_nan(rel, (size_t)nq * F)) return fail(CMR_ERR_INVALID, "NaN among the relevance scores");
    cmr_mmr::select(rel, gram, ids, nq, F, k, (float)lam, out_ids, out_scores);
    return CMR_OK;
}

int32_t cmr_index_pair_scores(cmr_index_t* idx, const int64_t* ids, int32_t nq, int32_t F, float* out) {
    if (!ids || !out) return fail(CMR_ERR_INVALID, "NULL argument");
    { int rc_ = cmr_mmr_args_check(nq, F, 1, 0.0); if (rc_) return rc_; }
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    SyncCall call(idx);
    int rc = call.open();
    if (rc) return rc;
    Workspace* const ws = call.ws;
    hipStream_t const s = call.s;
    HIP_TRY(ws->m_ids.ensure((size_t)nq * F * 8));
    HIP_TRY(hipMemcpyAsync(ws->m_ids.p, ids, (size_t)nq * F * 8, hipMemcpyHostToDevice, s));
    rc = mmr_gram_enqueue(idx, ws, (const int64_t*)ws->m_ids.p, nq, F, nullptr);
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    HIP_TRY(hipMemcpyAsync(out, ws->m_gram.p, (size_t)nq * F * F * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return CMR_OK;
}

int32_t cmr_index_mmr_select_dev(cmr_index_t* idx, const int64_t* cand_ids_dev, const float* cand_scores_dev, int32_t nq, int32_t F, int32_t k,
                                 double lam, int64_t* out_ids_dev, float* out_scores_dev, void* stream) {
    if (!cand_ids_dev || !cand_scores_dev || !out_ids_dev || !out_scores_dev) return fail(CMR_ERR_INVALID, "NULL argument");
    { int rc_ = cmr_mmr_args_check(nq, F, k, lam); if (rc_) return rc_; }
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    DevCall call(idx);
    const int rc = call.open(stream);
    if (rc) return rc;
    return mmr_select_enqueue(idx, call.ws, cand_ids_dev, cand_scores_dev, nq, F, k, (float)lam, out_ids_dev, out_scores_dev);
}

int32_t cmr_index_mmr_select(cmr_index_t* idx, const int64_t* cand_ids, const float* cand_scores, int32_t nq, int32_t F, int32_t k, double lam,
                             int64_t* out_ids, float* out_scores) {
    if (!cand_ids || !cand_scores || !out_ids || !out_scores) return fail(CMR_ERR_INVALID, "NULL argument");
    { int rc_ = cmr_mmr_args_check(nq, F, k, lam); if (rc_) return rc_; }
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    if (cmr_mmr::any_nan(cand_scores, (size_t)nq * F)) return fail(CMR_ERR_INVALID, "NaN among the candidate scores");
    const PackedInput in[] = {{&Workspace::m_ids, cand_ids, (size_t)nq * F * 8}, {&Workspace::m_sc, cand_scores, (size_t)nq * F * 4}};
    CmrPending* p = nullptr;
    const int rc = packed_begin(idx, nq, k, true, in, [&](Workspace* w, int64_t* ids, float* sc, float*, float*) {
        return mmr_select_enqueue(idx, w, (const int64_t*)w->m_ids.p, (const float*)w->m_sc.p, nq, F, k, (float)lam, ids, sc);
    }, &p);
    if (rc) return rc;
    return cmr_index_search_finish(p, out_ids, out_scores, nullptr, nullptr);
}

int32_t cmr_index_search_mmr_dev(cmr_index_t* idx, const float* q_dev, int32_t nq, int32_t k, int32_t fetch_k, double lam, int64_t* ids_dev,
                                 float* scores_dev, void* stream) {
    if (!q_dev || !ids_dev || !scores_dev) return fail(CMR_ERR_INVALID, "NULL argument");
    { int rc_ = cmr_mmr_args_check(nq, fetch_k, k, lam); if (rc_) return rc_; }
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    DevCall call(idx);
    const int rc = call.open(stream);
    if (rc) return rc;
    return search_mmr_enqueue(idx, call.ws, q_dev, nq, k, fetch_k, (float)lam, ids_dev, scores_dev);
}

// one packed round trip: the queries up, [nq, k] ids and scores and the non-finite flag down
int32_t cmr_index_search_mmr(cmr_index_t* idx, const float* q, int32_t nq, int32_t k, int32_t fetch_k, double lam, int64_t* out_ids,
                             float* out_scores) {
    if (!q || !out_ids || !out_scores) return fail(CMR_ERR_INVALID, "NULL argument");
    { int rc_ = cmr_mmr_args_check(nq, fetch_k, k, lam); if (rc_) return rc_; }
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    const PackedInput in[] = {{&Workspace::d_q, q, (size_t)nq * idx->dim * 4}};
    CmrPending* p = nullptr;
    const int rc = packed_begin(idx, nq, k, true, in, [&](Workspace* w, int64_t* ids, float* sc, float*, float*) {
        return search_mmr_enqueue(idx, w, (const float*)w->d_q.p, nq, k, fetch_k, (float)lam, ids, sc);
    }, &p);
    if (rc) return rc;
    return cmr_index_search_finish(p, out_ids, out_scores, nullptr, nullptr);
}

}  // extern "C"

int cmr_index_gram_rows(cmr_index_t* idx, const float* rows, const int64_t* ids, int nq, int F, float* out) {
    SyncCall call(idx);
    int rc = call.open();
    if (rc) return rc;
    Workspace* const ws = call.ws;
    hipStream_t const s = call.s;
    const int T = (F + 31) / 32;
    const size_t row_bytes = (size_t)nq * T * 32 * idx->dim * 4;
    HIP_TRY(ws->d_q.ensure(row_bytes));
    HIP_TRY(ws->m_ids.ensure((size_t)nq * F * 8));
    HIP_TRY(ws->qfrag.ensure((size_t)nq * T * idx->ks() * 1024));
    rc = arm_flag(ws, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ws->d_q.p, rows, row_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws->m_ids.p, ids, (size_t)nq * F * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(cmr_launch_prep_queries(idx->dtype, (const float*)ws->d_q.p, nq * T * 32, idx->dim, idx->dpad, nq * T, ws->qfrag.p, ws->flag_ptr, s));
    rc = mmr_gram_enqueue(idx, ws, (const int64_t*)ws->m_ids.p, nq, F, ws->qfrag.p);
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    HIP_TRY(hipMemcpyAsync(out, ws->m_gram.p, (size_t)nq * F * F * 4, hipMemcpyDeviceToHost, s));
    return check_query_flag(ws);      // (synchronises; stored rows are finite, so the flag stays clear)
}
