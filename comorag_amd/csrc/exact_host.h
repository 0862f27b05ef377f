// Exact fp32 top-k of a 16-bit index and nothing else: stage-1 candidates from the ordinary search, re-score and
// certificate.  Its scratch is in index_state.h.  Included by api.hip only, behind the enqueue core it calls.
#pragma once

// ---- exact fp32 top-k of a 16-bit index (include/comorag_hip.h: cmr_index_search_exact)
namespace {

int exact_scratch(ExactScratch* X, int nq, int kc, int k, bool outs, hipStream_t s) {
    HIP_TRY(X->ids.ensure((size_t)nq * kc * 8));
    HIP_TRY(X->sc.ensure((size_t)nq * kc * 4));
    HIP_TRY(X->part.ensure(cmr_exact_part_bytes(nq, kc)));
    if ((size_t)nq * sizeof(int) > X->arrive.cap || !X->arrive.p) {      // arrival counters: zeroed once, re-armed by the kernel
        HIP_TRY(X->arrive.ensure((size_t)nq * sizeof(int)));
        HIP_TRY(hipMemsetAsync(X->arrive.p, 0, X->arrive.cap, s));
    }
    if (outs) {
        HIP_TRY(X->oids.ensure((size_t)nq * k * 8));
        HIP_TRY(X->osc.ensure((size_t)nq * k * 4));
        HIP_TRY(X->oex.ensure((size_t)nq * 4));
    }
    return CMR_OK;
}

// re-score + certify the stage-1 lists in X (global ids, as every search returns them) on `s`; output ids translated like any search's
int exact_certify_enqueue(cmr_index* idx, ExactScratch* X, const float* q_dev, int nq, int kc, int k, int64_t* ids_dev, float* scores_dev,
                          int* exact_dev, hipStream_t s) {
    const int nb = (int)idx->blk_local.size();
    HIP_TRY(cmr_launch_exact_certify(idx->dtype, idx->shadow, idx->dim, idx->n, kernel_id_base(idx), nb > 1 ? idx->d_blk : nullptr, nb, q_dev, nq,
                                     (const int64_t*)X->ids.p, (const float*)X->sc.p, kc, k, idx->d_stats, X->part.p, (int*)X->arrive.p,
                                     ids_dev, scores_dev, exact_dev, s));
    return remap_ids_enqueue(idx, ids_dev, (long long)nq * k, s);
}

int exact_check(const cmr_index* idx, int k) {
    if (k <= 0 || k > 64) return fail(CMR_ERR_UNSUPPORTED, "exact search supports k in [1, 64], got %d", k);
    if (idx->dtype == CMR_F32) return CMR_OK;
    if (!(idx->flags & CMR_FLAG_KEEP_F32)) return fail(CMR_ERR_UNSUPPORTED, "exact search of a 16-bit index needs CMR_FLAG_KEEP_F32 (the fp32 shadow)");
    if (idx->exact_cand <= k) return fail(CMR_ERR_UNSUPPORTED, "exact_cand %d must be > k %d", idx->exact_cand, k);
    return CMR_OK;
}

}  // namespace

extern "C" {

int32_t cmr_index_search_exact(cmr_index_t* idx, const float* q, int32_t nq, int32_t k, int64_t* out_ids, float* out_scores, int32_t* out_exact) {
    if (!idx || !q || !out_ids || !out_scores || !out_exact) return fail(CMR_ERR_INVALID, "NULL argument");
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    { int rc_ = exact_check(idx, k); if (rc_) return rc_; }
    if (idx->dtype == CMR_F32) {      // an fp32 index ranks with fp32 arithmetic already: the plain search is the exact one
        const int rc = host_search(idx, q, nq, k, out_ids, out_scores, nullptr, nullptr, nullptr);
        if (rc) return rc;
        for (int i = 0; i < nq; ++i) out_exact[i] = 1;
        return CMR_OK;
    }
    SyncCall call(idx);
    int rc = call.open();
    if (rc) return rc;
    Workspace* const ws = call.ws;
    hipStream_t const s = call.s;
    ExactScratch* X = &ws->x;
    // one stage: top-kc of the 16-bit scan, re-score + certify, results to the host
    auto stage = [&](const float* qh, int n_q, int kc, int64_t* oi, float* os, int32_t* oe) -> int {
        HIP_TRY(ws->d_q.ensure((size_t)n_q * idx->dim * 4));
        HIP_TRY(hipMemcpyAsync(ws->d_q.p, qh, (size_t)n_q * idx->dim * 4, hipMemcpyHostToDevice, s));
        int rc_ = exact_scratch(X, n_q, kc, k, true, s);
        if (!rc_) rc_ = arm_flag(ws, s);
        if (!rc_) rc_ = search_enqueue(idx, ws, (const float*)ws->d_q.p, n_q, kc, (int64_t*)X->ids.p, (float*)X->sc.p, nullptr, nullptr);
        if (!rc_) rc_ = exact_certify_enqueue(idx, X, (const float*)ws->d_q.p, n_q, kc, k, (int64_t*)X->oids.p, (float*)X->osc.p, (int*)X->oex.p, s);
        if (rc_) { (void)hipStreamSynchronize(s); return rc_; }
        HIP_TRY(hipMemcpyAsync(oi, X->oids.p, (size_t)n_q * k * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(os, X->osc.p, (size_t)n_q * k * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(oe, X->oex.p, (size_t)n_q * 4, hipMemcpyDeviceToHost, s));
        return check_query_flag(ws);     // (synchronises)
    };
    rc = stage(q, nq, idx->exact_cand, out_ids, out_scores, out_exact);
    if (rc) return rc;
    // stage 2: the queries stage 1 could not certify, again from the two-pass search's CMR_MAX_K_2PASS candidates
    std::vector<int> u;
    for (int i = 0; i < nq; ++i) if (!out_exact[i]) u.push_back(i);
    if (u.empty() || idx->n <= idx->exact_cand) return CMR_OK;
    const int nu = (int)u.size(), kc2 = (int)std::min<long long>(CMR_MAX_K_2PASS, idx->n), d = idx->dim;
    std::vector<float> q2((size_t)nu * d);
    std::vector<int64_t> i2((size_t)nu * k);
    std::vector<float> s2((size_t)nu * k);
    std::vector<int32_t> e2((size_t)nu);
    for (int j = 0; j < nu; ++j) memcpy(&q2[(size_t)j * d], q + (size_t)u[j] * d, (size_t)d * 4);
    rc = stage(q2.data(), nu, kc2, i2.data(), s2.data(), e2.data());
    if (rc) return rc;
    for (int j = 0; j < nu; ++j) {
        memcpy(out_ids + (size_t)u[j] * k, &i2[(size_t)j * k], (size_t)k * 8);
        memcpy(out_scores + (size_t)u[j] * k, &s2[(size_t)j * k], (size_t)k * 4);
        out_exact[u[j]] = e2[j];
    }
    return CMR_OK;
}

int32_t cmr_index_search_exact_pipelined(cmr_index_t* idx, const float* q_dev, int32_t nq, int32_t k, int64_t* ids_dev, float* scores_dev,
                                         int32_t* exact_dev, void* wait_event, void** done_event) {
    if (!idx || !q_dev || !ids_dev || !scores_dev || !exact_dev) return fail(CMR_ERR_INVALID, "NULL argument");
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    { int rc_ = exact_check(idx, k); if (rc_) return rc_; }
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    std::lock_guard<std::mutex> pl(idx->pipe_mu);
    rc = ensure_pipe(idx);
    if (rc) return rc;
    hipStream_t const sq = idx->pipe.st[Pipe::sq];
    hipEvent_t done = nullptr;
    if (idx->dtype == CMR_F32) {
        rc = search_pipelined_enqueue_locked(idx, q_dev, nq, k, ids_dev, scores_dev, nullptr, nullptr, (hipEvent_t)wait_event, &done, nullptr);
        if (rc) return rc;
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)exact_dev, 1, (size_t)nq, sq));
    } else {
        // stage-1 candidates in per-slot scratch: their writers (the merges) and their reader (the re-score) are all on the post stream,
        // which orders each slot's next use behind this one
        const int kc = idx->exact_cand;
        ExactScratch* X = &idx->x_slot[idx->x_next++ % CMR_PIPE_SLOTS];
        rc = exact_scratch(X, nq, kc, k, false, sq);
        if (rc) return rc;
        rc = search_pipelined_enqueue_locked(idx, q_dev, nq, kc, (int64_t*)X->ids.p, (float*)X->sc.p, nullptr, nullptr, (hipEvent_t)wait_event, &done, nullptr);
        if (rc) return rc;
        rc = exact_certify_enqueue(idx, X, q_dev, nq, kc, k, ids_dev, scores_dev, exact_dev, sq);
        if (rc) return rc;
    }
    HIP_TRY(hipEventRecord(done, sq));      // (the last slot's main_done, re-recorded behind the re-score)
    if (done_event) *done_event = (void*)done;
    return CMR_OK;
}

}  // extern "C"
