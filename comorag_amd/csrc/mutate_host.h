// Row mutation of one index and nothing else: truncate, removal by stable in-place compaction, in-place update.
// Every call here holds the index's exclusive lock.  Included by api.hip only, behind row_filter.h (the keep words of a removal are built
// by the id-list filter's builder).
#pragma once

// roll a shard back to n_rows (multi.hip: an append that failed on a later shard).  Slots beyond n_rows keep stale data:
// every kernel masks by row index, and the next append rewrites them.
int cmr_index_truncate(cmr_index_t* idx, long long n_rows) {
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    if (n_rows < 0 || n_rows > idx->n) return fail(CMR_ERR_INVALID, "truncate to %lld rows of %lld", n_rows, idx->n);
    idx->n = n_rows;
    idx->q8c.rows = std::min(idx->q8c.rows, n_rows);      // (the next append rewrites the slots behind: their int8 companion is stale then)
    return CMR_OK;
}

// ---- row removal by stable in-place compaction (include/comorag_hip.h: cmr_index_remove_ids; compact_kernels.hip).
// The exclusive lock is held by the caller.  Everything that can fail for want of memory happens before the first row moves.
static int remove_ids_locked(cmr_index* idx, const int64_t* ids, int64_t n_ids, int64_t* n_removed) {
    idx->rm_chunks_last = 0;
    if (n_ids == 0 || idx->n == 0) return CMR_OK;
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    // searches hold the shared lock only while they enqueue (_dev, pipelined) or until they finish (host API): whatever this process
    // has in flight on the device — the pipeline's streams, the workspaces', callers' streams — reads the rows where they are now
    HIP_TRY(hipDeviceSynchronize());
    const long long n = idx->n, nw = idx->npanels();
    hipStream_t s = nullptr;
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_words = 16, o_kb = o_words + up16((size_t)nw * 4), o_ids = o_kb + up16(((size_t)nw + 1) * 4);
    HIP_TRY(idx->rm_buf.ensure(o_ids + (size_t)n_ids * 8));
    char* const b = (char*)idx->rm_buf.p;
    long long* const info = (long long*)b;
    unsigned* const words = (unsigned*)(b + o_words);
    unsigned* const kept_before = (unsigned*)(b + o_kb);
    HIP_TRY(hipMemcpy(b + o_ids, ids, (size_t)n_ids * 8, hipMemcpyHostToDevice));
    // the keep words by the builder of the id-list searches: its ignoring rules (negative ids, ids this index does not hold, duplicates), its translation
    rc = row_masks_enqueue(idx, CMR_IDS_EXCLUDE, 1, nullptr, (const int64_t*)(b + o_ids), n_ids, words, s);
    if (rc) return rc;
    HIP_TRY(cmr_launch_keep_prefix(words, nw, n, kept_before, info, s));
    long long h[2] = {n, n};
    HIP_TRY(hipMemcpy(h, info, sizeof(h), hipMemcpyDeviceToHost));
    const long long kept = h[0], first = h[1];
    if (kept < 0 || kept > n || first < 0 || first > n) return fail(CMR_ERR_HIP, "row removal: prefix sum returned %lld kept rows, first removed row %lld of %lld", kept, first, n);
    if (kept == n) return CMR_OK;
    if (first < kept) {      // (first == kept: the removed rows are the tail — a truncate)
        const long long p0 = first / CMR_PANEL_ROWS, affected = nw - p0;
        const size_t pb = idx->panel_bytes();
        long long sp = idx->rm_stage_panels ? idx->rm_stage_panels : std::max<long long>(2, (long long)((64ull << 20) / pb));
        sp = std::max<long long>(2, std::min(sp, affected + 1));
        const size_t stage_bytes = (size_t)sp * pb;
        HIP_TRY(idx->stage.ensure(stage_bytes));
        // from here on rows move: whatever happens, the int8 companion is no longer trusted behind the first removed row
        idx->q8c.rows = std::min(idx->q8c.rows, first);
        const int ks = idx->ks();
        const long long c_panels = sp - 1;      // the destination rows of c_panels source panels may straddle one panel more
        for (long long p = p0; p < nw; p += c_panels) {
            HIP_TRY(cmr_launch_compact_chunk(idx->corpus, ks, words, kept_before, p, std::min(nw, p + c_panels), idx->stage.p, sp, s));
            ++idx->rm_chunks_last;
        }
        if (idx->shadow) {      // the same buffer, at row granularity: sp * panel bytes >= 2 * 32 * dpad * 2 bytes hold at least one panel's 32 fp32 rows
            const long long stage_rows = (long long)(stage_bytes / ((size_t)idx->dim * 4)), s_panels = stage_rows / CMR_PANEL_ROWS;
            for (long long p = p0; p < nw; p += s_panels)
                HIP_TRY(cmr_launch_compact_shadow_chunk(idx->shadow, idx->dim, words, kept_before, p, std::min(nw, p + s_panels), idx->stage.p, stage_rows, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
    }
    idx->n = kept;
    idx->q8c.rows = std::min(idx->q8c.rows, first);      // the int8 companion is not compacted: the next pre-filtered call quantises again from the first removed row's panel
    if (n_removed) *n_removed = n - kept;
    return CMR_OK;
}

// cmr_index_remove_ids without the block-table restriction, for an owner that replaces the table itself right after (multi.hip:
// the ids are translated through the table the shard has NOW; the shard's table is stale when this returns with *n_removed > 0)
int cmr_index_compact_ids(cmr_index_t* idx, const int64_t* ids, int64_t n_ids, int64_t* n_removed) {
    if (n_removed) *n_removed = 0;
    if (!idx || (n_ids > 0 && !ids) || n_ids < 0) return fail(CMR_ERR_INVALID, "bad argument");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    return remove_ids_locked(idx, ids, n_ids, n_removed);
}

extern "C" int32_t cmr_index_remove_ids(cmr_index_t* idx, const int64_t* ids, int64_t n_ids, int64_t* n_removed) {
    if (n_removed) *n_removed = 0;
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    if (n_ids < 0) return fail(CMR_ERR_INVALID, "n_ids %lld < 0", (long long)n_ids);
    if (n_ids > 0 && !ids) return fail(CMR_ERR_INVALID, "NULL ids with n_ids = %lld", (long long)n_ids);
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    if (!idx->single_block())
        return fail(CMR_ERR_UNSUPPORTED, "row removal on an index with a block table of %d blocks (cmr_index_set_id_blocks): the owner of the table removes (cmr_mindex_remove_ids)",
                    (int)idx->blk_local.size());
    return remove_ids_locked(idx, ids, n_ids, n_removed);
}

// ---- in-place row update (include/comorag_hip.h: cmr_index_update_rows; update_rows_kernel in aux_kernels.hip).
// The exclusive lock is held by the caller.  Entry i of the plan replaces local row dst[i] (strictly ascending) by source row src[i] of
// `rows` [n_rows, dim] — host memory, or device memory (on_device: read in place, one chunk).  phases: CMR_UPD_CHECK runs the check
// launch over every winning row and reports the flag, CMR_UPD_WRITE scatters and folds the maxima; both at once is the one-index call,
// which reads the flag once at the end when everything fits one chunk (the scatter and the maxima return on a raised flag by
// themselves) and runs all checks before the first store otherwise.
static int update_planned_locked(cmr_index* idx, const int64_t* dst, const int64_t* src, long long m, const float* rows, long long n_rows,
                                 bool on_device, hipStream_t s, int phases) {
    if (phases & CMR_UPD_WRITE) idx->upd_chunks_last = 0;
    if (m <= 0) return CMR_OK;
    for (long long i = 0; i < m; ++i)      // the plan is the only thing between the launches and memory that is not theirs
        if (dst[i] < 0 || dst[i] >= idx->n || (i && dst[i] <= dst[i - 1]) || src[i] < 0 || src[i] >= n_rows)
            return fail(CMR_ERR_INVALID, "row update: plan entry %lld (row %lld of %lld <- source row %lld of %lld) out of range or out of order", i,
                        (long long)dst[i], idx->n, (long long)src[i], n_rows);
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    // searches hold the shared lock only while they enqueue (_dev, pipelined): whatever is in flight on the device reads the rows as they are now
    HIP_TRY(hipDeviceSynchronize());
    const size_t row_bytes = (size_t)idx->dim * 4;
    const bool both = phases == (CMR_UPD_CHECK | CMR_UPD_WRITE);
    // chunks: the source rows go through the staging buffer upd_stage_rows (default: 256 MiB worth) at a time; a chunk's entries are the
    // plan's entries whose source row lies in it, in the plan's order (ascending rows still), and only the span they use is uploaded
    const long long chunk_rows = on_device ? std::max<long long>(1, n_rows) : idx->upd_stage_rows ? idx->upd_stage_rows : std::max<long long>(1, (256ll << 20) / (long long)row_bytes);
    const long long n_chunks = (n_rows + chunk_rows - 1) / chunk_rows;
    std::vector<long long> at((size_t)n_chunks + 1, 0), lo((size_t)n_chunks, n_rows), hi((size_t)n_chunks, -1);
    for (long long i = 0; i < m; ++i) {
        const size_t c = (size_t)(src[i] / chunk_rows);
        ++at[c + 1]; lo[c] = std::min<long long>(lo[c], src[i]); hi[c] = std::max<long long>(hi[c], src[i]);
    }
    if (on_device) lo[0] = 0;
    for (long long c = 0; c < n_chunks; ++c) at[(size_t)c + 1] += at[(size_t)c];
    std::vector<long long> plan((size_t)2 * m);      // [dst[m] | src[m], relative to the chunk's first uploaded row], chunk by chunk
    {
        std::vector<long long> fill(at.begin(), at.end() - 1);
        for (long long i = 0; i < m; ++i) {
            const size_t c = (size_t)(src[i] / chunk_rows);
            const long long o = fill[c]++;
            plan[(size_t)o] = dst[i]; plan[(size_t)(m + o)] = src[i] - lo[c];
        }
    }
    long long used = 0;
    for (long long c = 0; c < n_chunks; ++c) used += at[(size_t)c + 1] > at[(size_t)c];
    const bool mapped = !on_device && used == 1 && idx->zero_copy && !idx->upd_stage_rows && (size_t)n_rows * row_bytes <= kMappedAppendMax && (size_t)m * 16 <= kMappedPlanMax;
    const long long* d_dst = nullptr; const long long* d_src = nullptr;
    int* flag = nullptr;
    char* h = nullptr;
    if (mapped) {      // rows, plan and flag in the append's pinned, device-mapped buffer: no copy in front of the launches, no flag copy behind
        { int rc_ = ensure_h_pin(idx); if (rc_) return rc_; }
        h = (char*)idx->h_pin;
        char* d = (char*)idx->h_pin_dev;
        memset(h, 0, 8);
        memcpy(h + 256 + kMappedAppendMax, plan.data(), (size_t)m * 16);
        flag = (int*)d;
        d_dst = (const long long*)(d + 256 + kMappedAppendMax); d_src = d_dst + m;
    } else {
        HIP_TRY(idx->rm_buf.ensure((size_t)m * 16));
        HIP_TRY(hipMemcpy(idx->rm_buf.p, plan.data(), (size_t)m * 16, hipMemcpyHostToDevice));
        flag = idx->d_flag;
        HIP_TRY(hipMemsetAsync(flag, 0, sizeof(int), s));
        d_dst = (const long long*)idx->rm_buf.p; d_src = d_dst + m;
        if (!on_device) {
            long long span = 0;
            for (long long c = 0; c < n_chunks; ++c) span = std::max(span, hi[(size_t)c] - lo[(size_t)c] + 1);
            hipError_t e = idx->stage.ensure((size_t)span * row_bytes);
            if (e != hipSuccess) return fail(CMR_ERR_OOM, "row update staging: %s", hipGetErrorString(e));
        }
    }
    // the chunk's source rows where the launches read them
    auto stage_chunk = [&](long long c, const float** out) -> int {
        if (on_device) { *out = rows; return CMR_OK; }
        const size_t bytes = (size_t)(hi[(size_t)c] - lo[(size_t)c] + 1) * row_bytes;
        const float* from = rows + (size_t)lo[(size_t)c] * idx->dim;
        if (mapped) { memcpy(h + 256, from, bytes); *out = (const float*)((char*)idx->h_pin_dev + 256); return CMR_OK; }
        HIP_TRY(hipMemcpyAsync(idx->stage.p, from, bytes, hipMemcpyHostToDevice, s));
        *out = (const float*)idx->stage.p;
        return CMR_OK;
    };
    auto read_flag = [&](int* out) -> int {
        if (mapped) { HIP_TRY(hipStreamSynchronize(s)); memcpy(out, h, sizeof(int)); return CMR_OK; }
        HIP_TRY(hipMemcpyAsync(out, flag, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return CMR_OK;
    };
    auto write_chunk = [&](long long c, const float* r) -> int {
        const long long o = at[(size_t)c], mc = at[(size_t)c + 1] - o;
        HIP_TRY(cmr_launch_update_rows(idx->dtype, false, r, d_dst + o, d_src + o, mc, idx->dim, idx->dpad, idx->corpus, idx->shadow, flag, s));
        HIP_TRY(cmr_launch_round_stats(idx->dtype, r, mc, idx->dim, flag, idx->d_stats, s, d_src + o));
        ++idx->upd_chunks_last;
        return CMR_OK;
    };
    const char* const nonfinite = "updated rows contain NaN/Inf or a value that rounds to Inf in the index dtype (index unchanged)";
    int flagged = 0;
    const bool one_pass = both && used == 1;
    if (phases & CMR_UPD_CHECK) {
        for (long long c = 0; c < n_chunks; ++c) {
            const long long o = at[(size_t)c], mc = at[(size_t)c + 1] - o;
            if (!mc) continue;
            const float* r = nullptr;
            if ((rc = stage_chunk(c, &r))) return rc;
            HIP_TRY(cmr_launch_update_rows(idx->dtype, true, r, d_dst + o, d_src + o, mc, idx->dim, idx->dpad, nullptr, nullptr, flag, s));
            if (one_pass) {      // the same upload feeds the stores: they return on the flag the check launch in front of them raised
                idx->q8c.rows = std::min<long long>(idx->q8c.rows, dst[0]);
                if ((rc = write_chunk(c, r))) return rc;
            }
        }
        if ((rc = read_flag(&flagged))) return rc;
        if (flagged) { idx->upd_chunks_last = 0; return fail(CMR_ERR_NONFINITE, "%s", nonfinite); }
        if (one_pass) return CMR_OK;
    }
    if (phases & CMR_UPD_WRITE) {
        // from the first store on the int8 companion is stale behind the first updated row: the next pre-filtered call quantises again from its panel
        idx->q8c.rows = std::min<long long>(idx->q8c.rows, dst[0]);
        for (long long c = 0; c < n_chunks; ++c) {
            if (at[(size_t)c + 1] == at[(size_t)c]) continue;
            const float* r = nullptr;
            if ((rc = stage_chunk(c, &r))) return rc;
            if ((rc = write_chunk(c, r))) return rc;
        }
        HIP_TRY(hipStreamSynchronize(s));
    }
    return CMR_OK;
}

// one shard's share of cmr_mindex_update_rows (multi.hip plans and owns the block tables): local rows, ascending, and the source rows they take
int cmr_index_update_planned(cmr_index_t* idx, const int64_t* local_rows, const int64_t* src, int64_t m, const float* rows, int64_t n_rows, int phases) {
    if (!idx || m < 0 || (m > 0 && (!local_rows || !src || !rows))) return fail(CMR_ERR_INVALID, "bad argument");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    return update_planned_locked(idx, local_rows, src, m, rows, n_rows, false, nullptr, phases);
}

static int32_t update_rows_entry(cmr_index_t* idx, const int64_t* ids, const float* rows, int64_t n, bool on_device, void* stream, int64_t* n_updated) {
    if (n_updated) *n_updated = 0;
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    if (n < 0) return fail(CMR_ERR_INVALID, "n %lld < 0", (long long)n);
    if (n > 0 && (!ids || !rows)) return fail(CMR_ERR_INVALID, "NULL ids or rows with n = %lld", (long long)n);
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    idx->upd_chunks_last = 0;
    if (n == 0 || idx->n == 0) return CMR_OK;
    // the one id parser (cmr_mindex_plan_update): this index is its one-shard case, id base or block table as shard 0's table
    const int64_t rows_of = idx->n, zero = 0, base = idx->id_base;
    const int32_t nb = idx->single_block() ? 1 : (int32_t)idx->blk_local.size();
    const int64_t* bl = idx->single_block() ? &zero : (const int64_t*)idx->blk_local.data();
    const int64_t* bg = idx->single_block() ? &base : (const int64_t*)idx->blk_global.data();
    std::vector<int32_t> shard((size_t)n);
    std::vector<int64_t> local((size_t)n), src((size_t)n);
    int64_t count = 0, m = 0;
    int rc = cmr_mindex_plan_update(1, &rows_of, &nb, bl, bg, ids, n, shard.data(), local.data(), src.data(), &count, &m);
    if (rc) return rc;
    rc = update_planned_locked(idx, local.data(), src.data(), m, rows, n, on_device, (hipStream_t)stream, CMR_UPD_CHECK | CMR_UPD_WRITE);
    if (!rc && n_updated) *n_updated = m;
    return rc;
}

extern "C" int32_t cmr_index_update_rows(cmr_index_t* idx, const int64_t* ids, const float* rows_f32, int64_t n, int64_t* n_updated) {
    return update_rows_entry(idx, ids, rows_f32, n, false, nullptr, n_updated);
}

extern "C" int32_t cmr_index_update_rows_dev(cmr_index_t* idx, const int64_t* ids_host, const float* rows_f32_dev, int64_t n, void* stream, int64_t* n_updated) {
    return update_rows_entry(idx, ids_host, rows_f32_dev, n, true, stream, n_updated);
}
