// C-ABI of libcomorag_hip.so (include/comorag_hip.h): index lifetime, append, search, scores,
// re-score, shard merge, profiling; the filtered, range, exact, diversified and row-mutation calls are in the headers included at the end.  Host-side C++: what a C entry point checks and how a planned pass is enqueued (the
// state lives in index_state.h, the route and shape decisions in search_plan.h); every numeric step is a HIP
// kernel from scan_kernels.hip / aux_kernels.hip.  There is no CPU fallback in this library.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <atomic>
#include <climits>
#include <map>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "../../include/comorag_hip.h"
#include "cmr_kernels.h"
#include "cmr_internal.h"
#include "index_state.h"
#include "search_plan.h"
#include "prefilter_host.h"
#include "mmr_select.h"

namespace {
thread_local std::string g_err;
}

// sets the thread's error message; used by every host source of the library
int cmr_fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define fail cmr_fail

int cmr_set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return CMR_OK;
}

namespace {

// Route selectors of an index (cmr_index_set_option).  Every one of them picks between implementations that return the
// SAME results; they exist so that tests can hold the routes against each other and tools can A/B a kernel decision.
// One row per name: where a value is stored and what happens to it on the way — taken as it is (any), clamped to [a, b]
// (clamp), or refused with `reject` unless it is one of a / b / c (oneof), inside [a, b] (range) or 0 or inside [a, b] (zero_or) — and, for the names
// cmr_index_get_option answers, how it is read.  The measurements behind the defaults are on the fields (index_state.h).
struct Option {
    const char* name;
    void (*store)(cmr_index*, long long);      // nullptr: read-only
    enum Kind { any, clamp, oneof, range, zero_or } kind;
    long long a, b, c;
    const char* reject;
    long long (*read)(const cmr_index*);       // nullptr: not readable
};
#define CMR_STR_(x) #x
#define CMR_STR(x) CMR_STR_(x)
#define OPT_FIELD(f) [](cmr_index* i, long long v) { i->f = (decltype(i->f))v; }
#define OPT_READ(expr) [](const cmr_index* i) -> long long { return expr; }
const Option kOptions[] = {
    {"scan_ring", OPT_FIELD(force_ring), Option::any, 0, 0, 0, nullptr, nullptr},
    {"scan_asm_ring", OPT_FIELD(force_asm), Option::any, 0, 0, 0, nullptr, nullptr},
    {"scan_grid", OPT_FIELD(force_grid), Option::any, 0, 0, 0, nullptr, nullptr},
    {"scan_no_sample", OPT_FIELD(no_sample), Option::any, 0, 0, 0, nullptr, nullptr},
    {"scan_no_wide", OPT_FIELD(no_wide), Option::any, 0, 0, 0, nullptr, nullptr},
    {"scan_no_tiny", OPT_FIELD(no_tiny), Option::any, 0, 0, 0, nullptr, nullptr},
    {"scan_no_small", OPT_FIELD(no_small), Option::any, 0, 0, 0, nullptr, nullptr},
    {"small_max_panels", OPT_FIELD(small_max_panels), Option::clamp, 32, 6144, 0, nullptr, nullptr},
    {"tiny_multi", OPT_FIELD(tiny_multi), Option::any, 0, 0, 0, nullptr, nullptr},
    {"zero_copy", OPT_FIELD(zero_copy), Option::any, 0, 0, 0, nullptr, nullptr},
    {"sample_single", OPT_FIELD(single_level), Option::any, 0, 0, 0, nullptr, nullptr},
    {"sample_single_max", OPT_FIELD(single_level_max), Option::clamp, 0, LLONG_MAX, 0, nullptr, nullptr},
    {"sample_tau_in_scan", OPT_FIELD(tau_in_scan), Option::any, 0, 0, 0, nullptr, nullptr},
    {"scan_fin", OPT_FIELD(scan_fin), Option::any, 0, 0, 0, nullptr, nullptr},
    {"sync_poll", OPT_FIELD(sync_poll), Option::any, 0, 0, 0, nullptr, nullptr},
    {"scan_fin_dense", OPT_FIELD(fin_dense), Option::clamp, 1, 1 << 16, 0, nullptr, nullptr},
    {"scan_fin_cap", OPT_FIELD(fin_cap), Option::oneof, 0, 128, 256, "scan_fin_cap must be 0, 128 or 256", nullptr},
    {"scan_fin_suppliers", OPT_FIELD(fin_suppliers), Option::clamp, 0, CMR_FIN_SLOTS / CMR_SCAN_WAVES, 0, nullptr, nullptr},
    {"scan_fin_spin", OPT_FIELD(fin_spin), Option::clamp, 0, 1000, 0, nullptr, nullptr},
    {"scan_fin_queries", OPT_FIELD(fin_max_q), Option::clamp, 1, CMR_FIN_MAX_QUERIES, 0, nullptr, nullptr},
    {"sample_div", OPT_FIELD(sample_div), Option::clamp, 2, LLONG_MAX, 0, nullptr, nullptr},
    {"sample_maxmul", OPT_FIELD(sample_maxmul), Option::clamp, 0, LLONG_MAX, 0, nullptr, nullptr},
    {"pipe_reserve_cus", OPT_FIELD(reserve_cus), Option::any, 0, 0, 0, nullptr, nullptr},
    {"pipe_slots", OPT_FIELD(pipe_slots), Option::any, 0, 0, 0, nullptr, nullptr},
    {"wide_mode", OPT_FIELD(wide_mode), Option::range, 0, 2, 0, "wide_mode must be 0 (default), 1 (register-resident kernel) or 2 (query-split grid)", nullptr},
    {"stream_nt", OPT_FIELD(stream_nt), Option::any, 0, 0, 0, nullptr, nullptr},
    {"pipe_dual_scan", OPT_FIELD(dual_scan), Option::any, 0, 0, 0, nullptr, nullptr},
    {"pipe_cu_mask", OPT_FIELD(cu_mask), Option::any, 0, 0, 0, nullptr, nullptr},
    {"exact_cand", OPT_FIELD(exact_cand), Option::range, 2, CMR_MAX_K, 0, "exact_cand must be in [2, " CMR_STR(CMR_MAX_K) "]", OPT_READ(i->exact_cand)},
    {"combine", [](cmr_index* i, long long v) { i->combine.store((int)v, std::memory_order_relaxed); }, Option::zero_or, 2, cmr_combine::kMaxWidth, 0,
     "combine must be 0 (off) or in [2, " CMR_STR(CMR_PPR_MAX_BATCH) "]", OPT_READ(i->combine.load(std::memory_order_relaxed))},
    {"combine_wait_us", [](cmr_index* i, long long v) { i->combine_wait_us.store(v, std::memory_order_relaxed); }, Option::clamp, 0, 10000000, 0, nullptr,
     OPT_READ(i->combine_wait_us.load(std::memory_order_relaxed))},
    {"combine_filtered", [](cmr_index* i, long long v) { i->combine_filtered.store((int)v, std::memory_order_relaxed); }, Option::range, 0, 1, 0,
     "combine_filtered must be 0 or 1", OPT_READ(i->combine_filtered.load(std::memory_order_relaxed))},
    {"prefilter", OPT_FIELD(prefilter), Option::range, -1, 2, 0, "prefilter must be -1 (auto), 0 (off), 1 (on) or 2 (on, the filter keeps every row)", OPT_READ(i->prefilter)},
    {"prefilter_rescore_wgs", OPT_FIELD(pf_rescore_wgs), Option::clamp, 0, 1024, 0, nullptr, nullptr},
    {"prefilter_tighten", OPT_FIELD(pf_tighten), Option::range, 0, 1, 0, "prefilter_tighten must be 0 or 1", OPT_READ(i->pf_tighten)},
    {"prefilter_pair_cap", OPT_FIELD(pf_pair_cap), Option::clamp, 0, 1 << 20, 0, nullptr, OPT_READ(i->pf_pair_cap)},
    {"prefilter_wave_cap", OPT_FIELD(pf_wave_cap), Option::clamp, 0, 1 << 20, 0, nullptr, OPT_READ(i->pf_wave_cap)},
    {"prefilter_sample", OPT_FIELD(pf_sample), Option::range, -1, 1, 0, "prefilter_sample must be -1 (auto), 0 (bf16 sampling) or 1 (int8 sample)", OPT_READ(i->pf_sample)},
    {"prefilter_sample_panels", OPT_FIELD(pf_sample_panels), Option::clamp, 0, INT_MAX, 0, nullptr, OPT_READ(i->pf_sample_panels)},
    {"prefilter_sample_run", OPT_FIELD(pf_sample_run), Option::clamp, 0, 1 << 16, 0, nullptr, OPT_READ(i->pf_sample_run)},
    {"prefilter_sample_wave_cap", OPT_FIELD(pf_sample_wave_cap), Option::clamp, 0, 1 << 20, 0, nullptr, OPT_READ(i->pf_sample_wave_cap)},
    {"prefilter_sample_level0", OPT_FIELD(pf_sample_level0), Option::clamp, 0, 128, 0, nullptr, OPT_READ(i->pf_sample_level0)},
    {"prefilter_sample_active", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->prefilter_sample_active)},
    {"prefilter_sample_pairs", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(q8_read_counter(i, Q8Counter::sample_pairs))},
    {"prefilter_sample_overflow", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(q8_read_counter(i, Q8Counter::sample_overflow))},
    {"prefilter_active", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->prefilter_active)},
    {"prefilter_rows", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->q8c.q8 ? i->q8c.rows : 0)},
    {"prefilter_bytes", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ((long long)i->q8c.bytes(i->dpad))},
    {"prefilter_candidates", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(q8_read_counter(i, Q8Counter::candidates))},
    {"prefilter_pairs", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(q8_read_counter(i, Q8Counter::pairs))},
    {"prefilter_pair_overflow", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(q8_read_counter(i, Q8Counter::pair_overflow))},
    {"prefilter_wave_overflow", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(q8_read_counter(i, Q8Counter::wave_overflow))},
    {"remove_stage_panels", [](cmr_index* i, long long v) { i->rm_stage_panels = v <= 0 ? 0 : (int)std::max(2ll, v); }, Option::clamp, 0, 1 << 22, 0, nullptr,
     OPT_READ(i->rm_stage_panels)},
    {"remove_chunks_last", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->rm_chunks_last)},
    {"update_stage_rows", [](cmr_index* i, long long v) { i->upd_stage_rows = v <= 0 ? 0 : v; }, Option::clamp, 0, 1ll << 40, 0, nullptr, OPT_READ(i->upd_stage_rows)},
    {"update_chunks_last", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->upd_chunks_last)},
    {"range_block_queries", OPT_FIELD(range_block_queries), Option::clamp, 0, INT_MAX, 0, nullptr, OPT_READ(i->range_block_queries)},
    {"range_scratch_hits", OPT_FIELD(range_scratch_hits), Option::clamp, 0, 1ll << 31, 0, nullptr, OPT_READ(i->range_scratch_hits)},
    {"range_blocks_last", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->range_blocks_last.load(std::memory_order_relaxed))},
    {"range_groups_last", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->range_groups_last.load(std::memory_order_relaxed))},
    {"last_route", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->last_route.load(std::memory_order_relaxed))},
    {"pipe_dual_scan_active", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->dual_active)},
    {"pipe_dual_scan_wide_active", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->dual_wide_active)},
    {"pipe_cu_mask_active", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->pipe.last_masked)},
    {"pipe_scan_cus", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->pipe.last_masked ? i->pipe.scan_cus : i->n_cu)},
    {"combine_batches", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->combiner.batches())},
    {"combine_queries", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->combiner.queries())},
    {"combine_max_width", nullptr, Option::any, 0, 0, 0, nullptr, OPT_READ(i->combiner.max_width())},
};
#undef OPT_FIELD
#undef OPT_READ

const Option* find_option(const char* name) {
    for (const Option& o : kOptions) if (strcmp(o.name, name) == 0) return &o;
    return nullptr;
}

int set_option(cmr_index* idx, const char* name, long long v) {
    const Option* o = find_option(name ? name : "");
    if (!o || !o->store) return fail(CMR_ERR_INVALID, "unknown option '%s'", name ? name : "");
    const bool refused = o->kind == Option::oneof ? (v != o->a && v != o->b && v != o->c) : o->kind == Option::range ? (v < o->a || v > o->b) : o->kind == Option::zero_or ? (v != 0 && (v < o->a || v > o->b)) : false;
    if (refused) return fail(CMR_ERR_INVALID, "%s", o->reject);
    if (o->kind == Option::clamp) v = std::max(o->a, std::min(v, o->b));
    o->store(idx, v);
    return CMR_OK;
}

// shard-local ids -> global ids, on the stream that produced them (no-op for a single block)
int remap_ids_enqueue(cmr_index* idx, int64_t* ids_dev, long long n, hipStream_t s);
// global id -> shard-local row, -1 when this shard does not hold it
long long to_local_row(const cmr_index* idx, long long gid) {
    if (gid < 0) return -1;
    if (idx->single_block()) { const long long r = gid - idx->id_base; return (r >= 0 && r < idx->n) ? r : -1; }
    const size_t nb = idx->blk_local.size();
    size_t b = std::upper_bound(idx->blk_global.begin(), idx->blk_global.end(), gid) - idx->blk_global.begin();
    if (b == 0) return -1;
    --b;
    const long long len = (b + 1 < nb ? idx->blk_local[b + 1] : idx->n) - idx->blk_local[b];
    const long long off = gid - idx->blk_global[b];
    return off < len ? idx->blk_local[b] + off : -1;
}

// would appending n rows push the last block's global ids past what the packed exchange can carry?
bool global_id_overflow(const cmr_index* idx, long long n) {
    const long long l0 = idx->blk_local.size() > 1 ? idx->blk_local.back() : 0;
    const long long g0 = idx->blk_local.size() > 1 ? idx->blk_global.back() : idx->id_base;
    return g0 + (idx->n + n - l0) - 1 > 0xFFFFFFFEll;
}

}  // namespace

int cmr_check_device(int device_id) {
    static std::mutex mu;
    static std::vector<char> ok;                  // devices already validated (hipGetDeviceProperties is slow)
    {
        std::lock_guard<std::mutex> g(mu);
        if (device_id >= 0 && (size_t)device_id < ok.size() && ok[device_id]) return CMR_OK;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(CMR_ERR_NO_DEVICE, "no HIP device visible (%s); libcomorag_hip has no CPU fallback",
                                               e == hipSuccess ? "count 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(CMR_ERR_NO_DEVICE, "device_id %d out of range [0,%d)", device_id, n);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(CMR_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", device_id, prop.gcnArchName);
    {
        std::lock_guard<std::mutex> g(mu);
        if (ok.size() <= (size_t)device_id) ok.resize((size_t)device_id + 1, 0);
        ok[device_id] = 1;
    }
    return CMR_OK;
}

namespace {

// Synchronous host API, results in the workspace's pinned, device-mapped buffer: the search's last kernel stores a word (bytes 4..7 of the
// buffer, zeroed by the caller before the launch) behind its results — both by system-scope stores, the device's writes arrive in order —
// and the host polls it: seen ~5.5 us before hipStreamSynchronize returns (tools/probe/poll_probe.hip).  Bounded: a launch that never
// reports (a fault) is left to the stream, whose error comes back.
int wait_done_word(Workspace* ws, int* state = nullptr) {
    volatile int* const w = (volatile int*)((char*)ws->h_pin + 4);
    int st = *w;
    if (!st) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spin = 1; !(st = *w); ++spin) {
            __builtin_ia32_pause();
            if ((spin & 4095u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) break;
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    if (!st) { HIP_TRY(hipStreamSynchronize(ws->stream)); st = *w; }
    if (state) *state = st;
    return CMR_OK;
}

// the workspace's non-finite flag, allocated and zeroed on first use
int arm_flag(Workspace* ws, hipStream_t s) {
    if (ws->flag_ptr) return CMR_OK;
    HIP_TRY(ws->flag.ensure(sizeof(int)));
    HIP_TRY(hipMemsetAsync(ws->flag.p, 0, sizeof(int), s));
    ws->flag_ptr = (int*)ws->flag.p;
    return CMR_OK;
}

int remap_ids_enqueue(cmr_index* idx, int64_t* ids_dev, long long n, hipStream_t s) {
    if (idx->single_block()) return CMR_OK;
    HIP_TRY(cmr_launch_remap_ids(ids_dev, n, idx->d_blk, (int)idx->blk_local.size(), s));
    return CMR_OK;
}

// Enqueue a full search (all passes) on ws->stream.  Device pointers in, device pointers out.
int scores_enqueue(cmr_index* idx, Workspace* ws, const float* q_dev, int nq, float* out_dev, long long ld);

// k above CMR_MAX_K (retrieve_knn's synonymy_edge_topk = 2047): materialise the scores of a block of
// queries on the device, then select per row (radix select + ordered compaction + bitonic sort).
int search_large_k_enqueue(cmr_index* idx, Workspace* ws, const float* q_dev, int nq, int k, int64_t* ids_dev,
                           float* scores_dev, float* min_dev, float* max_dev) {
    hipStream_t s = ws->stream;
    const long long n = idx->n;
    const long long ld = (n + 3) / 4 * 4;
    const int blockq = (int)std::max<long long>(1, std::min<long long>(nq, (1ll << 31) / std::max<long long>(ld * 4, 1)));  // <= 2 GiB
    HIP_TRY(ws->d_out.ensure((size_t)blockq * ld * 4));
    for (int q0 = 0; q0 < nq; q0 += blockq) {
        const int nb = std::min(blockq, nq - q0);
        int rc = scores_enqueue(idx, ws, q_dev + (size_t)q0 * idx->dim, nb, (float*)ws->d_out.p, ld);
        if (rc) return rc;
        idx->last_route.store(route_code(CMR_ROUTE_LARGE_K), std::memory_order_relaxed);
        HIP_TRY(cmr_launch_topk_rows((const float*)ws->d_out.p, ld, (int)n, nb, k, kernel_id_base(idx), ids_dev + (size_t)q0 * k,
                                     scores_dev + (size_t)q0 * k, min_dev ? min_dev + q0 : nullptr,
                                     max_dev ? max_dev + q0 : nullptr, s));
    }
    return remap_ids_enqueue(idx, ids_dev, (long long)nq * k, s);
}

// The streams and events of one pass.  The pre-phase (query packing + sampling levels) goes to `sp`, the main scan to `sm`, the
// candidate merge to `sq`; where they differ (pipelined mode) the events order them, so the pre-phase of the NEXT pass/batch
// can overlap this pass's main scan.  A synchronous caller passes one stream three times and no events.
struct PassStreams {
    hipStream_t sp, sm, sq;
    hipEvent_t ev_pre, ev_scan, ev_lists_free;      // ev_lists_free: the previous merge of this workspace's lists (nullptr: none)
    static PassStreams one(hipStream_t s) { return {s, s, s, nullptr, nullptr, nullptr}; }
    PassRequest request(int nqp, int k, Route route, bool has_min_score, int reserve_cus) const {
        PassRequest rq;
        rq.nqp = nqp; rq.k = k; rq.route = route; rq.has_min_score = has_min_score;
        rq.single_stream = sp == sm && sm == sq; rq.pipelined = sp != sm; rq.reserve_cus = reserve_cus;
        return rq;
    }
};

// One pass (<= 64 queries, or one wide / query-split pass) of the fused search, as plan_pass shaped it (search_plan.h): this
// function only allocates, launches, records and waits.
// row_mask: the allow words of a filtered pass (p.masked; device, one word per panel) — its sampling levels and its main scan are the masked variant
// mask_stride: p.masked_each — row_mask holds a block of mask_stride words for each of the pass's nqp queries, the first query's first
int enqueue_pass(cmr_index* idx, Workspace* ws, const PassStreams& st, const PassPlan& p, const float* q_dev, const float* min_score,
                 int64_t* ids_dev, float* scores_dev, float* min_dev, float* max_dev, const unsigned* row_mask = nullptr, long long mask_stride = 0) {
    hipStream_t const sp = st.sp, sm = st.sm, sq = st.sq;
    const CmrScanGeom& g = p.g;
    const int nqp = p.nqp, k = p.k, G = p.G;
    int rc = arm_flag(ws, sp);   // zeroed once; the reader re-arms it after reporting
    if (rc) return rc;
    HIP_TRY(ws->qfrag.ensure(p.bytes.qfrag));
    HIP_TRY(ws->lists.ensure(p.bytes.lists));
    HIP_TRY(ws->cnt.ensure(p.bytes.cnt));
    HIP_TRY(ws->mm.ensure(p.bytes.mm));
    if (p.Ws) {
        HIP_TRY(ws->s_lists.ensure(p.bytes.s_lists));
        HIP_TRY(ws->s_cnt.ensure(p.bytes.s_cnt));
        HIP_TRY(ws->s_mm.ensure(p.bytes.s_mm));
    }
    HIP_TRY(ws->tau.ensure(p.bytes.tau));
    // the re-score of the workspace's previous pass reads the query fragments and thresholds on the merge stream
    if (ws->q8.pf_prev && sp != sm && st.ev_lists_free) HIP_TRY(hipStreamWaitEvent(sp, st.ev_lists_free, 0));
    ws->q8.pf_prev = p.prefilter != 0;
    HIP_TRY(cmr_launch_prep_queries(idx->dtype, q_dev, nqp, idx->dim, idx->dpad, p.tiles, ws->qfrag.p, ws->flag_ptr, sp));
    CmrQ8Args f{};      // the pre-filter's launches (prefilter_host.h), where the plan takes that route
    if (p.prefilter && (rc = q8_prepare(idx, ws, p, q_dev, sp, f))) return rc;
    CmrScanArgs a{};
    a.corpus = idx->corpus; a.qfrag = ws->qfrag.p; a.nrows = idx->n; a.npanels = (int)idx->npanels(); a.k = k;
    a.nq = nqp;
    a.qgroups = G;
    if (p.masked) {
        if (!row_mask) return fail(CMR_ERR_INVALID, "filtered pass without allow words");
        a.row_mask = row_mask;
        if (p.masked_each) {
            if (mask_stride < idx->npanels()) return fail(CMR_ERR_INVALID, "per-query allow words: stride %lld < %lld panels", mask_stride, idx->npanels());
            a.row_mask_stride = mask_stride;
        }
    }
    if (min_score) {
        // key > tau  <=>  score >= *min_score: tau = (smallest key with that score) - 1
        HIP_TRY(cmr_launch_fill_threshold(*min_score, p.NQA, (u64*)ws->tau.p, sp));
        a.tau_init = (u64*)ws->tau.p;
    }
    for (int lv = 0; lv < p.n_levels; ++lv) {
        const PassPlan::Level& L = p.level[lv];
        CmrScanGeom gs = g;
        gs.grid = L.grid;
        CmrScanArgs as = a;
        as.lists = (u64*)ws->s_lists.p; as.cnt = (int*)ws->s_cnt.p; as.mm = (float2*)ws->s_mm.p;
        as.sample_waves = (int)L.panels; as.sample_chunk_log2 = L.clog; as.sample_stride = L.stride;
        u64* tau_out = (u64*)ws->tau.p + (size_t)(lv & 1) * p.NQA;
        if (lv == 1 && p.sample_q8) {      // level 1 from the int8 companion: filter in sample mode, bucket, select (prefilter_host.h)
            if ((rc = q8_sample(idx, f, a.tau_init, tau_out, p.bytes.q8[Q8_SPAIRCNT], sp))) return rc;
            a.tau_init = tau_out;
            continue;
        }
        HIP_TRY(p.wide ? cmr_launch_scan_wide(gs, as, sp) : p.masked_each ? cmr_launch_scan_masked_each(gs, as, sp) : p.masked ? cmr_launch_scan_masked(gs, as, sp) : cmr_launch_scan_topk(gs, as, sp));
        if (p.tau_in_scan) {      // the main scan's workgroups derive the thresholds from these lists themselves
            a.sample_lists = (const u64*)ws->s_lists.p; a.sample_cnt = (const int*)ws->s_cnt.p; a.sample_W = L.Wl;
            a.tau_init = nullptr;
            continue;
        }
        HIP_TRY(cmr_launch_merge_query((const u64*)ws->s_lists.p, (const int*)ws->s_cnt.p, L.Wl, p.NQ, g.cap, nqp, k, nullptr, 0, nullptr,
                                       nullptr, nullptr, nullptr, tau_out, sp, G > 1));
        a.tau_init = tau_out;
    }
    if (sp != sm && st.ev_lists_free) HIP_TRY(hipStreamWaitEvent(sp, st.ev_lists_free, 0));   // previous merge of this slot's lists
    if (p.prefilter) HIP_TRY(hipMemsetAsync(f.pair_cnt, 0, p.bytes.q8[Q8_PAIRCNT], sp));   // (behind that wait: the previous tightening read the counters and the pairs)
    if (sp != sm) {
        HIP_TRY(hipEventRecord(st.ev_pre, sp));
        HIP_TRY(hipStreamWaitEvent(sm, st.ev_pre, 0));
    }
    a.lists = (u64*)ws->lists.p; a.cnt = (int*)ws->cnt.p; a.mm = (float2*)ws->mm.p;
    ProfEvent pe{};
    bool prof = false;
    {
        std::lock_guard<std::mutex> pg(idx->prof_mu);
        prof = idx->prof_on && (idx->prof_seq++ % (unsigned)idx->prof_every) == 0;
    }
    if (prof) {
        HIP_TRY(hipEventCreate(&pe.a));
        HIP_TRY(hipEventCreate(&pe.b));
        HIP_TRY(hipEventRecord(pe.a, sm));
    }
    const int* fin_state = nullptr;
    if (p.fin) {
        if (!ws->fin_ctl_armed) {               // zeroed once; the kernel's last workgroup re-arms the words
            HIP_TRY(ws->fin_ctl.ensure(p.bytes.fin_ctl));
            HIP_TRY(hipMemsetAsync(ws->fin_ctl.p, 0, p.bytes.fin_ctl, sm));
            ws->fin_ctl_armed = true;           // (only once the zeroing is in the stream: garbage counters would end in garbage results)
        }
        HIP_TRY(ws->fin_pmax.ensure(p.bytes.fin_pmax));
        HIP_TRY(ws->fin_tau.ensure(p.bytes.fin_tau));
        HIP_TRY(ws->fin_mm.ensure(p.bytes.fin_mm));
        a.fin_mm = (u64*)ws->fin_mm.p;
        HIP_TRY(ws->fin_dense.ensure(p.bytes.fin_dense));
        a.fin = (int*)ws->fin_ctl.p; a.fin_pmax = (u64*)ws->fin_pmax.p; a.fin_tau = (u64*)ws->fin_tau.p; a.fin_dense = (u64*)ws->fin_dense.p;
        a.fin_first = p.fin_first; a.fin_wgs = p.fin_wgs; a.fin_mul = p.fin_mul; a.fin_dcap = p.fin_dcap; a.fin_spin = p.fin_spin;
        a.out_ids = ids_dev; a.out_scores = scores_dev; a.out_min = min_dev; a.out_max = max_dev; a.id_base = kernel_id_base(idx);
        fin_state = (const int*)ws->fin_ctl.p + CMR_FIN_STATE;
        // the synchronous host API (results in its mapped buffer, nothing to remap behind the scan): the kernel reports its state in the
        // caller's done word and the merge launch — which would return in its first instruction on state 1 — is issued only on state 2
        if (ws->done_ptr && idx->single_block()) a.fin_done = ws->done_ptr;
    }
    if (p.prefilter) { if ((rc = q8_filter(idx, f, a, sm))) return rc; }
    else HIP_TRY(p.wide ? cmr_launch_scan_wide(g, a, sm) : p.fin ? cmr_launch_scan_fin(g, a, sm) : p.masked_each ? cmr_launch_scan_masked_each(g, a, sm) : p.masked ? cmr_launch_scan_masked(g, a, sm) : cmr_launch_scan_topk(g, a, sm));
    if (prof) {
        HIP_TRY(hipEventRecord(pe.b, sm));
        std::lock_guard<std::mutex> pg(idx->prof_mu);
        idx->prof_events.push_back(pe);
        idx->prof_bytes = p.prefilter ? prefilter_bytes(idx, p) : algorithmic_bytes(idx, nqp, k);
    }
    if (a.fin_done) {
        ws->lazy.due = true;
        ws->lazy.lists = (const u64*)ws->lists.p; ws->lazy.cnt = (const int*)ws->cnt.p; ws->lazy.W = p.W; ws->lazy.NQ = p.NQ; ws->lazy.cap = g.cap; ws->lazy.nqp = nqp; ws->lazy.k = k;
        ws->lazy.mm = (const float2*)ws->mm.p; ws->lazy.id_base = kernel_id_base(idx); ws->lazy.ids = ids_dev; ws->lazy.scores = scores_dev; ws->lazy.mn = min_dev; ws->lazy.mx = max_dev;
        ws->lazy.state = fin_state;
        ws->done_used = true;
        return CMR_OK;
    }
    if (sq != sm) {   // pipelined: the candidate merge leaves the scan stream so the next main scan starts at once
        HIP_TRY(hipEventRecord(st.ev_scan, sm));
        HIP_TRY(hipStreamWaitEvent(sq, st.ev_scan, 0));
    }
    if (p.prefilter && (rc = q8_rescore(f, sq))) return rc;
    HIP_TRY(cmr_launch_merge_query((const u64*)ws->lists.p, (const int*)ws->cnt.p, p.W, p.NQ, g.cap, nqp, k, (const float2*)ws->mm.p,
                                   kernel_id_base(idx), ids_dev, scores_dev, min_dev, max_dev, nullptr, sq, G > 1, fin_state));
    return remap_ids_enqueue(idx, ids_dev, (long long)nqp * k, sq);
}

// plan one pass and enqueue it
int plan_and_enqueue_pass(cmr_index* idx, Workspace* ws, const PassStreams& st, const PassSplit& ps, int k, int reserve_cus, const float* q_dev,
                          const float* min_score, int64_t* ids_dev, float* scores_dev, float* min_dev, float* max_dev, int prefilter = 0) {
    PassPlan plan;
    PassRequest rq = st.request(ps.nqp, k, ps.route, min_score != nullptr, reserve_cus);
    rq.prefilter = prefilter;
    int rc = plan_pass(idx, rq, &plan);
    if (rc) return rc;
    if (ps.q0 == 0)      // (a batch of several passes: its first, and the bit that says more follow)
        idx->last_route.store(route_code(plan, min_score != nullptr) | (ps.nqp < ps.nq ? CMR_ROUTE_MORE_PASSES : 0), std::memory_order_relaxed);
    return enqueue_pass(idx, ws, st, plan, q_dev + (size_t)ps.q0 * idx->dim, min_score, ids_dev + (size_t)ps.q0 * k, scores_dev + (size_t)ps.q0 * k,
                        min_dev ? min_dev + ps.q0 : nullptr, max_dev ? max_dev + ps.q0 : nullptr);
}

int search_enqueue(cmr_index* idx, Workspace* ws, const float* q_dev, int nq, int k, int64_t* ids_dev, float* scores_dev,
                   float* min_dev, float* max_dev, const float* min_score = nullptr) {
    if (k > CMR_MAX_K) {
        if (min_score) return fail(CMR_ERR_UNSUPPORTED, "threshold search supports k <= %d", CMR_MAX_K);
        return search_large_k_enqueue(idx, ws, q_dev, nq, k, ids_dev, scores_dev, min_dev, max_dev);
    }
    if (const int kind = small_path_kind(idx, nq, k, min_score != nullptr)) {   // small corpus, few queries: ONE launch does packing, scan, selection and min/max
        const long long npanels = idx->npanels();
        idx->last_route.store(route_code(kind == 1 ? CMR_ROUTE_TINY : CMR_ROUTE_SMALL), std::memory_order_relaxed);
        { int rc_ = arm_flag(ws, ws->stream); if (rc_) return rc_; }
        HIP_TRY(ws->d_out.ensure(cmr_tiny_scratch_bytes(nq, (int)npanels, k, idx->tiny_multi, idx->small_max_panels)));
        if (!ws->arrive.p) {          // arrival counter of the multi-workgroup search: zeroed once, re-armed by the kernel
            HIP_TRY(ws->arrive.ensure(sizeof(int)));
            HIP_TRY(hipMemsetAsync(ws->arrive.p, 0, sizeof(int), ws->stream));
        }
        HIP_TRY(cmr_launch_tiny_search(idx->dtype, idx->corpus, q_dev, nq, idx->dim, idx->dpad, idx->n, k, kernel_id_base(idx), ws->d_out.p,
                                       ids_dev, scores_dev, min_dev, max_dev, ws->flag_ptr, idx->tiny_multi ? (int*)ws->arrive.p : nullptr, idx->small_max_panels, ws->stream,
                                       (ws->done_ptr && idx->single_block()) ? ws->done_ptr : nullptr));
        if (ws->done_ptr && idx->single_block()) ws->done_used = true;
        return remap_ids_enqueue(idx, ids_dev, (long long)nq * k, ws->stream);
    }
    const PassStreams st = PassStreams::one(ws->stream);
    for (PassSplit ps(idx, nq); ps.next();) {
        int rc = plan_and_enqueue_pass(idx, ws, st, ps, k, 0, q_dev, min_score, ids_dev, scores_dev, min_dev, max_dev);
        if (rc) return rc;
    }
    return CMR_OK;
}

// Streams and per-slot events of the pipelined search, created on first use (idx->pipe_mu held).  Everything is built into
// locals and committed to idx->pipe only when ALL of it exists: a failure half way leaves the index without a pipeline (the next
// call tries again), never with a half-built one that a later call would take for complete.  A device / driver that refuses
// CU-masked streams gets plain streams (the masks buy time, not results).
int create_pipe_streams(cmr_index* idx, Pipe& T, int mask, bool dual) {
    HIP_TRY(hipStreamCreateWithFlags(&T.st[Pipe::sq], hipStreamNonBlocking));
    if (mask) {
        // wide batches: the matrix-pipe-bound kernel wants CUs — n_cu - 32 for its scans (28 per XCD), the 32 it used to leave
        // free by trimming its grid for the pre-phase; two scan streams for short scans as below
        uint32_t wscan[8], wrest[8];
        for (int w = 0; w < 8; ++w) {
            wscan[w] = mask == 2 ? 0x0FFFFFFFu : (w < 7 ? 0xFFFFFFFFu : 0u);
            wrest[w] = ~wscan[w];
        }
        HIP_TRY(hipExtStreamCreateWithCUMask(&T.st[Pipe::wm], 8, wscan));
        if (dual) HIP_TRY(hipExtStreamCreateWithCUMask(&T.st[Pipe::wm2], 8, wscan));
        HIP_TRY(hipExtStreamCreateWithCUMask(&T.st[Pipe::wp], 8, wrest));
        T.wide_cus = idx->n_cu - 32;
        // Scans of the narrow kernel on n_cu - 64 CUs, their pre-phases on the other 64: the reservation that trimming the
        // grid only approximates, made explicit — and the precondition for TWO scan streams: the next scan's workgroups then
        // start on whatever CU of the scan set falls free (no idle gap, the tail of one scan under the ramp of the next),
        // never on the pre-phase's CUs.  Measured (profiles/r3_pipe_cu_mask_dual_scan.txt): 1 M rows 0.270 -> 0.250 ms per
        // step, 1.25 M 0.334 -> 0.308, 10 M 2.396 -> 2.331; masks alone <= 2 %, two streams without masks slower.
        // Mask bit i is CU i of the driver's enumeration, which interleaves the XCDs: the first 192 bits are 24 CUs of each.
        uint32_t scan[8], rest[8];
        for (int w = 0; w < 8; ++w) {
            scan[w] = mask == 2 ? 0x00FFFFFFu : (w < 6 ? 0xFFFFFFFFu : 0u);      // 2: 24 of every 32 bits (same split if 32 consecutive bits were one XCD)
            rest[w] = ~scan[w];
        }
        HIP_TRY(hipExtStreamCreateWithCUMask(&T.st[Pipe::sm], 8, scan));
        if (dual) HIP_TRY(hipExtStreamCreateWithCUMask(&T.st[Pipe::sm2], 8, scan));
        HIP_TRY(hipExtStreamCreateWithCUMask(&T.st[Pipe::sp], 8, rest));
        T.scan_cus = idx->n_cu - 64;
        for (Pipe::Stream u : {Pipe::usp, Pipe::usm, Pipe::uwp, Pipe::uwm}) HIP_TRY(hipStreamCreateWithFlags(&T.st[u], hipStreamNonBlocking));
    } else {
        HIP_TRY(hipStreamCreateWithFlags(&T.st[Pipe::wp], hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&T.st[Pipe::wm], hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&T.st[Pipe::sp], hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&T.st[Pipe::sm], hipStreamNonBlocking));
        if (dual) HIP_TRY(hipStreamCreateWithFlags(&T.st[Pipe::sm2], hipStreamNonBlocking));
    }
    return CMR_OK;
}
int ensure_pipe(cmr_index* idx) {
    Pipe& P = idx->pipe;
    if (P.st[Pipe::sq]) return CMR_OK;
    int mask = idx->cu_mask < 0 ? (idx->n_cu == 256 ? 1 : 0) : (idx->n_cu == 256 ? idx->cu_mask : 0);
    hipEvent_t ev[CMR_PIPE_SLOTS][3] = {};
    Pipe T;
    auto undo = [&]() {
        T.destroy_streams();
        for (auto& slot : ev) for (hipEvent_t& e : slot) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        T.scan_cus = T.wide_cus = 0;
    };
    int rc = create_pipe_streams(idx, T, mask, idx->dual_scan < 0 ? mask != 0 : idx->dual_scan != 0);
    if (rc && mask) {                     // no CU-masked streams here: plain ones
        undo();
        mask = 0;
        rc = create_pipe_streams(idx, T, 0, idx->dual_scan > 0);
    }
    if (rc) { undo(); return rc; }
    auto make_events = [&]() -> int {
        for (auto& slot : ev) for (hipEvent_t& e : slot) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return CMR_OK;
    };
    rc = make_events();
    if (rc) { undo(); return rc; }
    // commit (slots keep their workspaces: none exists before the first pipelined call)
    for (int i = 0; i < Pipe::n_streams; ++i) if (i != Pipe::sq) P.st[i] = T.st[i];
    P.scan_cus = T.scan_cus; P.wide_cus = T.wide_cus;
    for (int i = 0; i < CMR_PIPE_SLOTS; ++i) {
        P.slot[i].pre_done = ev[i][0]; P.slot[i].main_done = ev[i][1]; P.slot[i].scan_done = ev[i][2];
        P.slot[i].ws.stream = P.st[Pipe::sm];
    }
    P.st[Pipe::sq] = T.st[Pipe::sq];      // the "pipeline exists" marker: last
    return CMR_OK;
}

// Pipelined search: three internal streams.  Pre-phases run on `sp` back to back, candidate merges
// on `sq`; main scans are serialised on `sm` (two HBM-bound scans at once only slow each other down) and leave
// `reserve_cus` CUs free, on which the next pass's sampling scans and the merges run concurrently.
int search_pipelined_enqueue_locked(cmr_index* idx, const float* q_dev, int nq, int k, int64_t* ids_dev, float* scores_dev, float* min_dev,
                                    float* max_dev, hipEvent_t wait_event, hipEvent_t* done_event, const float* min_score, bool may_prefilter = false) {
    Pipe& P = idx->pipe;
    { int rc_ = ensure_pipe(idx); if (rc_) return rc_; }
    P.nslots = std::min(CMR_PIPE_SLOTS, std::max(2, idx->pipe_slots));
    if (k > CMR_MAX_K) return fail(CMR_ERR_UNSUPPORTED, "pipelined search supports k <= %d", CMR_MAX_K);
    // Scans shorter than 1 ms at the streaming rate (shards up to ~4 M x 768 bf16 rows) run on the CU-masked streams — and
    // alternate between two of them; longer ones on the unmasked twins with the trimmed grid: in bench.py's flow the masks cost
    // the 10 M-row scans CUs (same-box A/B: B = 64 step 2.441 vs 2.396 ms, B = 256 4.444 vs 4.069) where they bought the
    // short ones 7-8 %.  pipe_cu_mask = 1 | 2 forces the masks for every scan, 0 creates none.
    const bool masked = P.scan_cus != 0 && (idx->cu_mask > 0 || idx->short_scan());
    const bool twins = P.scan_cus != 0 && !masked;      // masked streams exist but this call's scans use the unmasked ones
    P.last_masked = masked ? 1 : 0;
    hipStream_t const nsp = P.st[twins ? Pipe::usp : Pipe::sp], wsp = P.st[twins ? Pipe::uwp : Pipe::wp];
    PassSplit ps(idx, nq);
    if (wait_event) {      // inputs ready: both pre-phase streams may read them
        HIP_TRY(hipStreamWaitEvent(nsp, wait_event, 0));
        if (ps.any_wide()) HIP_TRY(hipStreamWaitEvent(wsp, wait_event, 0));
    }
    // Certified int8 pre-filter (prefilter_host.h): the companion is brought up to date in front of the call's pre-phase
    int prefilter = prefilter_eligible(idx, min_score != nullptr, min_dev || max_dev, nq, may_prefilter);
    if (prefilter && !q8_ensure_companion(idx, nsp)) prefilter = 0;
    idx->prefilter_active = 0;
    idx->prefilter_sample_active = 0;
    PipeSlot* last = nullptr;
    while (ps.next()) {
        const bool wide = ps.wide_streams();
        PipeSlot* sl = &P.slot[P.next++ % (unsigned)P.nslots];
        hipStream_t sp = wide ? wsp : nsp;
        if (sl->used) {
            // The pre-phase rewrites the slot's query fragments / thresholds: free once the slot's previous
            // main scan is over.  Its candidate lists are still being merged (on sq) at that point, so only the
            // new MAIN scan waits for that merge — a full scan period later, i.e. never in practice; that wait
            // sits at the END of the pre-phase (enqueue_pass, before pre_done is recorded): every wait packet on
            // the scan stream itself costs ~10 us between two main scans.
            HIP_TRY(hipStreamWaitEvent(sp, sl->scan_done, 0));
        }
        // Two scan streams for the narrow kernel: consecutive main scans are not ordered by a stream any more — the second
        // one's workgroups start as the first one's retire.  A slot's own scans stay ordered through its events (pre-phase ->
        // scan -> merge -> next pre-phase), and nothing else is shared between two batches.
        // Only short scans (< 1 ms at the streaming rate: shards up to ~4 M x 768 bf16 rows) alternate: there the ramp / tail /
        // packet gap is 7-8 % of a step (1 M rows 0.270 -> 0.250 ms), at 10 M rows 2.7 % — and overlapping launches have no
        // per-launch duration any more (a kernel's begin-to-end then includes the wait for the previous scan's CUs), which
        // is what the roofline of the long headline scan is measured with.
        const bool dual = !twins && P.st[wide ? Pipe::wm2 : Pipe::sm2] != nullptr && (idx->dual_scan > 0 || idx->short_scan());
        if (!wide) idx->dual_active = dual ? 1 : 0;
        else idx->dual_wide_active = dual ? 1 : 0;
        hipStream_t sm = P.st[twins ? (wide ? Pipe::uwm : Pipe::usm)
                                    : wide ? ((dual && (P.nwscan++ & 1)) ? Pipe::wm2 : Pipe::wm) : ((dual && (P.nscan++ & 1)) ? Pipe::sm2 : Pipe::sm)];
        const PassStreams st{sp, sm, P.st[Pipe::sq], sl->pre_done, sl->scan_done, sl->used ? sl->main_done : nullptr};
        int rc = plan_and_enqueue_pass(idx, &sl->ws, st, ps, k, (masked && !wide) ? idx->n_cu - P.scan_cus : (masked && wide) ? idx->n_cu - P.wide_cus : idx->reserve_cus,
                                       q_dev, min_score, ids_dev, scores_dev, min_dev, max_dev, wide ? 0 : prefilter);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(sl->main_done, P.st[Pipe::sq]));
        sl->used = true;
        last = sl;
    }
    if (done_event) *done_event = last ? last->main_done : nullptr;
    return CMR_OK;
}
int search_pipelined_enqueue(cmr_index* idx, const float* q_dev, int nq, int k, int64_t* ids_dev, float* scores_dev, float* min_dev,
                             float* max_dev, hipEvent_t wait_event, hipEvent_t* done_event, const float* min_score = nullptr, bool may_prefilter = false) {
    std::lock_guard<std::mutex> pl(idx->pipe_mu);
    return search_pipelined_enqueue_locked(idx, q_dev, nq, k, ids_dev, scores_dev, min_dev, max_dev, wait_event, done_event, min_score, may_prefilter);
}

int scores_enqueue(cmr_index* idx, Workspace* ws, const float* q_dev, int nq, float* out_dev, long long ld) {
    hipStream_t s = ws->stream;
    CmrScanGeom g{};
    const int per_pass = idx->narrow_width(nq);
    const long long npanels = idx->npanels();
    { int rc_ = arm_flag(ws, s); if (rc_) return rc_; }
    for (int q0 = 0; q0 < nq; q0 += per_pass) {
        const int nqp = std::min(per_pass, nq - q0);
        int rc = make_geom(idx, nqp, 1, false, &g);
        if (rc) return rc;
        HIP_TRY(ws->qfrag.ensure((size_t)g.nqt * g.ks * 1024));
        HIP_TRY(cmr_launch_prep_queries(idx->dtype, q_dev + (size_t)q0 * idx->dim, nqp, idx->dim, idx->dpad, g.nqt, ws->qfrag.p,
                                        ws->flag_ptr, s));
        CmrScanArgs a{};
        a.corpus = idx->corpus; a.qfrag = ws->qfrag.p; a.nrows = idx->n; a.npanels = (int)npanels; a.k = 1;
        a.scores = out_dev + (size_t)q0 * ld; a.ld = ld; a.nq = nqp;
        HIP_TRY(cmr_launch_scan_scores(g, a, s));
    }
    return CMR_OK;
}

int check_query_flag(Workspace* ws) {
    int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, ws->flag_ptr, sizeof(int), hipMemcpyDeviceToHost, ws->stream));
    HIP_TRY(hipStreamSynchronize(ws->stream));
    if (h) {
        HIP_TRY(hipMemsetAsync(ws->flag_ptr, 0, sizeof(int), ws->stream));
        return fail(CMR_ERR_NONFINITE, "query contains NaN/Inf or a value that rounds to Inf in the index dtype");
    }
    return CMR_OK;
}

int grow(cmr_index* idx, long long need_panels) {
    if (need_panels <= idx->cap_panels) return CMR_OK;
    long long new_cap = std::max(need_panels, idx->cap_panels * 2);
    new_cap = std::max<long long>(new_cap, 8);
    const size_t pb = idx->panel_bytes();
    // outstanding async searches may still read the old buffer
    HIP_TRY(hipDeviceSynchronize());
    void* nc = nullptr;
    HIP_TRY(hipMalloc(&nc, (size_t)new_cap * pb + CMR_CORPUS_SLACK));
    HIP_TRY(hipMemsetAsync(nc, 0, (size_t)new_cap * pb + CMR_CORPUS_SLACK, nullptr));
    const long long used_panels = idx->npanels();
    if (idx->corpus && used_panels)
        HIP_TRY(hipMemcpyAsync(nc, idx->corpus, (size_t)used_panels * pb, hipMemcpyDeviceToDevice, nullptr));
    float* ns = nullptr;
    if ((idx->flags & CMR_FLAG_KEEP_F32) && idx->dtype != CMR_F32) {
        HIP_TRY(hipMalloc((void**)&ns, (size_t)new_cap * CMR_PANEL_ROWS * idx->dim * sizeof(float)));
        if (idx->shadow && idx->n)
            HIP_TRY(hipMemcpyAsync(ns, idx->shadow, (size_t)idx->n * idx->dim * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
    }
    HIP_TRY(hipDeviceSynchronize());
    if (idx->corpus) HIP_TRY(hipFree(idx->corpus));
    if (idx->shadow) HIP_TRY(hipFree(idx->shadow));
    idx->corpus = nc;
    idx->shadow = ns;
    idx->cap_panels = new_cap;
    return CMR_OK;
}

// rows_dev: fp32 [n, dim] on the device; converts on `s`, checks finiteness, bumps n.
int append_from_device(cmr_index* idx, const float* rows_dev, long long n, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(idx->d_flag, 0, sizeof(int), s));
    HIP_TRY(cmr_launch_convert_rows(idx->dtype, rows_dev, n, idx->dim, idx->dpad, idx->n, idx->corpus, idx->shadow, idx->d_flag, s));
    HIP_TRY(cmr_launch_round_stats(idx->dtype, idx->shadow ? idx->shadow + (size_t)idx->n * idx->dim : rows_dev, n, idx->dim, idx->d_flag, idx->d_stats, s));
    int h = 0;
    HIP_TRY(hipMemcpyAsync(&h, idx->d_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h) return fail(CMR_ERR_NONFINITE, "appended rows contain NaN/Inf or a value that rounds to Inf in the index dtype (index unchanged)");
    idx->n += n;
    return CMR_OK;
}

// the pinned, device-mapped buffer of small appends and small row updates (exclusive lock held): [flag, 256 | rows | an update's plan]
int ensure_h_pin(cmr_index* idx) {
    if (idx->h_pin_cap >= kMappedPinBytes) return CMR_OK;
    if (idx->h_pin) { HIP_TRY(hipHostFree(idx->h_pin)); idx->h_pin = nullptr; idx->h_pin_cap = 0; }
    HIP_TRY(hipHostMalloc(&idx->h_pin, kMappedPinBytes, hipHostMallocDefault));
    HIP_TRY(hipHostGetDevicePointer(&idx->h_pin_dev, idx->h_pin, 0));
    idx->h_pin_cap = kMappedPinBytes;
    return CMR_OK;
}

}  // namespace

// ---- for ppr.hip: host queries -> N raw scores each in the workspace's device buffer, index lock + workspace kept until release
namespace { thread_local Workspace* tl_scores_ws = nullptr; }

// nb host queries [nb, dim] -> [nb, n] scores.  Row b must hold the bits a ONE-query scan of query b gives (the batched PPR promises
// what the single call returns).
int cmr_index_scores_to_device_batch(cmr_index_t* idx, const float* q_host, int nb, float** scores_dev, long long* n, void** stream) {
    if (!idx || !q_host || !scores_dev || !n || !stream || nb < 1) return fail(CMR_ERR_INVALID, "NULL argument");
    if (tl_scores_ws) return fail(CMR_ERR_INVALID, "nested cmr_index_scores_to_device on one thread");
    idx->mu.lock_shared();
    Workspace* ws = nullptr;
    int rc = open_ws(idx, nullptr, false, &ws);
    if (!rc) {
        hipStream_t s = ws->stream;
        auto body = [&]() -> int {
            const size_t q_bytes = (size_t)nb * idx->dim * 4;
            HIP_TRY(ws->d_q.ensure(q_bytes));
            HIP_TRY(ws->d_out.ensure(std::max<size_t>((size_t)nb * idx->n * 4, 8)));
            HIP_TRY(ws->ensure_pin(q_bytes));
            memcpy(ws->h_pin, q_host, q_bytes);
            HIP_TRY(hipMemcpyAsync(ws->d_q.p, ws->h_pin, q_bytes, hipMemcpyHostToDevice, s));
            if (idx->n == 0) return CMR_OK;
            // up to 32 queries share ONE geometry (make_geom: nqt = 1, the same kernel variant and grid as a one-query scan) and a query
            // is one MFMA column whose products and sums never meet another column's: one nq = nb scan gives every row its one-query bits
            // (checked on the device at 5 K x 128, 5 K x 768 and 200 K x 768, f32 and bf16).  Above 32 the tile changes: one by one, no sync.
            if (nb <= 32) return scores_enqueue(idx, ws, (const float*)ws->d_q.p, nb, (float*)ws->d_out.p, idx->n);
            for (int b = 0; b < nb; ++b) {
                int rc_ = scores_enqueue(idx, ws, (const float*)ws->d_q.p + (size_t)b * idx->dim, 1, (float*)ws->d_out.p + (size_t)b * idx->n, idx->n);
                if (rc_) return rc_;
            }
            return CMR_OK;
        };
        rc = body();
        if (rc) (void)hipStreamSynchronize(s);
    }
    if (rc) {
        if (ws) release_ws(idx, ws);
        idx->mu.unlock_shared();
        return rc;
    }
    tl_scores_ws = ws;
    *scores_dev = (float*)ws->d_out.p; *n = idx->n; *stream = (void*)ws->stream;
    return CMR_OK;
}

int cmr_index_scores_to_device(cmr_index_t* idx, const float* q_host, float** scores_dev, long long* n, void** stream) {
    return cmr_index_scores_to_device_batch(idx, q_host, 1, scores_dev, n, stream);
}

long long cmr_index_row_count(cmr_index_t* idx) {      // for ppr.hip's argument checks (no device call)
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    return idx->n;
}

// ---- for ppr.hip: the index's combiner (combine.h) — its width (0: off; *dim and *dtype for the host check of the query), one submission
int cmr_index_combine_width(cmr_index_t* idx, int* dim, int* dtype) {
    if (!idx) return 0;
    *dim = idx->dim;
    *dtype = idx->dtype;
    return idx->combine.load(std::memory_order_relaxed);
}
void cmr_index_combine_submit(cmr_index_t* idx, const cmr_combine::Key& key, cmr_combine::Request* req, int width, cmr_combine::RunFn run, void* ctx) {
    idx->combiner.submit(key, req, width, idx->combine_wait_us.load(std::memory_order_relaxed), run, ctx);
}

int cmr_index_scores_release(cmr_index_t* idx) {
    Workspace* ws = tl_scores_ws;
    if (!idx || !ws) return CMR_OK;
    tl_scores_ws = nullptr;
    int rc = ws->flag_ptr ? check_query_flag(ws) : CMR_OK;
    release_ws(idx, ws);
    idx->mu.unlock_shared();
    return rc;
}

// ============================================================================================
extern "C" {

int32_t cmr_abi_version(void) { return CMR_ABI_VERSION; }
const char* cmr_last_error(void) { return g_err.c_str(); }

int32_t cmr_device_count(int32_t* n) {
    if (!n) return fail(CMR_ERR_INVALID, "n is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    *n = (e == hipSuccess) ? c : 0;
    return CMR_OK;
}

int32_t cmr_device_info(int32_t device_id, char* name, int32_t name_len, int32_t* n_cu, int64_t* hbm_bytes) {
    int rc = cmr_check_device(device_id);
    if (rc) return rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (name && name_len > 0) snprintf(name, (size_t)name_len, "%s (%s)", prop.name, prop.gcnArchName);
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    return CMR_OK;
}

int32_t cmr_index_create(int32_t device_id, int32_t dim, int32_t dtype, int64_t capacity_hint, uint32_t flags, cmr_index_t** out) {
    if (!out) return fail(CMR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (dim <= 0 || dim > 16384) return fail(CMR_ERR_INVALID, "dim %d out of range", dim);
    if (dtype != CMR_F32 && dtype != CMR_BF16 && dtype != CMR_F16) return fail(CMR_ERR_INVALID, "unknown dtype %d", dtype);
    int rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    cmr_index* idx = new cmr_index();
    idx->device = device_id;
    idx->dim = dim;
    idx->dpad = round_up(dim, 128);
    idx->dtype = dtype;
    idx->flags = flags;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess) idx->n_cu = prop.multiProcessorCount;
    if (cmr_scan_max_nqt(dtype, idx->dpad) == 0) {
        delete idx;
        return fail(CMR_ERR_UNSUPPORTED, "dim %d (padded %d) exceeds the LDS-resident query tile for dtype %d", dim, round_up(dim, 128), dtype);
    }
    if (hipMalloc((void**)&idx->d_flag, sizeof(int)) != hipSuccess) { delete idx; return fail(CMR_ERR_OOM, "hipMalloc flag"); }
    if (hipMalloc((void**)&idx->d_stats, 2 * sizeof(float)) != hipSuccess || hipMemset(idx->d_stats, 0, 2 * sizeof(float)) != hipSuccess) {
        if (idx->d_stats) (void)hipFree(idx->d_stats);
        (void)hipFree(idx->d_flag); delete idx; return fail(CMR_ERR_OOM, "hipMalloc round stats");
    }
    const long long hint_panels = std::max<long long>(panels_of(capacity_hint), 8);
    rc = grow(idx, hint_panels);
    if (rc) { (void)hipFree(idx->d_flag); (void)hipFree(idx->d_stats); delete idx; return rc; }
    *out = idx;
    return CMR_OK;
}

int32_t cmr_index_destroy(cmr_index_t* idx) {
    if (!idx) return CMR_OK;
    {
        std::unique_lock<std::shared_mutex> lk(idx->mu);
        (void)hipSetDevice(idx->device);
        (void)hipDeviceSynchronize();
        for (Workspace* w : idx->free_ws) { w->release(); delete w; }
        for (auto& kv : idx->stream_ws) { kv.second->release(); delete kv.second; }
        for (ProfEvent& pe : idx->prof_events) { (void)hipEventDestroy(pe.a); (void)hipEventDestroy(pe.b); }
        for (int i = 0; i < CMR_PIPE_SLOTS; ++i) {
            idx->pipe.slot[i].ws.stream = nullptr;
            idx->pipe.slot[i].ws.release();
            if (idx->pipe.slot[i].pre_done) (void)hipEventDestroy(idx->pipe.slot[i].pre_done);
            if (idx->pipe.slot[i].main_done) (void)hipEventDestroy(idx->pipe.slot[i].main_done);
            if (idx->pipe.slot[i].scan_done) (void)hipEventDestroy(idx->pipe.slot[i].scan_done);
        }
        idx->pipe.destroy_streams();
        idx->stage.release();
        idx->rm_buf.release();
        if (idx->h_pin) { (void)hipHostFree(idx->h_pin); idx->h_pin = nullptr; idx->h_pin_cap = 0; }
        if (idx->corpus) (void)hipFree(idx->corpus);
        if (idx->shadow) (void)hipFree(idx->shadow);
        if (idx->d_flag) (void)hipFree(idx->d_flag);
        if (idx->d_stats) (void)hipFree(idx->d_stats);
        idx->q8c.release();
        for (ExactScratch& x : idx->x_slot) x.release();
        if (idx->d_blk) (void)hipFree(idx->d_blk);
        for (void* p : idx->blk_retired) (void)hipFree(p);
    }
    delete idx;
    return CMR_OK;
}

int32_t cmr_index_size(cmr_index_t* idx, int64_t* n_rows) {
    if (!idx || !n_rows) return fail(CMR_ERR_INVALID, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    *n_rows = idx->n;
    return CMR_OK;
}

int32_t cmr_index_info(cmr_index_t* idx, int32_t* dim, int32_t* dtype, int64_t* capacity_rows, int64_t* device_bytes) {
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    if (dim) *dim = idx->dim;
    if (dtype) *dtype = idx->dtype;
    if (capacity_rows) *capacity_rows = idx->cap_panels * CMR_PANEL_ROWS;
    if (device_bytes)
        *device_bytes = (int64_t)(idx->cap_panels * idx->panel_bytes() + CMR_CORPUS_SLACK +
                                  (idx->shadow ? (size_t)idx->cap_panels * CMR_PANEL_ROWS * idx->dim * 4 : 0));
    return CMR_OK;
}

int32_t cmr_index_append(cmr_index_t* idx, const float* rows, int64_t n) {
    if (!idx || (n > 0 && !rows)) return fail(CMR_ERR_INVALID, "NULL argument");
    if (n < 0) return fail(CMR_ERR_INVALID, "n < 0");
    if (n == 0) return CMR_OK;
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    if (idx->n + n >= 0xFFFFFFF0ll) return fail(CMR_ERR_UNSUPPORTED, "more than 2^32 rows per shard");
    if (global_id_overflow(idx, n)) return fail(CMR_ERR_UNSUPPORTED, "appending %lld rows takes this shard's global ids beyond the 32-bit row of the packed candidate exchange", (long long)n);
    rc = grow(idx, panels_of(idx->n + n));
    if (rc) return rc;
    if (idx->zero_copy && (size_t)n * idx->dim * 4 <= kMappedAppendMax) {
        // A handful of rows (MemoryPool's per-cycle nodes, a store's freshly inserted strings): rows and the non-finite flag
        // in a pinned, device-mapped buffer that the convert kernel reads / writes itself — one launch and one
        // synchronisation instead of a pageable H2D, a memset, the launch, the flag's D2H and the synchronisation.
        const size_t bytes = (size_t)n * idx->dim * 4;
        { int rc_ = ensure_h_pin(idx); if (rc_) return rc_; }
        char* h = (char*)idx->h_pin;
        char* d = (char*)idx->h_pin_dev;
        memset(h, 0, 8);
        memcpy(h + 256, rows, bytes);
        HIP_TRY(cmr_launch_convert_rows(idx->dtype, (const float*)(d + 256), n, idx->dim, idx->dpad, idx->n, idx->corpus, idx->shadow, (int*)d, nullptr));
        HIP_TRY(cmr_launch_round_stats(idx->dtype, idx->shadow ? idx->shadow + (size_t)idx->n * idx->dim : (const float*)(d + 256), n, idx->dim, (int*)d,
                                       idx->d_stats, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        int flagged = 0;
        memcpy(&flagged, h, sizeof(int));
        if (flagged) return fail(CMR_ERR_NONFINITE, "appended rows contain NaN/Inf or a value that rounds to Inf in the index dtype (index unchanged)");
        idx->n += n;
        return CMR_OK;
    }
    // stage in chunks of <= 256 MiB of fp32
    const long long chunk_rows = std::max<long long>(1, (256ll << 20) / ((long long)idx->dim * 4));
    const long long n0 = idx->n;
    // an append of several chunks that fails on a later one leaves the maxima of the exact search as they were before it
    float stats0[2] = {0.0f, 0.0f};
    const bool chunks = n > chunk_rows;
    if (chunks) HIP_TRY(hipMemcpy(stats0, idx->d_stats, sizeof(stats0), hipMemcpyDeviceToHost));
    auto undo_stats = [&]() { if (chunks) (void)hipMemcpy(idx->d_stats, stats0, sizeof(stats0), hipMemcpyHostToDevice); };
    for (long long r0 = 0; r0 < n; r0 += chunk_rows) {
        const long long nr = std::min<long long>(chunk_rows, n - r0);
        const size_t bytes = (size_t)nr * idx->dim * 4;
        hipError_t e = idx->stage.ensure(bytes);
        if (e != hipSuccess) { idx->n = n0; undo_stats(); return fail(CMR_ERR_OOM, "append staging: %s", hipGetErrorString(e)); }
        e = hipMemcpyAsync(idx->stage.p, rows + (size_t)r0 * idx->dim, bytes, hipMemcpyHostToDevice, nullptr);
        if (e != hipSuccess) { idx->n = n0; undo_stats(); return fail(CMR_ERR_HIP, "H2D rows: %s", hipGetErrorString(e)); }
        rc = append_from_device(idx, (const float*)idx->stage.p, nr, nullptr);
        if (rc) { idx->n = n0; undo_stats(); return rc; }
    }
    return CMR_OK;
}

int32_t cmr_index_append_dev(cmr_index_t* idx, const float* rows_dev, int64_t n, void* stream) {
    if (!idx || (n > 0 && !rows_dev)) return fail(CMR_ERR_INVALID, "NULL argument");
    if (n <= 0) return n == 0 ? CMR_OK : fail(CMR_ERR_INVALID, "n < 0");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    if (idx->n + n >= 0xFFFFFFF0ll) return fail(CMR_ERR_UNSUPPORTED, "more than 2^32 rows per shard");
    if (global_id_overflow(idx, n)) return fail(CMR_ERR_UNSUPPORTED, "appending %lld rows takes this shard's global ids beyond the 32-bit row of the packed candidate exchange", (long long)n);
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipStreamSynchronize(s));  // rows_dev producer done before a possible grow() reallocates
    rc = grow(idx, panels_of(idx->n + n));
    if (rc) return rc;
    return append_from_device(idx, rows_dev, n, s);
}

int32_t cmr_index_search_dev(cmr_index_t* idx, const float* q_dev, int32_t nq, int32_t k, int64_t* ids_dev, float* scores_dev,
                             float* min_dev, float* max_dev, void* stream) {
    if (!idx || !q_dev || !ids_dev || !scores_dev) return fail(CMR_ERR_INVALID, "NULL argument");
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    if (k <= 0 || k > CMR_MAX_K_2PASS) return fail(CMR_ERR_UNSUPPORTED, "k = %d outside [1, %d]", k, CMR_MAX_K_2PASS);
    DevCall call(idx);
    int rc = call.open(stream);
    if (rc) return rc;
    return search_enqueue(idx, call.ws, q_dev, nq, k, ids_dev, scores_dev, min_dev, max_dev);
}

int32_t cmr_index_search_min_score_dev(cmr_index_t* idx, const float* q_dev, int32_t nq, int32_t k, float min_score, int64_t* ids_dev,
                                       float* scores_dev, void* stream) {
    if (!idx || !q_dev || !ids_dev || !scores_dev) return fail(CMR_ERR_INVALID, "NULL argument");
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    if (k <= 0 || k > CMR_MAX_K) return fail(CMR_ERR_UNSUPPORTED, "threshold search supports k in [1, %d]", CMR_MAX_K);
    if (int rc_ = cmr_min_score_check(min_score)) return rc_;
    DevCall call(idx);
    int rc = call.open(stream);
    if (rc) return rc;
    return search_enqueue(idx, call.ws, q_dev, nq, k, ids_dev, scores_dev, nullptr, nullptr, &min_score);
}

int32_t cmr_index_search_pipelined(cmr_index_t* idx, const float* q_dev, int32_t nq, int32_t k, int64_t* ids_dev, float* scores_dev,
                                   float* min_dev, float* max_dev, void* wait_event, void** done_event) {
    if (!idx || !q_dev || !ids_dev || !scores_dev) return fail(CMR_ERR_INVALID, "NULL argument");
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    if (k <= 0 || k > CMR_MAX_K) return fail(CMR_ERR_UNSUPPORTED, "k = %d outside [1, %d]", k, CMR_MAX_K);
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    hipEvent_t done = nullptr;
    rc = search_pipelined_enqueue(idx, q_dev, nq, k, ids_dev, scores_dev, min_dev, max_dev, (hipEvent_t)wait_event, &done, nullptr, true);
    if (done_event) *done_event = (void*)done;
    return rc;
}

int32_t cmr_index_search_min_score_pipelined(cmr_index_t* idx, const float* q_dev, int32_t nq, int32_t k, float min_score, int64_t* ids_dev,
                                             float* scores_dev, void* wait_event, void** done_event) {
    if (!idx || !q_dev || !ids_dev || !scores_dev) return fail(CMR_ERR_INVALID, "NULL argument");
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    if (k <= 0 || k > CMR_MAX_K) return fail(CMR_ERR_UNSUPPORTED, "threshold search supports k in [1, %d]", CMR_MAX_K);
    if (int rc_ = cmr_min_score_check(min_score)) return rc_;
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    hipEvent_t done = nullptr;
    rc = search_pipelined_enqueue(idx, q_dev, nq, k, ids_dev, scores_dev, nullptr, nullptr, (hipEvent_t)wait_event, &done, &min_score);
    if (done_event) *done_event = (void*)done;
    return rc;
}

// the packed candidate exchange (comm.hip) carries the global row in 32 bits: 0xFFFFFFFF - row, key 0 = empty
static const long long kMaxGlobalId = 0xFFFFFFFEll;

int32_t cmr_index_set_id_base(cmr_index_t* idx, int64_t base) {
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    if (base < 0) return fail(CMR_ERR_INVALID, "id base %lld < 0", (long long)base);
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    if (base + idx->n - 1 > kMaxGlobalId)
        return fail(CMR_ERR_UNSUPPORTED, "id base %lld + %lld rows exceeds the 32-bit global row of the packed candidate exchange", (long long)base, idx->n);
    idx->id_base = base;
    idx->blk_local.clear(); idx->blk_global.clear();
    return CMR_OK;
}

int32_t cmr_index_set_id_blocks(cmr_index_t* idx, int32_t n_blocks, const int64_t* local_start, const int64_t* global_start) {
    if (!idx || n_blocks <= 0 || !local_start || !global_start) return fail(CMR_ERR_INVALID, "bad argument");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    if (local_start[0] != 0) return fail(CMR_ERR_INVALID, "the first block must start at local row 0");
    for (int b = 0; b < n_blocks; ++b) {
        const long long len = (b + 1 < n_blocks ? local_start[b + 1] : std::max<long long>(idx->n, local_start[b])) - local_start[b];
        if (global_start[b] < 0 || len < 0 || (b > 0 && (local_start[b] <= local_start[b - 1] || global_start[b] < global_start[b - 1] + (local_start[b] - local_start[b - 1]))))
            return fail(CMR_ERR_INVALID, "block %d: local starts must ascend and the global id runs must ascend without overlap", b);
        if (global_start[b] + len - 1 > kMaxGlobalId)
            return fail(CMR_ERR_UNSUPPORTED, "block %d reaches global id %lld: the packed candidate exchange carries 32-bit rows", b, (long long)(global_start[b] + len - 1));
    }
    if (n_blocks == 1) {
        idx->id_base = global_start[0];
        idx->blk_local.clear(); idx->blk_global.clear();
        return CMR_OK;
    }
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    std::vector<long long> tab((size_t)2 * n_blocks);
    for (int b = 0; b < n_blocks; ++b) { tab[b] = local_start[b]; tab[n_blocks + b] = global_start[b]; }
    long long* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, tab.size() * 8));
    HIP_TRY(hipMemcpy(d, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    if (idx->d_blk) idx->blk_retired.push_back(idx->d_blk);    // searches already enqueued keep reading the table they were given
    if (idx->blk_retired.size() >= 8) {                        // ... until the device has drained: then the old tables go
        HIP_TRY(hipDeviceSynchronize());
        for (void* p : idx->blk_retired) (void)hipFree(p);
        idx->blk_retired.clear();
    }
    idx->d_blk = d;
    idx->blk_local.assign(local_start, local_start + n_blocks);
    idx->blk_global.assign(global_start, global_start + n_blocks);
    idx->id_base = global_start[0];
    return CMR_OK;
}

int32_t cmr_index_set_option(cmr_index_t* idx, const char* name, int64_t value) {
    if (!idx || !name) return fail(CMR_ERR_INVALID, "NULL argument");
    std::unique_lock<std::shared_mutex> lk(idx->mu);
    return set_option(idx, name, value);
}

int32_t cmr_index_get_option(cmr_index_t* idx, const char* name, int64_t* value) {
    if (!idx || !name || !value) return fail(CMR_ERR_INVALID, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    const Option* o = find_option(name);
    if (!o || !o->read) return fail(CMR_ERR_INVALID, "unknown readable option '%s'", name);
    *value = o->read(idx);
    return CMR_OK;
}

int32_t cmr_index_pipeline_stream(cmr_index_t* idx, int32_t which, void** stream) {
    if (!idx || !stream) return fail(CMR_ERR_INVALID, "NULL argument");
    if (which < 0 || which > 2) return fail(CMR_ERR_INVALID, "which must be 0 (pre), 1 (scan) or 2 (post)");
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    std::lock_guard<std::mutex> pl(idx->pipe_mu);
    Pipe& P = idx->pipe;
    rc = ensure_pipe(idx);
    if (rc) return rc;
    const bool twins = P.scan_cus != 0 && !P.last_masked && P.next != 0;      // the set the last narrow batch ran on
    *stream = (void*)P.st[which == 0 ? (twins ? Pipe::usp : Pipe::sp) : which == 1 ? (twins ? Pipe::usm : Pipe::sm) : Pipe::sq];
    return CMR_OK;
}

int32_t cmr_index_query_status(cmr_index_t* idx, int32_t* nonfinite) {
    if (!idx || !nonfinite) return fail(CMR_ERR_INVALID, "NULL argument");
    *nonfinite = 0;
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    std::vector<Workspace*> wss;
    {
        std::lock_guard<std::mutex> pl(idx->pipe_mu);
        for (int i = 0; i < CMR_PIPE_SLOTS; ++i) if (idx->pipe.slot[i].used) wss.push_back(&idx->pipe.slot[i].ws);
        if (idx->pipe.st[Pipe::sq]) {
            for (hipStream_t st : idx->pipe.st) if (st) HIP_TRY(hipStreamSynchronize(st));
        }
    }
    {
        std::lock_guard<std::mutex> g(idx->ws_mu);
        for (auto& kv : idx->stream_ws) wss.push_back(kv.second);
    }
    for (Workspace* ws : wss) {
        if (!ws->flag_ptr) continue;
        if (ws->stream || !ws->own_stream) HIP_TRY(hipStreamSynchronize(ws->stream));
        int h = 0;
        HIP_TRY(hipMemcpy(&h, ws->flag_ptr, sizeof(int), hipMemcpyDeviceToHost));
        if (h) {
            *nonfinite = 1;
            HIP_TRY(hipMemset(ws->flag_ptr, 0, sizeof(int)));
        }
    }
    return CMR_OK;
}

int32_t cmr_stream_wait_event(void* stream, void* event) {
    if (!event) return CMR_OK;
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
    return CMR_OK;
}

int32_t cmr_event_synchronize(void* event) {
    if (!event) return CMR_OK;
    HIP_TRY(hipEventSynchronize((hipEvent_t)event));
    return CMR_OK;
}

}  // extern "C"

// ---- synchronous host-buffer search in two halves (cmr_internal.h): `begin` enqueues everything on the workspace's stream and
// returns without waiting, `finish` waits, checks the non-finite flag and copies the results out.  cmr_index_search is begin +
// finish; the multi-device index (multi.hip) begins on every shard before it finishes on any, so all devices scan at once.
// Every synchronous top-k call — unfiltered, masked, from id lists, on one index or on the shards of a multi-device one — is begin +
// finish on a CmrPending; everything but the mapped branch of cmr_index_search_begin begins in packed_begin.

// the packed result buffer of such a call, on the device and in the pinned host buffer: [flag 8 B | ids nq*k i64 | scores nq*k f32 | min nq | max nq]
struct PackLayout {
    size_t o_ids = 8, o_sc, o_min, o_max, bytes;
    PackLayout(int nq, int k) {
        o_sc = o_ids + (size_t)nq * k * 8; o_min = o_sc + (size_t)nq * k * 4; o_max = o_min + (size_t)nq * 4; bytes = o_max + (size_t)nq * 4;
    }
};

struct CmrPending {
    cmr_index* idx;
    Workspace* ws = nullptr;
    bool locked = false;          // holds idx->mu shared (released by finish / abandon ON THE SAME THREAD)
    bool mapped = false;          // results land in the pinned buffer by themselves (zero-copy) / by the enqueued D2H copy
    bool poll = false;            // the search's last kernel sets the done word of the pinned buffer (Workspace::done_ptr): finish polls it
    int nq, k;
    PackLayout at;
    CmrPending(cmr_index* i, int nq_, int k_) : idx(i), nq(nq_), k(k_), at(nq_, k_) {}
};

static void pending_release(CmrPending* p) {
    if (p->ws) release_ws(p->idx, p->ws);
    if (p->locked) p->idx->mu.unlock_shared();
    delete p;
}
// a begin that failed with work possibly enqueued: nothing of it outlives the call
static int pending_fail(CmrPending* p, int rc) {
    (void)hipStreamSynchronize(p->ws->stream);
    pending_release(p);
    return rc;
}

// the index's shared lock (take_lock), the device, a pooled workspace
static int pending_open(cmr_index* idx, int nq, int k, bool take_lock, CmrPending** out) {
    CmrPending* P = new CmrPending(idx, nq, k);
    if (take_lock) { idx->mu.lock_shared(); P->locked = true; }
    const int rc = open_ws(idx, nullptr, false, &P->ws);
    if (rc) { pending_release(P); return rc; }
    *out = P;
    return CMR_OK;
}

// One host input of a packed call: up to two host pieces that go up as ONE block, into a buffer of the workspace.
struct PackedInput { DevBuf Workspace::* dst; const void* a; size_t a_bytes; const void* b = nullptr; size_t b_bytes = 0; };

// The copy path of a synchronous top-k call, on an opened pending call: the inputs staged in the pinned buffer (each at an 8-byte
// boundary) and copied up, one copy per input (none for an empty one); `enqueue(ws, ids, scores, min, max)` — the device work, writing
// the four areas of the packed device buffer, whose head is the call's non-finite flag; the pack copied down into the pinned buffer (which
// still holds what the H2D copies read: stream order puts the D2H copy behind them).  Ends in cmr_index_search_finish / _abandon; a
// failure releases the pending call here.
template <int N, class Enqueue>
static int packed_enqueue(CmrPending* P, const PackedInput (&in)[N], Enqueue&& enqueue) {
    Workspace* const ws = P->ws;
    hipStream_t const s = ws->stream;
    const PackLayout& at = P->at;
    auto body = [&]() -> int {
        size_t o_in[N], staged = 0;
        for (int i = 0; i < N; ++i) {
            const size_t bytes = in[i].a_bytes + in[i].b_bytes;
            HIP_TRY((ws->*in[i].dst).ensure(std::max<size_t>(bytes, 8)));
            o_in[i] = staged;
            staged += (bytes + 7) & ~(size_t)7;
        }
        if (at.bytes > ws->d_pack.cap || !ws->d_pack.p) {        // (re)allocation moves the flag: re-arm it at the new place
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(ws->d_pack.ensure(std::max<size_t>(at.bytes, 4096)));
            HIP_TRY(hipMemsetAsync(ws->d_pack.p, 0, 8, s));
        }
        char* const pk = (char*)ws->d_pack.p;
        FlagOverride flag(ws, (int*)pk);
        HIP_TRY(ws->ensure_pin(std::max(at.bytes, staged)));
        char* const hp = (char*)ws->h_pin;
        for (int i = 0; i < N; ++i) {
            if (in[i].a_bytes) memcpy(hp + o_in[i], in[i].a, in[i].a_bytes);
            if (in[i].b_bytes) memcpy(hp + o_in[i] + in[i].a_bytes, in[i].b, in[i].b_bytes);
        }
        // (everything staged first: the copies then reach the stream back to back, with no host memcpy of a mask between two submissions)
        for (int i = 0; i < N; ++i)
            if (const size_t bytes = in[i].a_bytes + in[i].b_bytes) HIP_TRY(hipMemcpyAsync((ws->*in[i].dst).p, hp + o_in[i], bytes, hipMemcpyHostToDevice, s));
        const int rc_ = enqueue(ws, (int64_t*)(pk + at.o_ids), (float*)(pk + at.o_sc), (float*)(pk + at.o_min), (float*)(pk + at.o_max));
        if (rc_) return rc_;
        HIP_TRY(hipMemcpyAsync(hp, pk, at.bytes, hipMemcpyDeviceToHost, s));
        return CMR_OK;
    };
    const int rc = body();
    return rc ? pending_fail(P, rc) : CMR_OK;
}

template <int N, class Enqueue>
static int packed_begin(cmr_index* idx, int nq, int k, bool take_lock, const PackedInput (&in)[N], Enqueue&& enqueue, CmrPending** out) {
    CmrPending* P = nullptr;
    int rc = pending_open(idx, nq, k, take_lock, &P);
    if (rc) return rc;
    rc = packed_enqueue(P, in, enqueue);
    if (rc) return rc;
    *out = P;
    return CMR_OK;
}

int cmr_index_search_begin(cmr_index_t* idx, const float* q, int nq, int k, const float* min_score, bool take_lock, CmrPending** out) {
    if (!idx || !q || !out) return fail(CMR_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    if (k <= 0 || k > CMR_MAX_K_2PASS) return fail(CMR_ERR_UNSUPPORTED, "k = %d outside [1, %d]", k, CMR_MAX_K_2PASS);
    CmrPending* P = nullptr;
    int rc = pending_open(idx, nq, k, take_lock, &P);
    if (rc) return rc;
    Workspace* const ws = P->ws;
    hipStream_t const s = ws->stream;
    const PackLayout& at = P->at;
    const size_t q_bytes = (size_t)nq * idx->dim * 4;
    if (idx->zero_copy && k <= CMR_MAX_K && q_bytes <= kZeroCopyMax && at.bytes <= kZeroCopyMax) {
        auto body = [&]() -> int {
            // (the hierarchical single-launch path packs the queries in up to 64 workgroups: they read a device copy, not
            // 64 times across the link)
            const bool map_in = small_path_kind(idx, nq, k, min_score != nullptr) != 2;
            // Small calls (what ComoRAG issues: one query, a few hundred rows) are all latency.  A copy each way costs two more
            // submissions in front of / behind the kernels (36 us per call at 6 rows, of which the search itself is ~8); so
            // there are none: queries, results and the non-finite flag live in ONE pinned, device-mapped host buffer
            // (fine-grained: kernel stores are visible once the stream has been synchronised) that the kernels read and
            // write over PCIe themselves — a few KiB either way.
            MappedStage m;
            { int rc_ = stage_mapped(ws, at.bytes, q_bytes, true, &m); if (rc_) return rc_; }
            char* const d = m.d;
            memcpy(m.h + m.o_in, q, q_bytes);
            const float* q_in = (const float*)(d + m.o_in);
            if (!map_in) {
                HIP_TRY(ws->d_q.ensure(q_bytes));
                HIP_TRY(hipMemcpyAsync(ws->d_q.p, m.h + m.o_in, q_bytes, hipMemcpyHostToDevice, s));
                q_in = (const float*)ws->d_q.p;
            }
            FlagOverride flag(ws, (int*)d);
            ws->done_ptr = idx->sync_poll ? (int*)(d + 4) : nullptr; ws->done_used = false; ws->lazy.due = false;      // (bytes 4..7 of the header were zeroed by stage_mapped)
            const int rc_ = search_enqueue(idx, ws, q_in, nq, k, (int64_t*)(d + at.o_ids), (float*)(d + at.o_sc), (float*)(d + at.o_min), (float*)(d + at.o_max), min_score);
            ws->done_ptr = nullptr;
            P->mapped = true;
            P->poll = rc_ == CMR_OK && ws->done_used;
            return rc_;
        };
        rc = body();
        if (rc) return pending_fail(P, rc);
    } else {
        // packed device buffer and its pinned host twin, one copy each way; the queries go through the pinned buffer too (a
        // pageable H2D is staged by the runtime anyway)
        const PackedInput in[] = {{&Workspace::d_q, q, q_bytes}};
        rc = packed_enqueue(P, in, [&](Workspace* w, int64_t* ids, float* sc, float* mn, float* mx) {
            return search_enqueue(idx, w, (const float*)w->d_q.p, nq, k, ids, sc, mn, mx, min_score);
        });
        if (rc) return rc;
    }
    *out = P;
    return CMR_OK;
}

int cmr_index_search_finish(CmrPending* P, int64_t* out_ids, float* out_scores, float* out_min, float* out_max) {
    if (!P) return fail(CMR_ERR_INVALID, "NULL pending search");
    struct Rel { CmrPending* p; ~Rel() { pending_release(p); } } rel{P};
    int rc = cmr_set_device(P->idx->device);
    if (rc) return rc;
    Workspace* ws = P->ws;
    if (P->poll) {
        int st = 0;
        { int rc_ = wait_done_word(ws, &st); if (rc_) return rc_; }
        if (ws->lazy.due && st != 1) {      // a dense list or a staging area of the finishing stage overflowed: the merge works from the per-wave lists
            const Workspace::LazyMerge& L = ws->lazy;
            ws->lazy.due = false;
            HIP_TRY(cmr_launch_merge_query(L.lists, L.cnt, L.W, L.NQ, L.cap, L.nqp, L.k, L.mm, L.id_base, L.ids, L.scores, L.mn, L.mx, nullptr, ws->stream, false, L.state));
            HIP_TRY(hipStreamSynchronize(ws->stream));
        }
        ws->lazy.due = false;
    } else {
        HIP_TRY(hipStreamSynchronize(ws->stream));
    }
    const char* hp = (const char*)ws->h_pin;
    int flagged = 0;
    memcpy(&flagged, hp, sizeof(int));
    if (flagged) {
        if (!P->mapped) HIP_TRY(hipMemsetAsync(ws->d_pack.p, 0, sizeof(int), ws->stream));
        return fail(CMR_ERR_NONFINITE, "query contains NaN/Inf or a value that rounds to Inf in the index dtype");
    }
    const size_t nk = (size_t)P->nq * P->k;
    if (out_ids) memcpy(out_ids, hp + P->at.o_ids, nk * 8);
    if (out_scores) memcpy(out_scores, hp + P->at.o_sc, nk * 4);
    if (out_min) memcpy(out_min, hp + P->at.o_min, (size_t)P->nq * 4);
    if (out_max) memcpy(out_max, hp + P->at.o_max, (size_t)P->nq * 4);
    return CMR_OK;
}

void cmr_index_search_abandon(CmrPending* P) {
    if (!P) return;
    (void)hipSetDevice(P->idx->device);
    (void)hipStreamSynchronize(P->ws->stream);
    P->ws->lazy.due = false;
    // a query flagged non-finite leaves its mark in the packed DEVICE buffer of the copy path: clear it for the next call
    if (!P->mapped && P->ws->d_pack.p) (void)hipMemsetAsync(P->ws->d_pack.p, 0, sizeof(int), P->ws->stream);
    pending_release(P);
}

extern "C" {

static int32_t host_search(cmr_index_t* idx, const float* q, int32_t nq, int32_t k, int64_t* out_ids, float* out_scores,
                           float* out_min, float* out_max, const float* min_score) {
    if (!idx || !q || !out_ids || !out_scores) return fail(CMR_ERR_INVALID, "NULL argument");
    CmrPending* p = nullptr;
    int rc = cmr_index_search_begin(idx, q, nq, k, min_score, true, &p);
    if (rc) return rc;
    return cmr_index_search_finish(p, out_ids, out_scores, out_min, out_max);
}

// ---- combined synchronous calls (combine.h): what the leader of a batch runs.  A batch of one is the caller's own call,
// unchanged; a wider one is ONE call of the same entry point on the concatenated queries, whose rows hold the bits of the single calls
// (DESIGN 4.9b), scattered to the participants.
struct CombinedSearch { const float* q; int nq, k; int64_t* ids; float* scores; float* mn; float* mx; };
struct CombinedScores { const float* q; int nq; float* out; long long ld; };
static const CombinedSearch* search_args(const cmr_combine::Request* r) { return (const CombinedSearch*)r->args; }

// code and (on failure) this thread's message into the request; the participant publishes them in its own thread
static void combine_answer(cmr_combine::Request* r, int rc) {
    r->rc = rc;
    if (rc) r->err = g_err;
}
static int combine_result(const cmr_combine::Request& r) {
    if (r.rc) g_err = r.err;
    return r.rc;
}

// The one call of a batch of top-k calls of one k (search_args of every request: a CombinedSearch, or what extends it): the participants'
// queries gathered into one block, room for the batch's rows (`all`), and the answer with each participant's rows scattered to it.
struct CombinedTopk {
    std::vector<float> q, sc, mm;
    std::vector<int64_t> ids;
    CombinedSearch all;
    CombinedTopk(cmr_combine::Request** reqs, int n, size_t dim) {
        int NQ = 0;
        for (int i = 0; i < n; ++i) NQ += reqs[i]->nq;
        const int k = search_args(reqs[0])->k;
        q.resize((size_t)NQ * dim); sc.resize((size_t)NQ * k); mm.resize((size_t)NQ * 2); ids.resize((size_t)NQ * k);
        for (int i = 0, q0 = 0; i < n; q0 += reqs[i++]->nq) memcpy(q.data() + (size_t)q0 * dim, search_args(reqs[i])->q, (size_t)reqs[i]->nq * dim * 4);
        all = CombinedSearch{q.data(), NQ, k, ids.data(), sc.data(), mm.data(), mm.data() + NQ};
    }
    CombinedTopk(const CombinedTopk&) = delete;      // (`all` points into this object's vectors)
    void answer(cmr_combine::Request** reqs, int n, int rc) const {
        for (int i = 0, q0 = 0; i < n; q0 += reqs[i++]->nq) {
            const CombinedSearch* a = search_args(reqs[i]);
            combine_answer(reqs[i], rc);
            if (rc) continue;
            const size_t nk = (size_t)a->nq * all.k;
            memcpy(a->ids, all.ids + (size_t)q0 * all.k, nk * 8);
            memcpy(a->scores, all.scores + (size_t)q0 * all.k, nk * 4);
            if (a->mn) memcpy(a->mn, all.mn + q0, (size_t)a->nq * 4);
            if (a->mx) memcpy(a->mx, all.mx + q0, (size_t)a->nq * 4);
        }
    }
};

static void combined_search_run(void* ctx, cmr_combine::Request** reqs, int n) {
    cmr_index* const idx = (cmr_index*)ctx;
    const CombinedSearch* a0 = search_args(reqs[0]);
    if (n == 1) { combine_answer(reqs[0], host_search(idx, a0->q, a0->nq, a0->k, a0->ids, a0->scores, a0->mn, a0->mx, nullptr)); return; }
    const CombinedTopk b(reqs, n, (size_t)idx->dim);
    b.answer(reqs, n, host_search(idx, b.all.q, b.all.nq, b.all.k, b.all.ids, b.all.scores, b.all.mn, b.all.mx, nullptr));
}

int32_t cmr_index_search(cmr_index_t* idx, const float* q, int32_t nq, int32_t k, int64_t* out_ids, float* out_scores,
                         float* out_min, float* out_max) {
    const int W = idx ? idx->combine.load(std::memory_order_relaxed) : 0;
    // joins a batch: fewer queries than the batch holds, the fused search (k <= CMR_MAX_K), and finite queries — the batch kernels carry one
    // non-finite flag per launch, so such a query takes the single call and gets its CMR_ERR_NONFINITE there, as every refused argument gets its error
    if (!W || !q || !out_ids || !out_scores || nq <= 0 || nq >= W || k <= 0 || k > CMR_MAX_K || !cmr_combine::all_finite(q, (size_t)nq * idx->dim, idx->dtype))
        return host_search(idx, q, nq, k, out_ids, out_scores, out_min, out_max, nullptr);
    CombinedSearch a{q, nq, k, out_ids, out_scores, out_min, out_max};
    cmr_combine::Request r;
    r.args = &a; r.nq = nq;
    cmr_combine::Key key;
    key.w[0] = 1; key.w[1] = (uint64_t)k;
    idx->combiner.submit(key, &r, W, idx->combine_wait_us.load(std::memory_order_relaxed), combined_search_run, idx);
    return combine_result(r);
}

int32_t cmr_index_search_min_score(cmr_index_t* idx, const float* q, int32_t nq, int32_t k, float min_score, int64_t* out_ids,
                                   float* out_scores) {
    if (int rc_ = cmr_min_score_check(min_score)) return rc_;
    return host_search(idx, q, nq, k, out_ids, out_scores, nullptr, nullptr, &min_score);
}

int32_t cmr_index_scores_dev(cmr_index_t* idx, const float* q_dev, int32_t nq, float* out_dev, int64_t ld, void* stream) {
    if (!idx || !q_dev || !out_dev) return fail(CMR_ERR_INVALID, "NULL argument");
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    DevCall call(idx);
    if (ld == 0) ld = idx->n;
    if (ld < idx->n) return fail(CMR_ERR_INVALID, "ld %lld < rows %lld", (long long)ld, idx->n);
    int rc = call.open(stream);
    if (rc) return rc;
    if (idx->n == 0) return CMR_OK;
    return scores_enqueue(idx, call.ws, q_dev, nq, out_dev, ld);
}

// cmr_index_scores behind its argument checks: `call` holds the index's shared lock, ld >= idx->n > 0
static int scores_sync(SyncCall& call, const float* q, int32_t nq, float* out, int64_t ld) {
    cmr_index* const idx = call.idx;
    int rc = call.open();
    if (rc) return rc;
    Workspace* const ws = call.ws;
    hipStream_t const s = call.s;
    {   // Small corpus, few queries (dense_passage_retrieval / get_fact_scores on a few thousand rows, one query per call):
        // ONE launch packs, scans and writes the scores straight into a pinned, device-mapped host buffer — no pack
        // launch, no copies, one synchronisation (the general path: pageable H2D, pack, scan, 2-D D2H, flag D2H, two syncs).
        const long long npanels = idx->npanels();
        const size_t sc_bytes = (size_t)nq * idx->n * 4, q_bytes = (size_t)nq * idx->dim * 4;
        if (idx->zero_copy && !idx->no_tiny && !idx->no_small && nq <= 16 && npanels <= idx->small_max_panels && idx->small_operands_fit() &&
            sc_bytes <= 4 * kZeroCopyMax) {
            const size_t o_sc = 256;      // (results: the 8-byte header, the scores from byte 256 on)
            MappedStage m;
            { int rc_ = stage_mapped(ws, o_sc + sc_bytes, q_bytes, true, &m); if (rc_) return rc_; }
            char* const h = m.h; char* const d = m.d;
            const size_t o_q = m.o_in;
            memcpy(h + o_q, q, q_bytes);
            const float* q_in = (const float*)(d + o_q);
            if (npanels > 32) {               // many workgroups pack the queries: from a device copy, not across the link once each
                HIP_TRY(ws->d_q.ensure(q_bytes));
                HIP_TRY(hipMemcpyAsync(ws->d_q.p, h + o_q, q_bytes, hipMemcpyHostToDevice, s));
                q_in = (const float*)ws->d_q.p;
            }
            HIP_TRY(ws->d_out.ensure((size_t)nq * npanels * CMR_PANEL_ROWS * 4));
            idx->last_route.store(route_code(CMR_ROUTE_SCORES_SINGLE), std::memory_order_relaxed);
            if (idx->sync_poll && !ws->arrive.p) {          // arrival counter: zeroed once, re-armed by the kernel
                HIP_TRY(ws->arrive.ensure(sizeof(int)));
                HIP_TRY(hipMemsetAsync(ws->arrive.p, 0, sizeof(int), s));
            }
            HIP_TRY(cmr_launch_tiny_scores(idx->dtype, idx->corpus, q_in, nq, idx->dim, idx->dpad, idx->n, ws->d_out.p, (float*)(d + o_sc), idx->n,
                                           (int*)d, s, idx->sync_poll ? (int*)ws->arrive.p : nullptr, idx->sync_poll ? (int*)(d + 4) : nullptr));
            if (idx->sync_poll) { int rc_ = wait_done_word(ws); if (rc_) return rc_; }      // the last workgroup's word behind everybody's rows (bytes 4..7, zeroed above)
            else HIP_TRY(hipStreamSynchronize(s));
            int flagged = 0;
            memcpy(&flagged, h, sizeof(int));
            if (flagged) return fail(CMR_ERR_NONFINITE, "query contains NaN/Inf or a value that rounds to Inf in the index dtype");
            for (int qi = 0; qi < nq; ++qi) memcpy(out + (size_t)qi * ld, h + o_sc + (size_t)qi * idx->n * 4, (size_t)idx->n * 4);
            return CMR_OK;
        }
    }
    HIP_TRY(ws->d_q.ensure((size_t)nq * idx->dim * 4));
    HIP_TRY(ws->d_out.ensure((size_t)nq * idx->n * 4));
    HIP_TRY(hipMemcpyAsync(ws->d_q.p, q, (size_t)nq * idx->dim * 4, hipMemcpyHostToDevice, s));
    rc = scores_enqueue(idx, ws, (const float*)ws->d_q.p, nq, (float*)ws->d_out.p, idx->n);
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    idx->last_route.store(route_code(CMR_ROUTE_SCORES), std::memory_order_relaxed);
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)ld * 4, ws->d_out.p, (size_t)idx->n * 4, (size_t)idx->n * 4, (size_t)nq,
                             hipMemcpyDeviceToHost, s));
    return check_query_flag(ws);
}

// one lock for the batch; every caller's ld is judged under it and a caller that fails is answered alone
static void combined_scores_run(void* ctx, cmr_combine::Request** reqs, int n) {
    cmr_index* const idx = (cmr_index*)ctx;
    SyncCall call(idx);
    const long long rows = idx->n;
    cmr_combine::Request* live[cmr_combine::kMaxWidth];
    int nl = 0, NQ = 0;
    for (int i = 0; i < n; ++i) {
        CombinedScores* a = (CombinedScores*)reqs[i]->args;
        if (a->ld == 0) a->ld = rows;
        if (a->ld < rows) { combine_answer(reqs[i], fail(CMR_ERR_INVALID, "ld %lld < rows %lld", a->ld, rows)); continue; }
        if (rows == 0) { combine_answer(reqs[i], CMR_OK); continue; }
        live[nl++] = reqs[i];
        NQ += reqs[i]->nq;
    }
    if (nl == 0) return;
    if (nl == 1) {
        const CombinedScores* a = (const CombinedScores*)live[0]->args;
        combine_answer(live[0], scores_sync(call, a->q, a->nq, a->out, a->ld));
        return;
    }
    const size_t dim = (size_t)idx->dim;
    std::unique_ptr<float[]> q(new float[(size_t)NQ * dim]), out(new float[(size_t)NQ * rows]);
    for (int i = 0, at = 0; i < nl; at += live[i++]->nq) memcpy(q.get() + (size_t)at * dim, ((const CombinedScores*)live[i]->args)->q, (size_t)live[i]->nq * dim * 4);
    const int rc = scores_sync(call, q.get(), NQ, out.get(), rows);
    for (int i = 0, at = 0; i < nl; at += live[i++]->nq) {
        const CombinedScores* a = (const CombinedScores*)live[i]->args;
        combine_answer(live[i], rc);
        if (rc) continue;
        for (int qi = 0; qi < a->nq; ++qi) memcpy(a->out + (size_t)qi * a->ld, out.get() + (size_t)(at + qi) * rows, (size_t)rows * 4);
    }
}

int32_t cmr_index_scores(cmr_index_t* idx, const float* q, int32_t nq, float* out, int64_t ld) {
    if (!idx || !q || !out) return fail(CMR_ERR_INVALID, "NULL argument");
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    const int W = idx->combine.load(std::memory_order_relaxed);
    if (W && nq < W && cmr_combine::all_finite(q, (size_t)nq * idx->dim, idx->dtype)) {      // (a non-finite query: the single call below, and its error)
        CombinedScores a{q, nq, out, ld};
        cmr_combine::Request r;
        r.args = &a; r.nq = nq;
        cmr_combine::Key key;
        key.w[0] = 2;
        idx->combiner.submit(key, &r, W, idx->combine_wait_us.load(std::memory_order_relaxed), combined_scores_run, idx);
        return combine_result(r);
    }
    SyncCall call(idx);
    if (ld == 0) ld = idx->n;
    if (ld < idx->n) return fail(CMR_ERR_INVALID, "ld %lld < rows %lld", (long long)ld, idx->n);
    if (idx->n == 0) return CMR_OK;
    return scores_sync(call, q, nq, out, ld);
}

int32_t cmr_index_sorted_scores(cmr_index_t* idx, const float* q, int32_t nq, int64_t* out_ids, float* out_scores, float* out_min,
                                float* out_max) {
    if (!idx || !q || !out_ids || !out_scores) return fail(CMR_ERR_INVALID, "NULL argument");
    if (nq <= 0) return fail(CMR_ERR_INVALID, "nq must be > 0");
    SyncCall call(idx);
    const long long n = idx->n;
    if (n == 0) return CMR_OK;
    int rc = call.open();
    if (rc) return rc;
    Workspace* const ws = call.ws;
    hipStream_t const s = call.s;
    HIP_TRY(ws->d_q.ensure((size_t)nq * idx->dim * 4));
    HIP_TRY(ws->d_out.ensure((size_t)n * 4));
    HIP_TRY(ws->d_cand.ensure(cmr_sort_workspace_bytes(n, 1, 4)));
    HIP_TRY(hipMemcpyAsync(ws->d_q.p, q, (size_t)nq * idx->dim * 4, hipMemcpyHostToDevice, s));
    idx->last_route.store(route_code(CMR_ROUTE_SORTED), std::memory_order_relaxed);
    // Several queries: scan + sort of query i + 1 run while the 12 N bytes of query i cross the link on a second stream
    // (two result sets, two event pairs; one query: no second stream, no events).  Nothing synchronises per query.
    const int nset = nq > 1 ? 2 : 1;
    if (nset > 1) { rc = call.open_second(); if (rc) return rc; }
    Workspace* const wc = call.ws2;      // its stream carries the copies
    DevBuf* ids_buf[2] = {&ws->d_ids, wc ? &wc->d_ids : nullptr};
    DevBuf* sc_buf[2] = {&ws->d_scores, wc ? &wc->d_scores : nullptr};
    hipEvent_t sorted[2] = {nullptr, nullptr}, copied[2] = {nullptr, nullptr};
    struct Ev { hipEvent_t* a; hipEvent_t* b; ~Ev() { for (int i = 0; i < 2; ++i) { if (a[i]) (void)hipEventDestroy(a[i]); if (b[i]) (void)hipEventDestroy(b[i]); } } } evs{sorted, copied};
    for (int i = 0; i < nset; ++i) {
        HIP_TRY(ids_buf[i]->ensure((size_t)n * 8));
        HIP_TRY(sc_buf[i]->ensure((size_t)n * 4));
        if (nset > 1) {
            HIP_TRY(hipEventCreateWithFlags(&sorted[i], hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&copied[i], hipEventDisableTiming));
        }
    }
    hipStream_t sc = wc ? wc->stream : s;
    auto copy_out = [&](int qi) -> int {         // a pageable destination may hold the calling thread until the copy is done:
        const int b = qi % nset;                  // issued only AFTER the next query's scan + sort are in the queue
        if (nset > 1) HIP_TRY(hipStreamWaitEvent(sc, sorted[b], 0));
        HIP_TRY(hipMemcpyAsync(out_ids + (size_t)qi * n, ids_buf[b]->p, (size_t)n * 8, hipMemcpyDeviceToHost, sc));
        HIP_TRY(hipMemcpyAsync(out_scores + (size_t)qi * n, sc_buf[b]->p, (size_t)n * 4, hipMemcpyDeviceToHost, sc));
        if (nset > 1) HIP_TRY(hipEventRecord(copied[b], sc));
        return CMR_OK;
    };
    auto body = [&]() -> int {
        for (int qi = 0; qi < nq; ++qi) {
            const int b = qi % nset;
            if (nset > 1 && qi >= nset) HIP_TRY(hipStreamWaitEvent(s, copied[b], 0));      // the set's previous contents are on the host
            int rc_ = scores_enqueue(idx, ws, (const float*)ws->d_q.p + (size_t)qi * idx->dim, 1, (float*)ws->d_out.p, n);
            if (rc_) return rc_;
            HIP_TRY(cmr_launch_sort_scores((const float*)ws->d_out.p, n, kernel_id_base(idx), ws->d_cand.p, (int64_t*)ids_buf[b]->p, (float*)sc_buf[b]->p, s));
            rc_ = remap_ids_enqueue(idx, (int64_t*)ids_buf[b]->p, n, s);
            if (rc_) return rc_;
            if (nset > 1) HIP_TRY(hipEventRecord(sorted[b], s));
            if (qi > 0) { rc_ = copy_out(qi - 1); if (rc_) return rc_; }
        }
        return copy_out(nq - 1);
    };
    rc = body();
    const hipError_t e1 = hipStreamSynchronize(s);
    const hipError_t e2 = sc != s ? hipStreamSynchronize(sc) : hipSuccess;
    if (rc) return rc;
    if (e1 != hipSuccess || e2 != hipSuccess) return fail(CMR_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    for (int qi = 0; qi < nq; ++qi) {
        if (out_max) out_max[qi] = out_scores[(size_t)qi * n];
        if (out_min) out_min[qi] = out_scores[(size_t)qi * n + n - 1];
    }
    return check_query_flag(ws);
}

int32_t cmr_index_rescore(cmr_index_t* idx, const float* q, int32_t nq, const int64_t* cand, int32_t n_cand, int32_t k,
                          int64_t* out_ids, float* out_scores) {
    if (!idx || !q || !cand || !out_ids || !out_scores) return fail(CMR_ERR_INVALID, "NULL argument");
    if (nq <= 0 || n_cand <= 0 || k <= 0) return fail(CMR_ERR_INVALID, "nq, n_cand, k must be > 0");
    if (n_cand > 4096) return fail(CMR_ERR_UNSUPPORTED, "n_cand %d > 4096", n_cand);
    if (k > n_cand) k = n_cand;
    SyncCall call(idx);
    int rc = call.open();
    if (rc) return rc;
    Workspace* const ws = call.ws;
    hipStream_t const s = call.s;
    // a shard with a block table: candidates come in as global ids, the kernel works on local rows (base 0), its output
    // ids are translated back on the stream
    std::vector<int64_t> local_cand;
    if (!idx->single_block()) {
        local_cand.resize((size_t)nq * n_cand);
        for (size_t i = 0; i < local_cand.size(); ++i) local_cand[i] = to_local_row(idx, cand[i]);
        cand = local_cand.data();
    }
    const long long base = kernel_id_base(idx);
    {   // few queries (the exact re-scorer behind a top-100 search): candidates + queries go down in ONE copy from the pinned
        // buffer (the kernel re-reads each query once per candidate: not across the link), the results are written straight
        // into its mapped half — one copy, one launch, one sync instead of two copies each way
        const size_t q_bytes = (size_t)nq * idx->dim * 4, c_bytes = ((size_t)nq * n_cand * 8 + 255) & ~(size_t)255, i_bytes = (size_t)nq * k * 8,
                     s_bytes = (size_t)nq * k * 4;
        if (idx->zero_copy && i_bytes + s_bytes <= kZeroCopyMax && c_bytes + q_bytes <= 16 * kZeroCopyMax) {
            const size_t o_ids = 0, o_sc = o_ids + i_bytes;      // (no header: nothing reports through this buffer)
            MappedStage m;
            { int rc_ = stage_mapped(ws, o_sc + s_bytes, c_bytes + q_bytes, false, &m); if (rc_) return rc_; }
            HIP_TRY(ws->d_cand.ensure(c_bytes + q_bytes));
            char* const h = m.h; char* const d = m.d;
            const size_t o_in = m.o_in;
            memcpy(h + o_in, cand, (size_t)nq * n_cand * 8);
            memcpy(h + o_in + c_bytes, q, q_bytes);
            HIP_TRY(hipMemcpyAsync(ws->d_cand.p, h + o_in, c_bytes + q_bytes, hipMemcpyHostToDevice, s));
            HIP_TRY(cmr_launch_rescore(idx->dtype, idx->corpus, idx->shadow, idx->dim, idx->dpad, idx->n, base,
                                       (const float*)((const char*)ws->d_cand.p + c_bytes), nq, (const int64_t*)ws->d_cand.p, n_cand, k,
                                       (int64_t*)(d + o_ids), (float*)(d + o_sc), s));
            { int rc_ = remap_ids_enqueue(idx, (int64_t*)(d + o_ids), (long long)nq * k, s); if (rc_) { (void)hipStreamSynchronize(s); return rc_; } }
            HIP_TRY(hipStreamSynchronize(s));
            memcpy(out_ids, h + o_ids, i_bytes);
            memcpy(out_scores, h + o_sc, s_bytes);
            return CMR_OK;
        }
    }
    HIP_TRY(ws->d_q.ensure((size_t)nq * idx->dim * 4));
    HIP_TRY(ws->d_cand.ensure((size_t)nq * n_cand * 8));
    HIP_TRY(ws->d_ids.ensure((size_t)nq * k * 8));
    HIP_TRY(ws->d_scores.ensure((size_t)nq * k * 4));
    HIP_TRY(hipMemcpyAsync(ws->d_q.p, q, (size_t)nq * idx->dim * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(ws->d_cand.p, cand, (size_t)nq * n_cand * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(cmr_launch_rescore(idx->dtype, idx->corpus, idx->shadow, idx->dim, idx->dpad, idx->n, base, (const float*)ws->d_q.p, nq,
                               (const int64_t*)ws->d_cand.p, n_cand, k, (int64_t*)ws->d_ids.p, (float*)ws->d_scores.p, s));
    { int rc_ = remap_ids_enqueue(idx, (int64_t*)ws->d_ids.p, (long long)nq * k, s); if (rc_) { (void)hipStreamSynchronize(s); return rc_; } }
    HIP_TRY(hipMemcpyAsync(out_ids, ws->d_ids.p, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_scores, ws->d_scores.p, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return CMR_OK;
}

int32_t cmr_index_round_stats(cmr_index_t* idx, float* max_row_norm, float* max_round_err) {
    if (!idx || !max_row_norm || !max_round_err) return fail(CMR_ERR_INVALID, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    float h[2] = {0.0f, 0.0f};
    HIP_TRY(hipMemcpy(h, idx->d_stats, sizeof(h), hipMemcpyDeviceToHost));
    *max_row_norm = h[0];
    *max_round_err = h[1];
    return CMR_OK;
}

int32_t cmr_index_prefilter_stats(cmr_index_t* idx, float* max_row_norm, float* max_quant_err) {
    if (!idx || !max_row_norm || !max_quant_err) return fail(CMR_ERR_INVALID, "NULL argument");
    std::shared_lock<std::shared_mutex> lk(idx->mu);
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    std::lock_guard<std::mutex> pl(idx->pipe_mu);
    float h[2] = {0.0f, 0.0f};
    if (idx->q8c.q8) {
        HIP_TRY(hipStreamSynchronize(idx->q8c.stream));
        HIP_TRY(hipMemcpy(h, idx->q8c.stats, sizeof(h), hipMemcpyDeviceToHost));
    }
    *max_row_norm = h[0];
    *max_quant_err = h[1];
    return CMR_OK;
}

int32_t cmr_index_get_rows(cmr_index_t* idx, const int64_t* ids, int64_t n, float* out) {
    if (!idx || (n > 0 && (!ids || !out))) return fail(CMR_ERR_INVALID, "NULL argument");
    if (n <= 0) return CMR_OK;
    SyncCall call(idx);
    int rc = call.open();
    if (rc) return rc;
    Workspace* const ws = call.ws;
    hipStream_t const s = call.s;
    HIP_TRY(ws->d_cand.ensure((size_t)n * 8));
    HIP_TRY(ws->d_out.ensure((size_t)n * idx->dim * 4));
    std::vector<int64_t> local_ids;
    if (!idx->single_block()) {      // global ids -> local rows through the block table (a row this shard does not hold: -1, as an id outside [base, base + n))
        local_ids.resize((size_t)n);
        for (int64_t i = 0; i < n; ++i) local_ids[i] = to_local_row(idx, ids[i]);
        ids = local_ids.data();
    }
    HIP_TRY(hipMemcpyAsync(ws->d_cand.p, ids, (size_t)n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(cmr_launch_gather_rows(idx->dtype, idx->corpus, idx->dim, idx->dpad, idx->n, kernel_id_base(idx), (const int64_t*)ws->d_cand.p, n,
                                   (float*)ws->d_out.p, s));
    HIP_TRY(hipMemcpyAsync(out, ws->d_out.p, (size_t)n * idx->dim * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return CMR_OK;
}

int32_t cmr_merge_topk(const int64_t* ids, const float* scores, int32_t S, int32_t nq, int32_t k, int64_t* out_ids,
                       float* out_scores) {
    // Host-side final merge (north_star: "host-side final merge" after the RCCL all-gather).
    // Pure index/compare work on S*k <= a few hundred candidates per query; same tie rule.
    if (!ids || !scores || !out_ids || !out_scores) return fail(CMR_ERR_INVALID, "NULL argument");
    if (S <= 0 || nq <= 0 || k <= 0) return fail(CMR_ERR_INVALID, "S, nq, k must be > 0");
    std::vector<std::pair<float, int64_t>> v;
    v.reserve((size_t)S * k);
    for (int q = 0; q < nq; ++q) {
        v.clear();
        for (int s = 0; s < S; ++s)
            for (int j = 0; j < k; ++j) {
                const size_t o = ((size_t)s * nq + q) * k + j;
                if (ids[o] >= 0) v.emplace_back(scores[o] + 0.0f, ids[o]);
            }
        std::sort(v.begin(), v.end(), [](const std::pair<float, int64_t>& a, const std::pair<float, int64_t>& b) {
            return a.first > b.first || (a.first == b.first && a.second < b.second);
        });
        for (int j = 0; j < k; ++j) {
            const bool have = (size_t)j < v.size();
            out_ids[(size_t)q * k + j] = have ? v[j].second : -1;
            out_scores[(size_t)q * k + j] = have ? v[j].first : -INFINITY;
        }
    }
    return CMR_OK;
}

int32_t cmr_merge_topk_dev(int32_t device_id, const int64_t* ids_dev, const float* scores_dev, int32_t S, int32_t nq, int32_t k,
                           int64_t* out_ids_dev, float* out_scores_dev, void* stream) {
    if (!ids_dev || !scores_dev || !out_ids_dev || !out_scores_dev) return fail(CMR_ERR_INVALID, "NULL argument");
    if (S <= 0 || nq <= 0 || k <= 0) return fail(CMR_ERR_INVALID, "S, nq, k must be > 0");
    int rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_merge_shards(ids_dev, scores_dev, S, nq, k, out_ids_dev, out_scores_dev, (hipStream_t)stream));
    return CMR_OK;
}

int32_t cmr_profile_enable(cmr_index_t* idx, int32_t on) {
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    std::lock_guard<std::mutex> g(idx->prof_mu);
    idx->prof_on = on != 0;
    idx->prof_every = on > 1 ? on : 1;
    idx->prof_seq = 0;
    return CMR_OK;
}

int32_t cmr_profile_collect(cmr_index_t* idx, int64_t* n_launches, double* total_ms, double* bytes_per_launch) {
    if (!idx) return fail(CMR_ERR_INVALID, "NULL index");
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    std::vector<ProfEvent> ev;
    double bytes = 0;
    {
        std::lock_guard<std::mutex> g(idx->prof_mu);
        ev.swap(idx->prof_events);
        bytes = idx->prof_bytes;
    }
    double ms = 0;
    for (ProfEvent& pe : ev) {
        HIP_TRY(hipEventSynchronize(pe.b));
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, pe.a, pe.b));
        ms += t;
        (void)hipEventDestroy(pe.a);
        (void)hipEventDestroy(pe.b);
    }
    if (n_launches) *n_launches = (int64_t)ev.size();
    if (total_ms) *total_ms = ms;
    if (bytes_per_launch) *bytes_per_launch = bytes;
    return CMR_OK;
}

}  // extern "C"

// ---- the call families that share nothing but the index and what is above: a header each, included by this file only
#include "row_filter.h"      // the row filter; filtered top-k and threshold search
#include "range_host.h"      // range search and count, filtered or not
#include "exact_host.h"      // exact fp32 search
#include "mmr_host.h"        // diversified top-k
#include "mutate_host.h"     // remove, update, truncate

