// State of one index (cmr_index_t) and of the calls in flight on it: device buffers, per-stream workspaces, the pipeline's
// streams and slots, the quantities every route decision derives from the index shape, and the guards of the synchronous entry
// points.  Included by api.hip only (one translation unit owns the index); the headers that hold its call families (search_plan.h,
// prefilter_host.h, row_filter.h, range_host.h, exact_host.h, mmr_host.h, mutate_host.h) are parts of that unit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <shared_mutex>
#include <vector>

#include "../../include/comorag_hip.h"
#include "cmr_kernels.h"
#include "cmr_internal.h"
#include "combine.h"

#define CMR_DT_F32 0
#define CMR_PANEL_ROWS 32
#define CMR_SCAN_WAVES 8
#define CMR_CORPUS_SLACK (128 * 1024)

namespace {

int elem_size(int dtype) { return dtype == CMR_F32 ? 4 : 2; }
int round_up(int x, int m) { return (x + m - 1) / m * m; }
long long panels_of(long long rows) { return (rows + CMR_PANEL_ROWS - 1) / CMR_PANEL_ROWS; }

// Scratch of the exact search (cmr_index_search_exact): stage-1 candidate lists [nq][kc] (ids, 16-bit scan scores), the re-score's
// keys [nq][kc], its per-query arrival counters (zeroed when allocated, re-armed by the kernel) and the outputs of the sync call.
struct ExactScratch {
    DevBuf ids, sc, part, arrive, oids, osc, oex;
    void release() { ids.release(); sc.release(); part.release(); arrive.release(); oids.release(); osc.release(); oex.release(); }
};

// ---- certified int8 pre-filter (host side: prefilter_host.h).  The int8 companion of the corpus — int8 blocks, (scale, error norm) per row,
// (max ||x||, max error norm) — covers rows [0, rows) of a corpus buffer of cap_panels panels; a call that uses it brings it up to date first.  Freed by release() only.
struct Q8Companion {
    void* q8 = nullptr; float2* scales = nullptr; float* stats = nullptr;
    long long cap_panels = 0, rows = 0;
    long long failed_cap = -1;           // the companion of a corpus buffer of this many panels could not be allocated: the route stays off
    hipEvent_t ready = nullptr; hipStream_t stream = nullptr;      // the event behind the last quantise launch, and the stream it was recorded on
    size_t bytes(int dpad) const { return q8 ? (size_t)cap_panels * CMR_PANEL_ROWS * (dpad + sizeof(float2)) + CMR_CORPUS_SLACK : 0; }
    void release() { (void)hipFree(q8); (void)hipFree(scales); (void)hipFree(stats); if (ready) (void)hipEventDestroy(ready); *this = Q8Companion{}; }
};
// A workspace's buffers of a pre-filtered pass, sized by plan_pass (PassPlan::bytes.q8[]): int8 query parts, queries' constants, candidate
// rows and their counter, the filter's (row, ub, lb, query) records per wave of its grid and their counters, the same records per query
// and their counters, row mask per panel, tightened thresholds; the int8 sample's records per wave of ITS grid and per query, with
// their counters (areas of their own: the slot's wrec / pair may still be read by the previous batch's bucket step and tightening on
// the merge stream while the pre-phase stream samples for the next one).
enum Q8Buf { Q8_QPACK, Q8_QCONST, Q8_CAND, Q8_NCAND, Q8_WREC, Q8_WCNT, Q8_PAIR, Q8_PAIRCNT, Q8_KEEP, Q8_TAU, Q8_SWREC, Q8_SWCNT, Q8_SPAIR, Q8_SPAIRCNT, Q8_NBUF };
struct Q8Scratch {
    DevBuf buf[Q8_NBUF];
    bool pf_prev = false;                // the workspace's last pass ran the re-score, which reads qfrag / tau on the merge stream
    hipError_t ensure(const size_t (&bytes)[Q8_NBUF]) { for (int i = 0; i < Q8_NBUF; ++i) if (hipError_t e = buf[i].ensure(bytes[i])) return e; return hipSuccess; }
    void release() { for (DevBuf& b : buf) b.release(); }
};
// candidate counter, nq pair counters and their capacity, nw wave counters and their capacity; the int8 sample's pair counters and capacity
struct Q8LastPass {
    const unsigned* ncand = nullptr; const unsigned* paircnt = nullptr; int nq = 0, pcap = 0; const unsigned* wcnt = nullptr; int nw = 0, wave_cap = 0;
    const unsigned* s_paircnt = nullptr; int s_pcap = 0;
};

// Scratch of one in-flight search.  One per stream (searches on a stream are serialised by it).
struct Workspace {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DevBuf qfrag, lists, cnt, mm, flag, tau, s_lists, s_cnt, s_mm, arrive;
    DevBuf fin_ctl, fin_pmax, fin_tau, fin_dense, fin_mm;
    bool fin_ctl_armed = false;      // scan with the finishing stage (cmr_launch_scan_fin)
    // host-API staging
    DevBuf d_q, d_ids, d_scores, d_min, d_max, d_cand, d_out;
    DevBuf d_mask;               // cmr_index_search_masked: the call's allow words (a workspace per concurrent call, so a mask per call); cmr_index_search_masked_each: [nq][n_words]
    DevBuf d_lists;              // cmr_index_search_ids: the call's CSR offsets and row ids [offsets (nq + 1) | ids]; its words are built into d_mask, at most 64 queries' at a time
    // synchronous search: queries in, (ids | scores | min | max | non-finite flag) out through ONE pinned host buffer and
    // one copy each way — five pageable D2H copies cost more than the search of a small corpus
    DevBuf d_pack;
    DevBuf m_ids, m_sc, m_rows, m_gram;   // diversified top-k: a call's candidates [nq, F] (ids, scores), their local rows, their pair scores [nq, F, F]
    DevBuf r_cnt, r_counts, r_hits;   // range search:(query, tile) counters / offsets, per-query counts, a group's [keys a | keys b | rows a | rows b | histograms]
    Q8Scratch q8;                // certified int8 pre-filter
    ExactScratch x;              // cmr_index_search_exact
    int* flag_ptr = nullptr;     // the non-finite-query flag the kernels set: flag.p, or the head of d_pack for the host API
    // Synchronous host API with mapped results: the word (device view of the pinned buffer, bytes 4..7) that the search's LAST kernel sets
    // once its results are written — 1: final, 2: the finishing stage overflowed and the merge recorded in `lazy` is still due.  Offered by
    // cmr_index_search_begin; a route that can honour it (single-launch search, scan with the finishing stage) sets done_used, and
    // cmr_index_search_finish then polls the word instead of waiting for the stream (5.5 us per call: tools/probe/poll_probe.hip).
    int* done_ptr = nullptr;
    bool done_used = false;
    struct LazyMerge {
        bool due = false;
        const u64* lists = nullptr; const int* cnt = nullptr; int W = 0, NQ = 0, cap = 0, nqp = 0, k = 0; const float2* mm = nullptr; long long id_base = 0;
        int64_t* ids = nullptr; float* scores = nullptr; float* mn = nullptr; float* mx = nullptr; const int* state = nullptr;
    } lazy;
    void* h_pin = nullptr;
    void* h_pin_dev = nullptr;   // the same buffer as the device sees it (mapped, fine-grained)
    size_t h_pin_cap = 0;
    hipError_t ensure_pin(size_t need) {
        if (need <= h_pin_cap) return hipSuccess;
        if (h_pin) { hipError_t e = hipHostFree(h_pin); if (e != hipSuccess) return e; h_pin = nullptr; h_pin_dev = nullptr; h_pin_cap = 0; }
        const size_t want = std::max(need, h_pin_cap * 2);
        hipError_t e = hipHostMalloc(&h_pin, want, hipHostMallocDefault);
        if (e != hipSuccess) return e;
        e = hipHostGetDevicePointer(&h_pin_dev, h_pin, 0);
        if (e != hipSuccess) { (void)hipHostFree(h_pin); h_pin = nullptr; return e; }
        h_pin_cap = want;
        return hipSuccess;
    }
    void release() {
        qfrag.release(); lists.release(); cnt.release(); mm.release(); flag.release(); tau.release();
        s_lists.release(); s_cnt.release(); s_mm.release(); arrive.release();
        fin_ctl.release(); fin_pmax.release(); fin_tau.release(); fin_dense.release(); fin_mm.release();
        d_q.release(); d_ids.release(); d_scores.release(); d_min.release(); d_max.release(); d_cand.release(); d_out.release();
        d_mask.release();
        d_lists.release();
        d_pack.release();
        m_ids.release(); m_sc.release(); m_rows.release(); m_gram.release();
        r_cnt.release(); r_counts.release(); r_hits.release();
        q8.release();
        x.release();
        if (h_pin) (void)hipHostFree(h_pin);
        h_pin = nullptr; h_pin_dev = nullptr; h_pin_cap = 0;
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

struct ProfEvent { hipEvent_t a, b; };

constexpr size_t kMappedAppendMax = 128 * 1024;  // appends up to this many bytes of fp32 rows are read by the convert kernel from mapped host memory (BASELINE config 4 appends 25 rows x 768 = 75 KiB per cycle)
constexpr size_t kMappedPlanMax = 64 * 1024;     // a row update through that buffer: its plan (16 bytes per replaced row) lies behind the rows
constexpr size_t kMappedPinBytes = 256 + kMappedAppendMax + kMappedPlanMax;      // [flag, 256 | rows | plan]
constexpr size_t kZeroCopyMax =256 * 1024;   // synchronous host API: queries / results up to this size are mapped, not copied

struct PipeSlot { Workspace ws; hipEvent_t pre_done = nullptr, scan_done = nullptr, main_done = nullptr; bool used = false; };
#define CMR_PIPE_SLOTS 4
// sp / sm / sm2: pre-phase and main scans of batches of <= 64 queries (with CU masks: sm, sm2 on n_cu - 64 CUs, sp on the other
// 64); wp / wm: the same for wide batches (no masks: the wide kernel is matrix-pipe-bound and wants every CU); sq: candidate
// merges and whatever the caller appends behind a batch (no mask: its small workgroups fit beside a scan workgroup on any CU)
// usp / usm / uwp / uwm: unmasked twins of sp / sm / wp / wm, created with them — scans of a millisecond and longer run there
// (pipe_cu_mask = -1): the masks pay where ramp, tail and packet gaps are a visible share of a step, and cost a long scan CUs.
// Every stream of the pipeline is an element of `st`: whoever destroys or synchronises "all of them" loops over the array.
// st[sq] doubles as the "pipeline exists" marker.
struct Pipe {
    enum Stream { sp, sm, sm2, wp, wm, wm2, usp, usm, uwp, uwm, sq, n_streams };
    hipStream_t st[n_streams] = {};
    PipeSlot slot[CMR_PIPE_SLOTS]; unsigned next = 0; int nslots = 2; unsigned nscan = 0, nwscan = 0; int scan_cus = 0, wide_cus = 0; int last_masked = 0;
    void destroy_streams() { for (hipStream_t& s : st) if (s) { (void)hipStreamDestroy(s); s = nullptr; } }
};

}  // namespace

struct cmr_index {
    int device = 0;
    int dim = 0, dpad = 0, dtype = 0;
    uint32_t flags = 0;
    int n_cu = 256;
    long long n = 0;             // rows
    long long cap_panels = 0;    // allocated panels
    void* corpus = nullptr;      // panel-major blocks (+ slack)
    float* shadow = nullptr;     // optional fp32 row-major [cap_rows, dim]
    std::shared_mutex mu;        // searches shared, append/destroy exclusive
    std::mutex ws_mu;
    std::vector<Workspace*> free_ws;            // for the synchronous host API
    std::map<hipStream_t, Workspace*> stream_ws;  // for the _dev API
    DevBuf stage;                // append staging; row removal stages its chunks here too (both hold the exclusive lock)
    DevBuf rm_buf;               // row removal: [info (kept rows, first removed row) | keep words | kept_before | uploaded ids]
    int rm_stage_panels = 0;     // remove_stage_panels: panels the staging buffer of a removal holds (0: 64 MiB worth; at least 2)
    long long rm_chunks_last = 0;   // read-only ("remove_chunks_last"): chunks the corpus pass of the last removal ran (0: nothing moved)
    long long upd_stage_rows = 0;   // update_stage_rows: fp32 rows a staged chunk of a row update holds (0: 256 MiB worth, like the append's; a set value also keeps the call off the mapped buffer)
    long long upd_chunks_last = 0;  // read-only ("update_chunks_last"): chunks the last row update wrote (0: nothing written)
    // range search: range_block_queries — queries per materialised score block (0: as many as 2 GiB of scores hold);
    // range_scratch_hits — hits compacted and sorted at once (0: 1 GiB of scratch worth, 24 bytes a hit); read-only range_blocks_last /
    // range_groups_last — blocks and groups the last range search ran
    int range_block_queries = 0;
    long long range_scratch_hits = 0;
    std::atomic<long long> range_blocks_last{0}, range_groups_last{0};
    void* h_pin = nullptr;       // small appends / row updates: pinned, device-mapped [flag | rows | an update's plan] (exclusive lock held)
    void* h_pin_dev = nullptr;
    size_t h_pin_cap = 0;
    int* d_flag = nullptr;       // non-finite flag for appends
    // profiling
    std::mutex prof_mu;
    bool prof_on = false;
    int prof_every = 1;          // time every prof_every-th main scan (two event packets on the scan stream cost ~25 us between scans)
    unsigned prof_seq = 0;
    std::vector<ProfEvent> prof_events;
    double prof_bytes = 0.0;
    // route selectors (cmr_index_set_option, names in kOptions; results never depend on them)
    int force_ring = 0;      // scan_ring = 8 | 16
    int force_asm = -1;      // scan_asm_ring = 0 | 1
    int force_grid = 0;      // scan_grid
    int no_sample = 0;       // scan_no_sample = 1 disables the sampling pass
    int no_wide = 0;         // scan_no_wide = 1 disables the wide-batch (register-resident query) kernel
    int no_tiny = 0;         // scan_no_tiny = 1 disables the single-launch paths (search and all-scores) altogether
    long long single_level_max = 320000;   // sample_single_max: ONE sampling level while queries x panels stays at or below this
    int single_level = 1;    // sample_single = 0: small batches on mid-size corpora sample in two levels like everything else
    int tiny_multi = 1;      // tiny_multi = 0: the single-launch path always runs as one workgroup (<= 1024 rows only)
    int small_max_panels = 6144;   // small_max_panels: largest corpus (in 32-row panels) the single-launch path takes
    int no_small = 0;        // scan_no_small = 1: corpora of 1025 rows .. 64 K rows take the general path also for few queries
    int zero_copy = 1;       // zero_copy = 0: the synchronous host API copies queries / results instead of mapping them
    int dual_scan = -1;      // pipe_dual_scan: -1 (default: with the masks, for scans shorter than 1 ms) | 1 (always) | 0 (never): main scans alternate between two streams, so the next scan's workgroups take over the CUs this
                             // scan's workgroups leave (no idle gap between two scans); needs pipe_cu_mask, else the next scan would simply
                             // occupy the CUs left free for the pre-phase
    int cu_mask = -1;        // pipe_cu_mask = -1 (default on a 256-CU device: scans shorter than 1 ms) | 1 | 2 (every scan) | 0 (off): scan stream(s) with a CU mask of n_cu - 64 CUs, the pre-phase streams
                             // with the other 64 (1: mask bits interleave the XCDs — the amdgpu driver's enumeration; 2: 32 consecutive bits per XCD)
    int stream_nt = -1;      // stream_nt: -1 default (non-temporal corpus loads, default policy for the query-split grid) | 0 | 1: force
    int wide_mode = 0;       // wide_mode: batches of more than one narrow pass — 1: the register-resident wide kernel, 2: the query-split grid of the
                             // narrow kernel (up to 4 query tiles walk the same panel ranges on CUs of one XCD; any dim / dtype), 0: the measured default
    int tau_in_scan = 1;     // sample_tau_in_scan = 0: the single sampling level of a small batch is merged by a launch of its own again
    int sync_poll = 1;       // sync_poll = 0: the synchronous host API waits for the stream instead of polling the done word of its mapped result buffer
    int scan_fin = 1;        // scan_fin = 0: small synchronous batches on corpora beyond the single-launch path run the sampling / scan / merge chain
                             // instead of the scan with the finishing stage (thresholds and final selection inside the scan launch)
    int fin_dense = 16384;   // scan_fin_dense: keys per query of the finishing stage's dense candidate lists (~k x panels / 1024 beat a threshold taken
                             // from 1024 first panels: 600 at 1 M rows, 6 K at 10 M; a list that overflows hands the selection to the merge launch)
    int fin_cap = 0;         // scan_fin_cap: keys per (wave, query) list of the scan with the finishing stage (128 | 256; 0: the geometry's, by k).  256 measured: 1 M rows, 8 queries 304-309 us against 314-317, everything else level (2 M rows 548-552 against 537-548)
    int fin_suppliers = 0;   // scan_fin_suppliers: workgroups whose first panels make the threshold sample (0: 64, 128 from 4 M rows up; <= 128)
    int fin_spin = 0;        // scan_fin_spin: rounds of ~1.5 us the workgroups that do not supply thresholds wait for them before they scan without (0: they look once)
    int fin_max_q = 8;       // scan_fin_queries: largest batch the finishing stage takes (<= 16).  Measured at 768-d bf16, per call, stage / chain:
                             // 1 M rows — 1 / 2 / 4 / 8 / 16 queries 287 / 292 / 297 / 322 / 392 us against 300 / 313 / 333 / 336 / 372;
                             // 2 M rows — 520 / 523 / 525 / 538 / 589 against 563 / 560 / 577 / 588 / 615
    int dual_wide_active = 0;   // read-only ("pipe_dual_scan_wide_active"): the same for the last wide pass
    // read-only ("last_route"): how the last search / scores call planned on this index was routed (CMR_ROUTE_* in include/comorag_hip.h;
    // search_plan.h route_code).  Written by host code under the shared lock, so concurrent callers race benignly: relaxed atomic.
    std::atomic<long long> last_route{0};
    int dual_active = 0;     // read-only ("pipe_dual_scan_active"): did the last pipelined <= 64-query pass alternate between the two scan streams
    // combine (0 = off, 2..16): concurrent cmr_index_search / cmr_index_scores / cmr_index_ppr calls of up to this many queries in all share
    // ONE batched call (combine.h); combine_wait_us: the leader's gather window.  Read by the entry points before any lock.
    std::atomic<int> combine{0};
    std::atomic<long long> combine_wait_us{0};
    // combine_filtered (0 | 1): with combine on, the filtered host calls (cmr_index_search_masked, cmr_index_search_masked_each) go through the
    // combiner too and share one per-query-mask search.  Off: they never combine and never move the combiner's counters.
    std::atomic<int> combine_filtered{0};
    cmr_combine::Combiner combiner;
    long long id_base = 0;   // added to every returned row id (global ids of a row shard)
    // A row shard that took incremental appends holds several runs of consecutive global ids (cmr_index_set_id_blocks): the
    // kernels then run with base 0 and a remap launch translates their ids; candidate / row ids coming IN are translated
    // on the host.  One block = plain id_base.
    std::vector<long long> blk_local, blk_global;
    long long* d_blk = nullptr;          // [local0[nb] | global0[nb]] on the device
    std::vector<void*> blk_retired;      // earlier tables: in-flight searches may still read them (a few bytes each, freed at destroy)
    int sample_maxmul = 0;   // sample_maxmul: level-1 sample <= sample_maxmul x level 0 (0 = 128 narrow / 512 wide)
    int sample_div = 32;     // sample_div: level-1 sample = 1/sample_div of the panels (clamped to [8, 128] x level 0)
    // Certified int8 pre-filter of the pipelined 16-bit scan.  prefilter: -1 auto (kPrefilterAuto, prefilter_host.h, and a scan of 1 ms
    // or longer) | 0 off | 1 every eligible call | 2 the same with a filter that keeps every row (the re-score path alone).
    int prefilter = -1;
    int pf_rescore_wgs = 0;              // prefilter_rescore_wgs: workgroups of the re-score (0: one per CU)
    // prefilter_tighten: the k-th largest certified lower bound among a query's hits replaces its sampling threshold before the
    // re-score (0: every hit is re-scored — the kept set of the route before the tightening, the A/B arm).  prefilter_pair_cap: hit
    // records per query (16 bytes each: 16 MiB per workspace at 64 queries); a query that offers more keeps the rest directly.
    // prefilter_wave_cap: records per wave of the filter's grid, which writes them to an area of its own before they are sorted by
    // query (0: as many as the queries' lists hold, spread over the waves — plan_pass); a wave that offers more keeps the rest directly.
    int pf_tighten = 1;
    int pf_pair_cap = 16384;
    int pf_wave_cap = 0;
    // prefilter_sample: where the level-1 sampling threshold of a pre-filtered pass with record lists comes from — 1: from the int8 companion
    // (the filter body over strided runs of panels, bucket, select: DESIGN 4.14) | 0: from the bf16 panels (scan_kernel + merge, launch for
    // launch what every other route does) | -1 auto (kPrefilterSampleAuto, search_plan.h).  prefilter_sample_panels (0 = auto; a forced value
    // is taken as it is, up to every panel), prefilter_sample_run (panels per wave, 0 = auto), prefilter_sample_wave_cap (records per wave of
    // the sample's grid, 0 = auto), prefilter_sample_level0 (panels of the bf16 level 0 on this route, 0 = auto; at least k).
    int pf_sample = -1;
    int pf_sample_panels = 0;
    int pf_sample_run = 0;
    int pf_sample_wave_cap = 0;
    int pf_sample_level0 = 0;
    int prefilter_sample_active = 0;     // read-only: did the last pre-filtered pass draw its sampling threshold from the companion
    Q8Companion q8c;
    int prefilter_active = 0;            // read-only: did the last pipelined call run the pre-filter
    Q8LastPass q8_last;                  // the last pre-filtered pass's counters (the options prefilter_candidates / _pairs / _pair_overflow / _wave_overflow read them)
    int pipe_slots = 3;      // pipe_slots (2..4): batches in the pipeline.  A third slot lets the pre-phase of batch i+2 start before
                             // scan i has ended: 1 M x 768 bf16, B = 64 step 0.279 -> 0.264 ms; nothing at 10 M rows
    int reserve_cus = -1;    // pipe_reserve_cus: CUs the pipelined main scan leaves free (-1 = by corpus size, see plan_pass)
    std::mutex pipe_mu;
    Pipe pipe;
    // exact search (cmr_index_search_exact): the certificate's index-wide maxima (M_x, M_dx) on the device, updated by every
    // accepted append; stage-1 candidates per query (exact_cand, in (k, CMR_MAX_K]); per-slot scratch of the pipelined call
    float* d_stats = nullptr;
    int exact_cand = CMR_MAX_K;
    ExactScratch x_slot[CMR_PIPE_SLOTS];
    unsigned x_next = 0;

    // ---- quantities derived from the shape: one definition each
    size_t panel_bytes() const { return (size_t)CMR_PANEL_ROWS * dpad * elem_size(dtype); }
    long long npanels() const { return panels_of(n); }
    int ks() const { return dtype == CMR_F32 ? dpad / 8 : dpad / 16; }      // MFMA k-steps of one row
    // queries of one pass of the narrow kernel: two tiles of 32 where the LDS holds two and the batch has more than one
    int narrow_max() const { return cmr_scan_max_nqt(dtype, dpad) >= 2 ? 64 : 32; }
    int narrow_width(int nq) const { return nq > 32 ? narrow_max() : 32; }
    // one pass over the corpus at the streaming rate (~6 TB/s = 6.0e6 bytes per microsecond), in microseconds
    double scan_us() const { return (double)npanels() * panel_bytes() / 6.0e6; }
    // shorter than 1 ms (shards up to ~4 M x 768 bf16 rows): ramp, tail and packet gaps are a visible share of such a scan
    bool short_scan() const { return scan_us() < 1000.0; }
    bool single_block() const { return blk_local.size() <= 1; }      // no block table: the kernels add id_base themselves
    // the single-launch paths keep the packed operands of one query tile (+ 17 KiB of static LDS) in the LDS
    bool small_operands_fit() const { return (size_t)ks() * 1024 <= 143 * 1024; }
};

namespace {

// id base the kernels add themselves (0 when a block table translates afterwards)
long long kernel_id_base(const cmr_index* idx) { return idx->single_block() ? idx->id_base : 0; }

Workspace* acquire_ws(cmr_index* idx, hipStream_t user_stream, bool dev_api) {
    std::lock_guard<std::mutex> g(idx->ws_mu);
    if (dev_api && user_stream) {
        auto it = idx->stream_ws.find(user_stream);
        if (it != idx->stream_ws.end()) return it->second;
        Workspace* w = new Workspace();
        w->stream = user_stream;
        idx->stream_ws[user_stream] = w;
        return w;
    }
    if (dev_api) {  // NULL on the dev API is the legacy default stream itself (what torch's default stream is): work enqueued
                    // there is ordered with the caller's kernels on that stream, exactly as on any other stream handle
        auto it = idx->stream_ws.find(nullptr);
        if (it != idx->stream_ws.end()) return it->second;
        Workspace* w = new Workspace();
        w->stream = nullptr;
        idx->stream_ws[nullptr] = w;
        return w;
    }
    if (!idx->free_ws.empty()) { Workspace* w = idx->free_ws.back(); idx->free_ws.pop_back(); return w; }
    Workspace* w = new Workspace();
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) { delete w; return nullptr; }
    w->own_stream = true;
    return w;
}
void release_ws(cmr_index* idx, Workspace* w) {
    std::lock_guard<std::mutex> g(idx->ws_mu);
    idx->free_ws.push_back(w);
}

// The device set and a workspace taken: the pooled one of a synchronous call (dev_api = false, given back with release_ws) or the
// one that belongs to the caller's stream (dev_api = true, kept by the index).
int open_ws(cmr_index* idx, hipStream_t stream, bool dev_api, Workspace** ws) {
    int rc = cmr_set_device(idx->device);
    if (rc) return rc;
    *ws = acquire_ws(idx, stream, dev_api);
    return *ws ? CMR_OK : cmr_fail(CMR_ERR_HIP, "could not create a workspace stream");
}

// Prologue of a synchronous entry point.  Construction takes the index's shared lock (argument checks that read the index go
// between the two steps); open() sets the device and takes a pooled workspace (`ws`, its stream `s`).  Scope exit returns the
// workspace(s) and drops the lock.
struct SyncCall {
    cmr_index* idx;
    std::shared_lock<std::shared_mutex> lk;
    Workspace* ws = nullptr;
    Workspace* ws2 = nullptr;      // second workspace of a call that overlaps copies with scans (open_second)
    hipStream_t s = nullptr;
    explicit SyncCall(cmr_index* i) : idx(i), lk(i->mu) {}
    SyncCall(const SyncCall&) = delete;
    int open() {
        int rc = open_ws(idx, nullptr, false, &ws);
        if (rc) return rc;
        s = ws->stream;
        return CMR_OK;
    }
    int open_second() {
        ws2 = acquire_ws(idx, nullptr, false);
        return ws2 ? CMR_OK : cmr_fail(CMR_ERR_HIP, "could not create a copy stream");
    }
    ~SyncCall() {
        if (ws2) release_ws(idx, ws2);
        if (ws) release_ws(idx, ws);
    }
};

// Prologue of a _dev entry point, shaped like SyncCall: construction takes the shared lock, open(stream) sets the device and takes
// the workspace of the caller's stream (`ws`; it stays with the index, nothing to return); open() is for a call that needs none.
struct DevCall {
    cmr_index* idx;
    std::shared_lock<std::shared_mutex> lk;
    Workspace* ws = nullptr;
    explicit DevCall(cmr_index* i) : idx(i), lk(i->mu) {}
    DevCall(const DevCall&) = delete;
    int open() { return cmr_set_device(idx->device); }
    int open(void* stream) { return open_ws(idx, (hipStream_t)stream, true, &ws); }
};

// ws->flag_ptr points somewhere else (the header of a host API result buffer) for the enqueue calls of one scope
struct FlagOverride {
    Workspace* ws;
    int* saved;
    FlagOverride(Workspace* w, int* flag) : ws(w), saved(w->flag_ptr) { w->flag_ptr = flag; }
    FlagOverride(const FlagOverride&) = delete;
    ~FlagOverride() { ws->flag_ptr = saved; }
};

// The workspace's pinned, device-mapped buffer laid out as [results, `out_bytes` | inputs, `in_bytes`, at the next multiple of
// 256]: `h` / `d` are the host's and the device's view of it, `o_in` the offset of the inputs.  header: the first 8 bytes of
// the results are the call's non-finite flag (bytes 0..3) and done word (bytes 4..7, see wait_done_word), zeroed here.
struct MappedStage { char* h = nullptr; char* d = nullptr; size_t o_in = 0; };
int stage_mapped(Workspace* ws, size_t out_bytes, size_t in_bytes, bool header, MappedStage* m) {
    m->o_in = (out_bytes + 255) & ~(size_t)255;
    HIP_TRY(ws->ensure_pin(m->o_in + in_bytes));
    m->h = (char*)ws->h_pin;
    m->d = (char*)ws->h_pin_dev;
    if (header) memset(m->h, 0, 8);
    return CMR_OK;
}

}  // namespace
