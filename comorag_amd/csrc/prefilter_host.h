// Host side of the certified int8 pre-filter of the pipelined 16-bit scan and nothing else.  Its state is in
// index_state.h, its sizes and pass-level conditions in plan_pass (search_plan.h).  Included by api.hip only.
#pragma once
#include "search_plan.h"

namespace {

// Brings the int8 companion of the corpus up to date (idx->pipe_mu held): (re)allocated for the corpus buffer's capacity, rows [rows rounded down
// to a panel, n) quantised on `s`.  false: no companion — it is released whole, the route stays off for this capacity, the sticky HIP error is cleared.
bool q8_ensure_companion(cmr_index* idx, hipStream_t s) {
    Q8Companion& c = idx->q8c;
    if (c.failed_cap == idx->cap_panels) return false;
    auto give_up = [&]() { c.release(); c.failed_cap = idx->cap_panels; (void)hipGetLastError(); return false; };
    if (c.q8 && c.cap_panels != idx->cap_panels) {      // the corpus buffer was replaced: so is the companion, like grow() once nothing in flight reads the old one
        if (hipDeviceSynchronize() != hipSuccess) return give_up();
        c.release();
    }
    if (!c.q8) {
        const size_t bytes = (size_t)idx->cap_panels * CMR_PANEL_ROWS * idx->dpad;
        if (hipMalloc((void**)&c.stats, 2 * sizeof(float)) != hipSuccess) { c.stats = nullptr; return give_up(); }
        if (hipEventCreateWithFlags(&c.ready, hipEventDisableTiming) != hipSuccess) { c.ready = nullptr; return give_up(); }
        if (hipMalloc(&c.q8, bytes + CMR_CORPUS_SLACK) != hipSuccess) { c.q8 = nullptr; return give_up(); }
        if (hipMalloc((void**)&c.scales, (size_t)idx->cap_panels * CMR_PANEL_ROWS * sizeof(float2)) != hipSuccess) { c.scales = nullptr; return give_up(); }
        if (hipMemsetAsync((char*)c.q8 + bytes, 0, CMR_CORPUS_SLACK, s) != hipSuccess || hipMemsetAsync(c.stats, 0, 2 * sizeof(float), s) != hipSuccess) return give_up();
        c.cap_panels = idx->cap_panels;
    }
    c.rows = std::min(c.rows, idx->n);
    if (c.rows < idx->n) {
        const long long panel0 = c.rows / CMR_PANEL_ROWS;
        if (cmr_launch_q8_quantise(idx->dtype, idx->corpus, idx->dpad, panel0, idx->npanels() - panel0, idx->n, c.q8, c.scales, c.stats, s) != hipSuccess ||
            hipEventRecord(c.ready, s) != hipSuccess) return give_up();
        c.stream = s; c.rows = idx->n;
    }
    return true;
}

// May this pipelined call take the pre-filter?  Plain calls without min / max outputs (the int8 pass cannot give the 16-bit extremes) of one
// narrow pass on a non-empty 16-bit index, when the option says so; what a single pass adds to these conditions is in plan_pass.
constexpr bool kPrefilterAuto = true;      // prefilter = -1 (the default): scans of 1 ms and longer take it (DESIGN 4.14 has the measurement)
int prefilter_eligible(const cmr_index* idx, bool threshold, bool minmax, int nq, bool may_prefilter) {
    if (!may_prefilter || threshold || minmax || idx->dtype == CMR_F32 || idx->n <= 0 || nq > idx->narrow_max()) return 0;
    if (idx->prefilter < 0) return kPrefilterAuto && !idx->short_scan() ? 1 : 0;
    return idx->prefilter;      // 0: off, 1: on, 2: on, with a filter that keeps every row
}

// Step 1 of a pre-filtered pass, on the pre-phase stream behind prep_queries: the scratch as planned, the companion's last rows (quantised
// on another stream, maybe), the int8 query parts — and the arguments of the pass's launches.
int q8_prepare(cmr_index* idx, Workspace* ws, const PassPlan& p, const float* q_dev, hipStream_t sp, CmrQ8Args& f) {
    const Q8Companion& c = idx->q8c;
    DevBuf* const w = ws->q8.buf;
    HIP_TRY(ws->q8.ensure(p.bytes.q8));
    if (sp != c.stream) HIP_TRY(hipStreamWaitEvent(sp, c.ready, 0));
    HIP_TRY(cmr_launch_q8_pack_queries(idx->dtype, q_dev, p.nqp, idx->dim, idx->dpad, p.tiles, c.stats, w[Q8_QPACK].p, (float4*)w[Q8_QCONST].p, sp));
    f.dtype = idx->dtype; f.dpad = idx->dpad; f.nqt = p.g.nqt; f.cap = p.g.cap; f.grid = p.g.grid; f.rescore_grid = p.rescore_grid;
    f.corpus = idx->corpus; f.q8 = c.q8; f.scales = c.scales; f.qfrag = ws->qfrag.p; f.qpack = w[Q8_QPACK].p; f.qconst = (const float4*)w[Q8_QCONST].p;
    f.nrows = idx->n; f.npanels = (int)idx->npanels(); f.nq = p.nqp; f.k = p.k; f.keep_all = p.prefilter == 2 ? 1 : 0;
    f.cand_row = (unsigned*)w[Q8_CAND].p; f.n_cand = (unsigned*)w[Q8_NCAND].p; f.keep = (unsigned*)w[Q8_KEEP].p; f.tau_tight = (float*)w[Q8_TAU].p;
    f.wrec = w[Q8_WREC].p; f.wcnt = (unsigned*)w[Q8_WCNT].p; f.wave_cap = f.keep_all ? 0 : p.wave_cap;
    f.pair = w[Q8_PAIR].p; f.pair_cnt = (unsigned*)w[Q8_PAIRCNT].p; f.pcap = p.pair_cap;
    if (p.sample_q8) {
        f.s_grid = p.level[1].grid; f.s_run = p.s_run; f.s_stride = p.s_stride; f.s_nruns = p.s_nruns;
        f.s_wrec = w[Q8_SWREC].p; f.s_wcnt = (unsigned*)w[Q8_SWCNT].p; f.s_wave_cap = p.s_wave_cap;
        f.s_pair = w[Q8_SPAIR].p; f.s_pair_cnt = (unsigned*)w[Q8_SPAIRCNT].p; f.s_pcap = p.s_pair_cap;
    }
    return CMR_OK;
}
// Level 1 of a pre-filtered pass with record lists, on the pre-phase stream where the bf16 level-1 scan and its merge stand otherwise: the
// filter body over the sample's runs against the level-0 keys `tau0`, its records sorted by query, and per query the key of the k-th largest
// lower bound (or the level-0 key, whichever is larger) into `tau_out` — what the main filter, the tightening, the re-score and the merge
// then take as tau_init.  The sample's buffers are touched on this stream only, so stream order is all they need.
int q8_sample(cmr_index* idx, CmrQ8Args& f, const u64* tau0, u64* tau_out, size_t cnt_bytes, hipStream_t sp) {
    f.s_tau0 = tau0; f.s_tau_out = tau_out;
    HIP_TRY(hipMemsetAsync(f.s_pair_cnt, 0, cnt_bytes, sp));
    HIP_TRY(cmr_launch_q8_filter(f, sp, true));
    HIP_TRY(cmr_launch_q8_bucket(f, sp, true));
    HIP_TRY(cmr_launch_q8_select(f, sp));
    idx->prefilter_sample_active = 1;
    return CMR_OK;
}
// Step 2, on the scan stream in the place of the main scan: the filter, with that scan's thresholds and lists; the diagnostics now read this pass
int q8_filter(cmr_index* idx, CmrQ8Args& f, const CmrScanArgs& a, hipStream_t sm) {
    f.tau_init = a.tau_init; f.lists = a.lists; f.cnt = a.cnt;
    HIP_TRY(cmr_launch_q8_filter(f, sm));
    idx->q8_last = Q8LastPass{f.n_cand, f.pair_cnt, f.nq, f.pcap, f.wcnt, f.grid * CMR_SCAN_WAVES, f.wave_cap, f.s_grid > 0 ? f.s_pair_cnt : nullptr, f.s_pcap};
    idx->prefilter_active = 1;
    return CMR_OK;
}
// Step 3, on the merge stream in front of the merge: the waves' records sorted into the queries' lists, thresholds tightened into keep[], its bits
// listed, those rows scored into the merge's lists
int q8_rescore(const CmrQ8Args& f, hipStream_t sq) {
    if (f.pcap > 0) {
        HIP_TRY(cmr_launch_q8_bucket(f, sq));
        HIP_TRY(cmr_launch_q8_tighten(f, sq));
    }
    HIP_TRY(hipMemsetAsync(f.n_cand, 0, sizeof(unsigned), sq));
    HIP_TRY(cmr_launch_q8_expand(f, sq));
    HIP_TRY(cmr_launch_q8_rescore(f, sq));
    return CMR_OK;
}
// the profiler's bytes of a pre-filtered launch (elsewhere: algorithmic_bytes): what the filter reads — the companion, its scales, the two int8 query parts
double prefilter_bytes(const cmr_index* idx, const PassPlan& p) {
    return (double)idx->npanels() * CMR_PANEL_ROWS * (idx->dpad + sizeof(float2)) + (double)2 * p.tiles * idx->dpad * 32;
}

// The counters of the last pre-filtered pass, read once the pipeline has drained (0 before any such pass, -1: the read failed).  candidates:
// rows it handed to the re-score; pairs: the (row, query) records in the queries' lists, over all queries; pair_overflow: queries that were offered more than
// the capacity; wave_overflow: waves of the filter's grid that offered more records than their area holds; sample_pairs / sample_overflow: pairs and
// pair_overflow of the int8 sample's lists (0 where the pass had no int8 sample).
enum class Q8Counter { candidates, pairs, pair_overflow, wave_overflow, sample_pairs, sample_overflow };
long long q8_read_counter(const cmr_index* cidx, Q8Counter what) {
    cmr_index* idx = const_cast<cmr_index*>(cidx);
    if (cmr_set_device(idx->device)) return -1;
    std::lock_guard<std::mutex> pl(idx->pipe_mu);
    const Q8LastPass& L = idx->q8_last;
    const bool sample = what == Q8Counter::sample_pairs || what == Q8Counter::sample_overflow;
    const unsigned* const src = what == Q8Counter::candidates ? L.ncand : what == Q8Counter::wave_overflow ? L.wcnt : sample ? L.s_paircnt : L.paircnt;
    const unsigned pcap = (unsigned)(sample ? L.s_pcap : L.pcap);
    std::vector<unsigned> h(what == Q8Counter::candidates ? 1 : (size_t)std::max(what == Q8Counter::wave_overflow ? (L.wave_cap > 0 ? L.nw : 0) : L.nq, 0));
    if (!src || h.empty()) return 0;
    for (hipStream_t st : idx->pipe.st) if (st && hipStreamSynchronize(st) != hipSuccess) return -1;
    if (hipMemcpy(h.data(), src, h.size() * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    if (what == Q8Counter::candidates) return (long long)h[0];
    if (what == Q8Counter::wave_overflow) return (long long)std::count_if(h.begin(), h.end(), [&](unsigned c) { return c > (unsigned)L.wave_cap; });
    long long stored = 0, overflowed = 0;
    for (unsigned c : h) { stored += std::min(c, pcap); overflowed += c > pcap ? 1 : 0; }
    return what == Q8Counter::pairs || what == Q8Counter::sample_pairs ? stored : overflowed;
}

}  // namespace
