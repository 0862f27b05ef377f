// How a search is routed and shaped — pure host arithmetic on (index shape, options, request): which path a call takes, how a
// batch splits into corpus passes, and everything one pass needs before its first HIP call (plan_pass).  Nothing here calls
// HIP, touches a Workspace or changes the index; api.hip enqueues what is planned here.
#pragma once
#include <numeric>

#include "index_state.h"

bool cmr_ring_audit_ok(int dtype, int nqt, int cap, int ring, int mode);  // ring_audit.cpp (generated at build); mode: 0 top-k, 1 scores, 2 top-k with the finishing stage
static const long long kMaxMergeLists = 4096;                    // merge_query_kernel: W <= 16 * MERGE_THREADS
// The int8 sample of a pre-filtered pass (prefilter_sample; DESIGN 4.14 has the sweeps): auto on / off, and its auto shape — level-1 panels
// (no merge behind it, so no list cap), panels per wave, panels of the bf16 level 0 whose threshold the sample tests against
constexpr bool kPrefilterSampleAuto = false;     // off: at equal reserve it never beat the bf16 sampling by the project's rule
static const long long kQ8SamplePanels = 8192;
static const int kQ8SampleRun = 16;
static const int kQ8SampleLevel0 = 64;

namespace {

// Scan geometry for a pass of `nq` queries with top-`k`.
int make_geom(const cmr_index* idx, int nq, int k, bool topk, CmrScanGeom* g) {
    const int max_nqt = cmr_scan_max_nqt(idx->dtype, idx->dpad);
    if (max_nqt == 0) return cmr_fail(CMR_ERR_UNSUPPORTED, "dim %d too large for the LDS-resident query tile (dtype %d)", idx->dim, idx->dtype);
    g->dtype = idx->dtype;
    g->dpad = idx->dpad;
    g->nqt = (nq > 32 && max_nqt >= 2) ? 2 : 1;
    g->cap = (topk && k > 32) ? 256 : 128;
    const int ks = idx->ks();
    g->ring = (ks % 16 == 0) ? 16 : 8;
    if (idx->force_ring == 8 || (idx->force_ring == 16 && ks % 16 == 0)) g->ring = idx->force_ring;
    const int mode = topk ? 0 : 1;
    g->asm_ring = cmr_ring_audit_ok(g->dtype, g->nqt, g->cap, g->ring, mode) ? 1 : 0;
    if (idx->force_asm == 0) g->asm_ring = 0;
    if (idx->force_asm == 1 && !cmr_ring_audit_ok(g->dtype, g->nqt, g->cap, g->ring, mode))
        return cmr_fail(CMR_ERR_UNSUPPORTED, "CMR_SCAN_ASM_RING=1 but variant (dtype %d nqt %d cap %d ring %d) failed the ISA audit", g->dtype, g->nqt, g->cap, g->ring);
    if (!cmr_scan_geom(g)) return cmr_fail(CMR_ERR_UNSUPPORTED, "scan geometry does not fit LDS (dpad %d nqt %d)", idx->dpad, g->nqt);
    const int bpc = g->lds <= 80 * 1024 ? 2 : 1;
    long long grid = (idx->npanels() + CMR_SCAN_WAVES - 1) / CMR_SCAN_WAVES;  // >= 1 panel per wave
    grid = std::min<long long>(grid, (long long)idx->n_cu * bpc);
    if (idx->force_grid > 0) grid = std::min<long long>(grid, idx->force_grid);
    g->grid = (int)std::max<long long>(grid, 1);
    return CMR_OK;
}

double algorithmic_bytes(const cmr_index* idx, int nq, int k) {
    return (double)idx->npanels() * CMR_PANEL_ROWS * idx->dpad * elem_size(idx->dtype) + (double)nq * idx->dim * 4 + (double)nq * k * 12;
}

// Every wave (workgroup, for the wide kernel) scans a contiguous range of floor/ceil(npanels / W) panels and
// the kernel ends with the longest range: at 1 M rows on 256 CUs that is 16 panels against a mean of 15.3,
// a 5 % tail during which HBM idles.  The scan is bandwidth-bound, not CU-bound, so giving up a few workgroups
// (<= 1/8) for the W that minimises the padded panel count ceil(npanels / W) * W is free.  (Not for the wide
// kernel: it is MFMA-bound and wants every CU.)
int balanced_grid(long long npanels, int grid, int lists_per_wg) {
    // a dropped workgroup is not quite free (64 of 256 CUs cost ~3 % of the bandwidth): charge 0.05 % each
    int best = grid;
    double best_cost = -1.0;
    for (int g = grid; g >= std::max(1, grid - grid / 8); --g) {
        const long long W = (long long)g * lists_per_wg;
        const double cost = (double)((npanels + W - 1) / W * W) * (1.0 + 0.0005 * (grid - g));
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = g; }
    }
    return best;
}

// ---- one pass of the fused search: request -> plan

// narrow: <= 64 queries on the narrow kernel (scan_kernel).  wide: the register-resident wide kernel (scan_wide_kernel).
// quad: a batch of more than one narrow pass on the query-split grid of the NARROW kernel (scan_kernel, qgroups): the
// caller picks the streams as for a wide pass; geometry, lists and sampling are the narrow kernel's, one set per group
enum class Route { narrow, wide, quad };

struct PassRequest {
    int nqp = 0, k = 0;
    Route route = Route::narrow;
    bool has_min_score = false;      // threshold search: the caller's bound is every query's initial threshold
    bool single_stream = false;      // pre-phase, scan and merge on ONE stream (a synchronous caller)
    bool pipelined = false;          // the pre-phase has a stream of its own
    int reserve_cus = 0;             // CUs the main scan leaves free (< 0: by corpus size)
    int prefilter = 0;               // the call may take the int8 pre-filter (prefilter_eligible, prefilter_host.h: 1; 2: with a filter that keeps every row) if the pass is eligible
    bool masked = false;             // filtered search (cmr_index_search_masked*): the narrow chain on the masked scan variant — no finishing stage, no pre-filter
    bool masked_each = false;        // with masked: every query of the pass has allow words of its own (cmr_index_search_masked_each*)
};

struct PassPlan {
    int nqp = 0, k = 0;
    bool wide = false;
    CmrScanGeom g{};                 // the main scan's, g.grid = its launch grid (all query groups)
    bool fin = false;                // scan with the finishing stage: no sampling launches, no merge of its own
    bool masked = false;             // every scan of the pass (sampling levels and main) is the masked variant over the caller's allow words
    bool masked_each = false;        // ... the per-query variant: a block of allow words per query
    int prefilter = 0;               // 1 | 2: the int8 filter in the place of the main scan, the re-score in front of the merge (W: the re-score's lists)
    int rescore_grid = 0;
    int pair_cap = 0;                // pre-filter: hit records per query for the threshold tightening (0: none, every hit is re-scored)
    int wave_cap = 0;                // pre-filter: hit records per wave of the filter's grid (0 exactly when pair_cap is)
    // pre-filter with record lists: level 1 is the int8 sample — the filter body over s_nruns runs of s_run panels, run g at panel g * s_stride
    // (>= s_run), one per wave of level[1].grid workgroups, then bucket and select; level[1] holds its panels and grid, no lists (Wl = 0)
    bool sample_q8 = false;
    int s_run = 0, s_stride = 0, s_nruns = 0, s_wave_cap = 0, s_pair_cap = 0;
    int G = 1;                       // query groups of the query-split grid
    int n_levels = 0;                // sampling passes in front of the main scan
    struct Level { long long panels; int grid, Wl, clog, stride; } level[2] = {};      // grid: launch grid (all groups); Wl: candidate lists per query
    bool single_level = false;
    bool tau_in_scan = false;        // the single level hands its lists to the main scan (no merge launch between the two)
    int reserve_cus = 0;
    int lists_per_wg = CMR_SCAN_WAVES;
    int NQ = 0, W = 0, Ws = 0, tiles = 0, NQA = 0;      // query slots per group, main / sampling lists per query, query tiles, query slots over all groups
    int fin_first = 0, fin_wgs = 0, fin_mul = 1, fin_dcap = 0, fin_spin = 0;
    struct { size_t qfrag, lists, cnt, mm, s_lists, s_cnt, s_mm, tau, fin_ctl, fin_pmax, fin_tau, fin_mm, fin_dense, q8[Q8_NBUF]; } bytes = {};
};

int plan_pass(const cmr_index* idx, const PassRequest& rq, PassPlan* out) {
    PassPlan& p = *out;
    p = PassPlan{};
    const int nqp = rq.nqp, k = rq.k;
    const bool wide = rq.route == Route::wide, quad = rq.route == Route::quad;
    p.nqp = nqp; p.k = k; p.wide = wide;
    if (rq.masked && (wide || quad || rq.prefilter)) return cmr_fail(CMR_ERR_INVALID, "a filtered pass is a narrow pass without the pre-filter");
    if (rq.masked_each && !rq.masked) return cmr_fail(CMR_ERR_INVALID, "per-query allow words belong to a filtered pass");
    p.masked = rq.masked; p.masked_each = rq.masked_each;
    CmrScanGeom& g = p.g;
    const long long npanels = idx->npanels();
    int rc = make_geom(idx, quad ? std::min(nqp, idx->narrow_max()) : nqp, k, true, &g);
    if (rc) return rc;
    const int G = quad ? (nqp + g.nqt * 32 - 1) / (g.nqt * 32) : 1;      // query groups
    p.G = G;
    // the groups' twins re-read each corpus block from L2: default cache policy for them, non-temporal for single-group scans
    g.stream_default_policy = idx->stream_nt < 0 ? (G > 1 ? 1 : 0) : (idx->stream_nt ? 0 : 1);
    const int lists_per_wg = wide ? 1 : CMR_SCAN_WAVES;
    p.lists_per_wg = lists_per_wg;
    // A synchronous caller's handful of queries (everything on ONE stream) on a corpus beyond the single-launch path: the scan
    // with the finishing stage — no sampling launches, no merge of its own (scan_kernel MODE_FIN; 2 M x 768 bf16 rows, one
    // query: pack 5 + sample 15 + scan 471 + merge 46 us before, pack + scan with ~10 us of finishing after)
    bool fin = !rq.masked && idx->scan_fin && !idx->no_sample && !wide && G == 1 && !rq.has_min_score && rq.single_stream && g.nqt == 1 && nqp <= idx->fin_max_q &&
               k <= 64 && npanels >= 4096 && npanels >= (long long)idx->n_cu * 2 * CMR_SCAN_WAVES;      // (every wave of the grid has a first panel)
    if (fin) {
        // scan_fin_cap = 256: longer lists than k asks for — the panels a wave scans before the thresholds arrive go to its lists whole (32 keys
        // per query and panel, two to three panels), and a 128-key list is then "nearly full" at the first real candidate (a compaction)
        if ((idx->fin_cap == 256 || idx->fin_cap == 128) && idx->fin_cap > g.cap) {
            CmrScanGeom g2 = g;
            g2.cap = idx->fin_cap;
            if (cmr_scan_geom(&g2) && g2.lds + CMR_FIN_LDS <= 160 * 1024) g = g2;      // (else: the geometry's own lists)
        }
        const bool ok = cmr_ring_audit_ok(g.dtype, 1, g.cap, g.ring, 2);
        if (idx->force_asm == 1 && !ok) fin = false;       // the caller insists on the hand-counted ring: only audited variants
        if (g.lds + CMR_FIN_LDS > 160 * 1024 || g.grid > 512) fin = false;
        else g.asm_ring = (ok && idx->force_asm != 0) ? 1 : 0;
    }
    p.fin = fin;
    // Sampling passes (large corpora).  Level i scans S_i strided panels and takes the exact k-th
    // best of that sample per query as the threshold of the next level / of the main scan.  Any
    // subset's k-th best is a valid lower bound of the global k-th best, so results are unchanged;
    // what changes is that only ~S_{i+1}*k/S_i scores per query ever reach the candidate lists
    // (instead of k*ln(rows/k) per wave and query), which keeps every merge at a few thousand keys.
    //   S0 = max(512, 32k) rows, S1 = clamp(N/32, 8*S0, 128*S0) rows (only when N >= 128 Ki rows)
    // Narrow kernel: one sampled panel per wave = one candidate list per panel, and merge_query_kernel takes at
    // most 4096 lists, so S1 is capped there (k > 32 on multi-million-row shards would otherwise overrun it).
    // Wide kernel: the sampling workgroups split the sampled panels among them (one list per workgroup and query).
    // Certified int8 pre-filter: a narrow pass with thresholds from tau_init (16-bit index, no threshold search: tested by prefilter_eligible)
    const bool prefilter = rq.prefilter && !wide && G == 1 && !fin;
    // ... whose level-1 threshold is drawn from the int8 companion: only where the pass keeps record lists (the select step reads them)
    const bool sample_q8 = prefilter && rq.prefilter == 1 && idx->pf_tighten && idx->pf_pair_cap > 0 && npanels >= 4096 &&
                           (idx->pf_sample < 0 ? kPrefilterSampleAuto : idx->pf_sample == 1);
    long long level_panels[2] = {0, 0};
    long long bf16_level1 = 0;       // the bf16 level 1 this shape would sample (what the reserve rule was measured with)
    int n_levels = 0;
    bool single_level = false;
    // threshold search (min_score): the caller's bound is the initial threshold of every query — already selective, so no
    // sampling passes
    if (!idx->no_sample && npanels >= 256 && !rq.has_min_score && !fin) {
        // (int8 sample: a larger level 0 — its threshold decides how many of the sample's pairs become records; k panels at least, as everywhere)
        const long long s0 = sample_q8 ? std::max<long long>(idx->pf_sample_level0 > 0 ? idx->pf_sample_level0 : kQ8SampleLevel0, k) : std::max<long long>(16, k);      // panels
        // A handful of queries on a mid-size corpus (what a synchronous caller issues) is a chain of dependent launches
        // around a short scan: ONE sampling level of 128 panels instead of two saves a scan + merge pair (~45 us of a
        // 0.4 ms call at 1 M rows).  Its threshold lets ~k * npanels / 128 scores per query through — a few slow-path
        // entries per wave as long as queries x panels stays small.
        // (not with the pre-filter: a pipelined pass hides the second level, and every row a loose threshold lets through is a gather)
        single_level = !wide && !prefilter && idx->single_level && k <= 32 && nqp <= 8 && npanels >= 4096 && (long long)nqp * npanels <= idx->single_level_max;
        level_panels[n_levels++] = single_level ? 128 : s0;
        if (npanels >= 4096 && !single_level) {
            // wide kernel: 256 queries share a workgroup, so ANY of 8 tiles beating its threshold stalls all four waves at
            // the next barrier — a 4x larger level-1 sample (N/32 rows up to 512 x level 0) took the main pass from 4.09 to
            // 3.76 ms at 10 M rows; the sample itself is cheap there (256 queries per pass over it)
            // pre-filter: every row the threshold lets through costs a gather of 96 cache lines, so the sample is as large as the
            // merge allows (10 M rows, 2560 -> 4096 panels: 330 K -> 216 K kept rows per batch, step 2.00 -> 1.90 ms)
            const long long maxmul = idx->sample_maxmul > 0 ? idx->sample_maxmul : (wide ? 512 : prefilter ? kMaxMergeLists : 128);
            const long long b0 = std::max<long long>(16, k);
            long long s1 = std::min<long long>(std::max<long long>(npanels / idx->sample_div, 8 * b0), maxmul * b0);
            if (!wide) s1 = std::min<long long>(s1, kMaxMergeLists);
            if (s1 < npanels / 2) bf16_level1 = s1;
            if (sample_q8) {
                // int8 sample: half the bytes per row and no merge behind it, so the merge's list cap does not bind; a forced size is taken as
                // it is, up to every panel (8 * s0 <= 1024 < npanels / 2 here: auto always has its level 1)
                level_panels[n_levels++] = idx->pf_sample_panels > 0 ? std::min<long long>(idx->pf_sample_panels, npanels)
                                                                     : std::min<long long>(std::max<long long>(npanels / idx->sample_div, 8 * s0), kQ8SamplePanels);
            } else if (bf16_level1) level_panels[n_levels++] = bf16_level1;
        }
    }
    p.n_levels = n_levels;
    p.single_level = single_level;
    p.sample_q8 = sample_q8 && n_levels == 2;
    // (the largest bf16 sampling pass: the int8 sample has no candidate lists and runs one workgroup per 8 runs)
    const long long max_sample = std::max(level_panels[0], p.sample_q8 ? 0 : level_panels[1]);
    int reserve_cus = rq.reserve_cus;
    if (reserve_cus < 0) {
        if (!max_sample) reserve_cus = 0;
        else if (wide) {
            // Pipelined mode, wide kernel: a sampling workgroup owns a CU (512 registers per wave), so the next batch's
            // pre-phase runs on reserved CUs.  Workgroups are bound to a shader engine (8 CUs) at dispatch and then wait for
            // a free CU THERE: with 240 + 16 workgroups in flight some engines were full and a 16-workgroup sampling pass
            // waited 4.4 ms for the main scan to end (kernel trace), while 224 + 32 — one free CU in every one of the 32
            // engines — flows.  So the reserve is one CU per shader engine; the main pass is matrix-pipe-bound and pays for
            // them in proportion (4.2 -> 4.6 ms at 10 M rows), about what a serialised pre-phase would cost.
            reserve_cus = 32;
        } else if (prefilter && idx->scan_us() >= 1250.0) {
            // Pipelined mode, int8 pre-filter over a corpus of ~4.9 M x 768 16-bit rows and more: the filter is limited by the CUs it gets,
            // not by HBM (10 M rows: 1.31 ms alone on 256 CUs, 1.35 / 1.45 / 1.51 ms in the pipeline on 240 / 222 / 192), and the free
            // CUs carry BOTH the next batch's pre-phase and the previous batch's merge-stream chain — neither a sampling workgroup nor
            // a re-score workgroup finds registers beside a filter workgroup.  Kernel traces at 10 M rows: on 32 free CUs
            // the level-1 sampling scan takes 436 us and still ends 146 us (46 at worst) before the filter it runs under; on 16 it no
            // longer does, and an int8 sample there starves the re-score (0.2 -> 1 ms).  The pre-phase on 32 CUs is ~650 us in a row, so it
            // needs a filter of that length: 32 against 64 CUs, median ms per step — 10 M rows 1.50 / 1.57 (B = 33: 1.41 / 1.44, B = 8:
            // 1.30 / 1.30, B = 1: 1.26 / 1.26), 5 M rows 0.823 / 0.829, but 4 M rows 0.694 / 0.686: there, and below, the rule by size stays.
            reserve_cus = 32;
        } else {
            // Pipelined mode, reserve chosen by size: the next batch's pre-phase has to fit under this scan (~6 TB/s).
            // It is ~200 us of dependent small kernels plus ~200 us per round of its largest sampling pass on the
            // reserved CUs (every sampling workgroup stages the 96 KiB query tile and its loads crawl while the scan
            // saturates HBM: at 10 M rows 320 workgroups on 26 CUs took 2.3 ms and overran the scan by 90 us, on 34
            // CUs they fit).  Reserved CUs cost the scan bandwidth only at short scans (64 of 256: ~3 % at 1 M rows,
            // nothing measurable at 10 M).  Measured at 1 / 1.25 / 2.5 / 5 / 10 M rows x 768 bf16.
            const long long rounds = (long long)((0.7 * idx->scan_us() - 200.0) / 200.0);
            const long long wgs = std::max<long long>(1, (max_sample + lists_per_wg - 1) / lists_per_wg) * G;
            reserve_cus = rounds >= 1 ? (int)std::min<long long>(64, std::max<long long>(8, (wgs + rounds - 1) / rounds)) : 64;
        }
    }
    p.reserve_cus = reserve_cus;
    // workgroups of a sampling pass over spn panels, and candidate lists it produces
    auto sample_grid = [&](long long spn) -> int {
        if (!wide) return (int)((spn + lists_per_wg - 1) / lists_per_wg);
        // at most 48 sampled panels per workgroup: a level-1 pass pushes ~1 key per query and panel, and a candidate list
        // that fills up (CAP - 32 keys) costs a compaction, whose global loads drain the workgroup's DMA ring.  More
        // workgroups than (reserved) CUs simply run in rounds.
        const int cap_wgs = rq.pipelined && reserve_cus > 0 ? reserve_cus : idx->n_cu;
        return (int)std::min<long long>(spn, std::max<long long>(cap_wgs, (spn + 47) / 48));
    };
    const int Ws = max_sample ? std::max(sample_grid(level_panels[0]), n_levels > 1 && !p.sample_q8 ? sample_grid(level_panels[1]) : 0) * lists_per_wg : 0;
    int NQ, W, tiles;
    if (wide) {
        // register-resident queries: 4 waves x 2 (768-d) or 1 (1024-d) tiles of 32, one list row per
        // (workgroup, query); one workgroup per CU
        const int nqb = cmr_wide_queries(idx->dtype, idx->dpad);
        g.nqt = 1;
        g.grid = (int)std::max<long long>(1, std::min<long long>(npanels, idx->n_cu));
        if (reserve_cus > 0 && g.grid > idx->n_cu / 2) g.grid = std::max(g.grid - reserve_cus, idx->n_cu / 2);
        NQ = nqb; W = g.grid; tiles = nqb / 32;
    } else if (G > 1) {
        // query-split grid: G workgroups (one per query tile) share every virtual workgroup's panel ranges; the virtual grid is
        // a multiple of 8 so that the G twins land on one XCD (scan_kernel) and G x virtual grid fills the CUs once
        if (reserve_cus > 0 && g.grid > idx->n_cu / 2) g.grid = std::max(g.grid - reserve_cus, idx->n_cu / 2);
        int vg = g.grid / G;
        if (vg >= 8) vg &= ~7;
        g.grid = std::max(vg, 1);
        NQ = g.nqt * 32; W = g.grid * CMR_SCAN_WAVES; tiles = G * g.nqt;
    } else {
        if (reserve_cus > 0 && g.grid > idx->n_cu / 2) g.grid = std::max(g.grid - reserve_cus, idx->n_cu / 2);
        if (!idx->force_grid) g.grid = balanced_grid(npanels, g.grid, CMR_SCAN_WAVES);
        NQ = g.nqt * 32; W = g.grid * CMR_SCAN_WAVES; tiles = g.nqt;
    }
    // Pre-filter: the filter takes the main scan's grid; the candidate lists are the re-score's — a fixed grid of small workgroups, one
    // per CU by default (4 waves, ~70 registers, 5 KiB of LDS: they fit beside a filter workgroup; its gathers are 16-byte pieces,
    // one cache line each, and more CUs keep more of them in flight: 92 -> 256 workgroups 2.05 -> 2.01 ms per step at 10 M rows,
    // nothing beyond).  At most 1024 x 4 = the merge's 4096 lists.
    if (prefilter) {
        p.prefilter = rq.prefilter;
        p.rescore_grid = idx->pf_rescore_wgs > 0 ? idx->pf_rescore_wgs : std::min(idx->n_cu, 1024);
        W = p.rescore_grid * cmr_q8_rescore_waves();
        p.pair_cap = (rq.prefilter == 1 && idx->pf_tighten) ? idx->pf_pair_cap : 0;
        p.bytes.q8[Q8_QPACK] = (size_t)2 * tiles * (idx->dpad / 32) * 1024;
        p.bytes.q8[Q8_QCONST] = (size_t)NQ * sizeof(float4);
        p.bytes.q8[Q8_CAND] = (size_t)idx->cap_panels * CMR_PANEL_ROWS * sizeof(unsigned);      // (cap_panels: candidate rows and keep masks follow the corpus buffer)
        p.bytes.q8[Q8_NCAND] = sizeof(unsigned);
        // the waves' record areas: by default they hold together what the queries' lists hold, in multiples of a wave's 64 lanes
        const long long fw = (long long)g.grid * CMR_SCAN_WAVES;
        p.wave_cap = !p.pair_cap ? 0 : idx->pf_wave_cap > 0 ? idx->pf_wave_cap : (int)std::min<long long>(1 << 20, (((long long)NQ * p.pair_cap + fw - 1) / fw + 63) / 64 * 64);
        p.bytes.q8[Q8_WREC] = std::max<size_t>((size_t)fw * p.wave_cap * 16, 16);
        p.bytes.q8[Q8_WCNT] = (size_t)fw * sizeof(unsigned);
        p.bytes.q8[Q8_PAIR] = std::max<size_t>((size_t)NQ * p.pair_cap * 16, 16);
        p.bytes.q8[Q8_PAIRCNT] = (size_t)NQ * sizeof(unsigned);
        p.bytes.q8[Q8_KEEP] = (size_t)idx->cap_panels * sizeof(unsigned);
        p.bytes.q8[Q8_TAU] = (size_t)NQ * sizeof(float);
        if (p.sample_q8) {
            // runs of s_run panels spread evenly; a sample that does not fit with gaps (forced: beyond npanels / 2) is laid end to end — full
            // coverage, the last run cut by the corpus' end.  One wave per run; the area of a wave holds 1 / 16 of its run's (row, query)
            // pairs by default (the level-0 threshold of 64 panels lets ~2 % through), a hit beyond it is dropped
            const long long s1 = level_panels[1];
            const long long run = std::min<long long>(idx->pf_sample_run > 0 ? idx->pf_sample_run : kQ8SampleRun, s1);
            long long nruns = (s1 + run - 1) / run, stride = npanels / nruns;
            if (stride < run) { stride = run; nruns = std::min(nruns, (npanels + run - 1) / run); }
            p.s_run = (int)run; p.s_stride = (int)stride; p.s_nruns = (int)nruns;
            p.s_wave_cap = idx->pf_sample_wave_cap > 0 ? idx->pf_sample_wave_cap : (int)std::min<long long>(1 << 20, (run * CMR_PANEL_ROWS * NQ / 16 + 63) / 64 * 64);
            p.s_pair_cap = p.pair_cap;
            const long long sw = (nruns + CMR_SCAN_WAVES - 1) / CMR_SCAN_WAVES * CMR_SCAN_WAVES;
            p.bytes.q8[Q8_SWREC] = (size_t)sw * p.s_wave_cap * 16;
            p.bytes.q8[Q8_SWCNT] = (size_t)sw * sizeof(unsigned);
            p.bytes.q8[Q8_SPAIR] = (size_t)NQ * p.s_pair_cap * 16;
            p.bytes.q8[Q8_SPAIRCNT] = (size_t)NQ * sizeof(unsigned);
        }
    }
    const int NQA = G * NQ;          // query slots of the pass over all groups
    p.NQ = NQ; p.W = W; p.Ws = Ws; p.tiles = tiles; p.NQA = NQA;
    // sample passes and the main pass use separate list buffers: in pipelined mode the next batch's
    // sampling runs while this batch's main scan still owns `lists`
    p.bytes.qfrag = (size_t)tiles * g.ks * 1024;
    p.bytes.lists = (size_t)W * NQA * g.cap * 8;
    p.bytes.cnt = (size_t)W * NQA * 4;
    p.bytes.mm = (size_t)W * NQA * 8;
    p.bytes.s_lists = (size_t)Ws * NQA * g.cap * 8;
    p.bytes.s_cnt = (size_t)Ws * NQA * 4;
    p.bytes.s_mm = (size_t)Ws * NQA * 8;
    p.bytes.tau = (size_t)2 * NQA * 8;
    for (int lv = 0; lv < n_levels; ++lv) {
        PassPlan::Level& L = p.level[lv];
        const long long spn = level_panels[lv];
        L.panels = spn;
        if (lv == 1 && p.sample_q8) {      // (no candidate lists; the runs are in s_run / s_stride / s_nruns)
            L.grid = (p.s_nruns + CMR_SCAN_WAVES - 1) / CMR_SCAN_WAVES; L.Wl = 0; L.clog = 0; L.stride = p.s_stride;
            continue;
        }
        L.grid = sample_grid(spn);
        L.Wl = L.grid * lists_per_wg;
        L.grid *= G;                               // (query-split grid: every group samples the same panels)
        // chunks of 8 consecutive panels (384 KiB at 768-d bf16), chunk starts spread evenly over the corpus: a sampling
        // workgroup that hops one panel at a time pays a TLB miss / DRAM page run per 48 KiB (measured 11-14 us per
        // panel under a saturating main scan)
        L.clog = spn >= 64 ? 3 : 0;
        const long long nchunks = (spn + (1 << L.clog) - 1) >> L.clog;
        L.stride = (int)(npanels / nchunks);
    }
    // the one sampling level of ONE or TWO queries (what a synchronous caller issues): the main scan's workgroups derive
    // the thresholds from these lists themselves (scan_kernel) — no merge launch between the two scans.  Every
    // workgroup reads the whole sample of its queries (32 KiB each): with 8 queries that costs more than the merge
    // launch it saves (1 M rows: 371 -> 405 us per call), with one it wins (344 -> 330 us)
    // (not with the pre-filter: its filter and re-score take the thresholds from tau_init)
    p.tau_in_scan = n_levels > 0 && single_level && idx->tau_in_scan && NQ == 32 && nqp <= 2 && k <= 64 && !p.prefilter;
    if (G > 1) g.grid *= G;
    if (fin) {
        p.fin_dcap = idx->fin_dense;
        p.fin_spin = idx->fin_spin;
        p.bytes.fin_ctl = CMR_FIN_CTL * sizeof(int);
        p.bytes.fin_pmax = (size_t)32 * CMR_FIN_SLOTS * 8;
        p.bytes.fin_tau = 32 * 8;
        p.bytes.fin_mm = (size_t)32 * 512 * 8;
        p.bytes.fin_dense = (size_t)32 * p.fin_dcap * 8;
        // the first workgroups through their first panels supply the thresholds: 64 of them (512 maxima; the 64th of 256 is through at a
        // third of the time the slowest of 128 takes), 128 from 4 M rows up (a looser threshold lets k x panels / maxima keys per query through)
        p.fin_first = std::min(g.grid, idx->n_cu);      // (181 registers: one workgroup per CU)
        p.fin_wgs = std::min(std::min(idx->fin_suppliers > 0 ? idx->fin_suppliers : (npanels >= 131072 ? 128 : 64), CMR_FIN_SLOTS / CMR_SCAN_WAVES), p.fin_first);
        // the golden-ratio multiple of the grid, moved to the next value coprime with it: the first fin_wgs workgroups' ranges spread evenly
        p.fin_mul = 1;
        for (int m = std::max(1, (int)(g.grid * 0.6180339887)); m < g.grid; ++m)
            if (std::gcd(m, g.grid) == 1) { p.fin_mul = m; break; }
    }
    return CMR_OK;
}

// "last_route" (include/comorag_hip.h): path | sampling levels << 4 | tau_in_scan << 6 | single 128-panel level << 7 | query tiles per workgroup << 8 |
// threshold search << 10 | filtered << 12 | filtered with per-query masks << 13 (| CMR_ROUTE_MORE_PASSES where the batch is cut into several passes: plan_and_enqueue_pass)
long long route_code(int path, int n_levels = 0, bool tau_in_scan = false, bool single_level = false, int nqt = 1, bool threshold = false) {
    return (long long)path | ((long long)n_levels << 4) | ((long long)(tau_in_scan ? 1 : 0) << 6) | ((long long)(single_level ? 1 : 0) << 7) | ((long long)nqt << 8) |
           ((long long)(threshold ? 1 : 0) << 10);
}
long long route_code(const PassPlan& p, bool threshold) {
    const int path = p.wide ? CMR_ROUTE_WIDE : p.G > 1 ? CMR_ROUTE_QUERY_SPLIT : p.fin ? CMR_ROUTE_FIN : CMR_ROUTE_CHAIN;
    return route_code(path, p.n_levels, p.tau_in_scan, p.single_level, p.g.nqt, threshold) | (p.masked ? CMR_ROUTE_FILTERED : 0) | (p.masked_each ? CMR_ROUTE_FILTERED_EACH : 0);
}

// ---- a batch splits into passes

// Batches of more than one narrow pass: which kernel runs them, and how many queries it takes per corpus pass (0 = narrow passes).
// wide_mode 1: the register-resident wide kernel only (768-d: 256 queries, 1024-d: 128; 16-bit indexes) — other shapes run
// narrow passes; 2: always the query-split grid of the narrow kernel (4 tiles of 64 — or of 32 where the LDS holds one tile —
// in one pass, any dim and dtype); 0 (default): the wide kernel where it exists, the query-split grid everywhere else.
// Measured (profiles/r4_measurements.md, MI355X, 768-d bf16): at 10 M rows the wide kernel runs B = 256 in 3.79 ms, the grid in
// 6.24 (its twins stay in step only partly: 43 % L2 hits of an ideal 75 %, the rest comes over the fabric), four narrow passes in
// 9.4; at B = 128 the grid is level with the wide kernel (3.47 vs 3.26 ms; 0.39 vs 0.47 on a 1.25 M-row shard).
bool wide_pass_is_quad(const cmr_index* idx) {
    if (idx->wide_mode == 2) return true;
    if (idx->wide_mode == 1) return false;
    return cmr_wide_queries(idx->dtype, idx->dpad) == 0;
}
// A pass of 65 .. 128 queries over a SHORT scan (< 1 ms at the streaming rate: shards up to ~4 M x 768 bf16 rows) runs on the
// query-split grid although the shape has a wide kernel: two query tiles per corpus block are within what an XCD's L2 hands on
// (0.39 vs 0.47 ms at 1.25 M rows, B = 128; at 10 M rows the wide kernel wins, 3.26 vs 3.47 — profiles/r4_wide_routes_ab.txt)
bool short_two_tile_pass(const cmr_index* idx, int left) {
    if (idx->wide_mode != 0 || idx->no_wide || cmr_wide_queries(idx->dtype, idx->dpad) == 0) return false;
    if (cmr_scan_max_nqt(idx->dtype, idx->dpad) < 2 || left <= 64 || left > 128) return false;
    return idx->short_scan();
}
int wide_pass_queries(const cmr_index* idx) {
    if (idx->no_wide) return 0;
    if (!wide_pass_is_quad(idx)) return cmr_wide_queries(idx->dtype, idx->dpad);
    return 4 * idx->narrow_max();
}

// The passes of a batch of nq queries, in order: `for (PassSplit ps(idx, nq); ps.next();)` with ps.q0 / ps.nqp / ps.route of
// the current pass.  The synchronous and the pipelined search both iterate this, so they route a batch alike.
struct PassSplit {
    const cmr_index* idx;
    const int nq, narrow, wideq;
    const bool quad;
    int q0 = 0, nqp = 0;
    Route route = Route::narrow;
    PassSplit(const cmr_index* i, int nq_) : idx(i), nq(nq_), narrow(i->narrow_width(nq_)), wideq(wide_pass_queries(i)), quad(wide_pass_is_quad(i)) {}
    bool any_wide() const { return wideq > 0 && nq > narrow; }      // does the batch hold a pass that is not narrow (its first one, then)
    bool wide_streams() const { return route != Route::narrow; }    // wide kernel or query-split grid: the pipeline's wide streams
    bool next() {
        q0 += nqp;
        if (q0 >= nq) return false;
        const int left = nq - q0;
        const bool wide = wideq > 0 && left > narrow;          // more than one narrow pass left: go wide
        nqp = std::min(wide ? wideq : narrow, left);
        route = !wide ? Route::narrow : (quad || short_two_tile_pass(idx, left)) ? Route::quad : Route::wide;
        return true;
    }
};

// 0: the general pack / [sample] / scan / merge chain; 1: single launch, <= 1024 rows; 2: single launch, hierarchical
// selection (<= 16 queries, k <= 64, up to 64 K rows while workgroups x k <= 1024) — see tiny_search_kernel
// (a filtered search never asks: the single-launch kernels take no allow words, search_masked_enqueue plans narrow passes only)
int small_path_kind(const cmr_index* idx, int nq, int k, bool threshold_search) {
    if (idx->no_tiny || threshold_search || idx->n <= 0 || nq > 16 || k > CMR_MAX_K) return 0;
    if (idx->npanels() > idx->small_max_panels) return 0;
    if (!idx->small_operands_fit()) return 0;
    const int kind = cmr_tiny_kind(nq, (int)idx->npanels(), k, idx->tiny_multi, idx->small_max_panels);
    return (kind == 2 && idx->no_small) ? 0 : kind;
}

}  // namespace
