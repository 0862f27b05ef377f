// Personalised PageRank seeded by dense-retrieval scores, on the device.
//
// Replaces, for one query, the tail of ComoRAG.graph_search_with_fact_entities (src/comorag/ComoRAG.py:1034-1044: all N
// (passage id, normalised DPR score) pairs are copied to the host, scattered one by one into `passage_weights` through
// passage_node_keys -> node_name_to_vertex_idx) and ComoRAG.run_ppr (:1086-1105: igraph's prpack personalised PageRank,
// undirected, edge attribute 'weight', damping 0.5, reset = node weights; then doc_scores = pagerank[passage_node_idxs]).
// Here the N scores never leave HBM: scan -> global min / max -> scatter of min_max(score) * passage_node_weight into the
// reset vector through the passage-row -> vertex map -> power iteration on a CSR copy of the graph -> gather of the
// passage vertices; only n_passages doubles come back (8 * n_passages bytes instead of 12 * N + the igraph call).
//
// Semantics restated from igraph_personalized_pagerank(PRPACK): reset vector r (negative / NaN entries -> 0, then divided
// by its sum); transition i -> j with probability w_ij / s_i (s_i = sum of i's incident weights; undirected = both
// directions); a vertex without edges jumps according to r; x = d * (P^T x + (sum of dangling x) * r) + (1 - d) * r.
// prpack solves this system directly to ~1e-10; a power iteration contracts by d per step, so ceil(log(tol/2)/log(d))
// steps reach tol in the 1-norm (43 steps for tol = 1e-12 at d = 0.5).  fp64 throughout, fixed summation order
// (pull-style CSR rows, block-ordered reductions): results are reproducible bit for bit.
// (Round 3 built and measured a single-launch variant for ComoRAG-sized graphs — one workgroup, x / y in LDS, a thread's
// rows advanced together: 1064 us per query at 5 K passages / 1.5 K entities against 551 us for this chain of ~50 launches;
// one CU's L2-latency-bound row walks lose against 43 grid-wide steps.  Dropped.  gpurun_out of the round: profiles/r3_measurements.md.)
//
// One query or a batch of up to CMR_PPR_MAX_BATCH (ComoRAG.try_answer runs up to 16 graph searches at once, ComoRAG.py:432-453)
// go through ONE host path: a PprScratch of width bw (1 for one query; 2 / 4 / 8 / 16 for a batch, vectors stored [nv][bw]) out of
// the graph's one pool, one capture-and-replay routine (ppr_iterate), one body per C entry-point pair.  Only the kernels differ by
// width: bw == 1 runs the one-query kernels (a double per lane), wider scratches the templated ones (a double2 per lane).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <mutex>
#include <vector>

#include "../../include/comorag_hip.h"
#include "cmr_internal.h"
#include "cmr_kernels.h"

#define PPR_T 256
#define PPR_RED_BLOCKS 256

// The per-call vectors of `bw` queries: bw == 1 for one query, 2 / 4 / 8 / 16 for a batch ([nv][bw], vertex-major).
struct PprScratch {
    int bw = 1;
    double *reset = nullptr, *x = nullptr, *y = nullptr, *out = nullptr;
    double* red = nullptr;             // [bw][PPR_RED_BLOCKS] partial sums, then [bw] totals, then [bw] dangling masses
    float2* mm = nullptr;              // [bw][PPR_RED_BLOCKS] (min, max) partials of the raw scores, then [bw] finals
    int *seed_v = nullptr, *seed_q = nullptr;
    double* seed_w = nullptr;
    long long seed_cap = 0, out_cap = 0;
    void* rank = nullptr;              // the ranking's workspace (cmr_sort_workspace_bytes), allocated and grown by ranked calls only
    size_t rank_cap = 0;
    // the power iteration of THIS scratch as an instantiated hipGraph (clean + normalise + `iters` steps: every argument is
    // one of this scratch's pointers or a graph constant), keyed by (damping, iters); replayed with one hipGraphLaunch
    hipGraphExec_t iter_exec = nullptr;
    double iter_damping = 0.0;
    int iter_count = 0;
    double* iter_result = nullptr;
    hipStream_t own = nullptr;         // cmr_graph_ppr*'s stream (capturable, unlike the legacy default stream), created on first use there
    double* totals() const { return red + (size_t)bw * PPR_RED_BLOCKS; }
    double* dmass() const { return red + (size_t)bw * PPR_RED_BLOCKS + bw; }
    float2* mm_final() const { return mm + (size_t)bw * PPR_RED_BLOCKS; }
    void release() {
        if (iter_exec) (void)hipGraphExecDestroy(iter_exec);
        if (own) (void)hipStreamDestroy(own);
        for (void* p : {(void*)reset, (void*)x, (void*)y, (void*)red, (void*)out, (void*)mm, (void*)seed_v, (void*)seed_q, (void*)seed_w, rank})
            if (p) (void)hipFree(p);
    }
};

struct cmr_graph {
    int device = 0;
    long long nv = 0, ne = 0;          // vertices, directed CSR entries (2 x undirected edges, self-loops once)
    long long* rowptr = nullptr;       // [nv + 1]
    int* col = nullptr;                // [ne]
    double* wnorm = nullptr;           // [ne]  w_ij / s_j of the SOURCE j of the pulled term (so y_i = sum_j wnorm * x_j)
    int* dangling = nullptr;           // vertices with no incident weight (internal ids, ascending)
    long long n_dangling = 0;
    // Vertices are REORDERED at cmr_graph_create by degree class (the exported ids stay the caller's): internal order = rows of more
    // than PPR_WAVE_DEG entries (a wave each), rows of PPR_ONE_DEG + 1 .. PPR_WAVE_DEG entries (eight lanes each), rows of <= PPR_ONE_DEG
    // entries (ONE thread each, stored as 4-slot ELL records: one 16-byte column load + two 16-byte weight loads per thread).  A step then
    // runs ~4x fewer waves than eight lanes for every row did — the step is latency x occupancy bound: waves in flight x ~4 dependent
    // memory round trips each — and a hub vertex of thousands of edges is no longer a 1000-iteration tail on eight lanes.
    long long n_wave = 0, n_oct = 0, n_one = 0;
    int4* ell_col = nullptr;           // [n_one] columns of a short row (absent slots: column 0 with weight 0)
    double* ell_w = nullptr;           // [n_one][4]
    int* perm = nullptr;               // device: caller's vertex id -> internal vertex
    std::vector<int> perm_h;           // the same on the host (seed vertices, the passage map)
    int* vertex_of_row = nullptr;      // passage row -> INTERNAL vertex
    long long n_rows = 0;
    // Per-call scratch.  ComoRAG runs graph_search_with_fact_entities from up to 16 threads at once (ComoRAG.try_answer's
    // ThreadPoolExecutor, ComoRAG.py:437) and ctypes releases the GIL: every call takes its own set of vectors from this
    // pool (grown on demand, one set per concurrent caller and width), so concurrent queries on one graph never share a reset / x / y.
    std::mutex mu;                     // guards the pool and the passage-vertex map's replacement
    std::vector<PprScratch*> pool;     // idle scratches of every width, most recently returned last
    int users = 0;                     // calls in flight (cmr_graph_set_passage_vertices waits for none)
    std::atomic<bool> use_graph{true}; // power iteration replayed as a captured hipGraph (cleared if capture ever fails)
    std::condition_variable idle;
};

// ------------------------------------------------------------------------------------------ kernels
// Row b of a batch equals the single call bit for bit: for every (row, query) both families of kernels execute the same
// floating-point operations in the same order, and every one of them is written out — fma() / __dmul_rn / plain adds, compiled
// with contraction OFF, so the compiler has no choice left:
//   * a (virtual) lane's share of a CSR row: acc = +0.0, then acc = fma(w, x, acc) per entry in ascending order, four per round,
//     an absent entry of a round contributing fma(0.0, x[0], acc);
//   * a short row: t = w1 * x1 (a plain multiply), then fma(w0, x0, t), fma(w2, x2, .), fma(w3, x3, .) — NOT slot order: the
//     multiply is slot 1's;
//   * the xor tree (32 .. 1 over the 64 virtual lanes of a long row, 4 2 1 over the eight of a medium row) of plain adds;
//   * y = fma(1 - d, r, d * fma(D, r, acc))  (ppr_update);
//   * the reductions (clean + sum, dangling mass) are plain adds in the order thread -> wave xor tree -> waves 0 .. 3 -> blocks
//     0 .. nparts - 1; r / tot is an IEEE division.
// Only the MAPPING differs by width.  One query: a lane owns a double.  A batch: a lane owns a PAIR of queries (double2: one
// 16-byte load per gathered vertex — with [nv][BW] vectors the gather of one neighbour is an aligned BW * 8-byte run, a whole
// 128-byte line at BW = 16, and col / wnorm / the ELL records are read ONCE per step for all queries), BW / 2 adjacent lanes cover
// one vertex; the 64 virtual lanes of a long row are 64 / P lanes x P accumulators of a thread (P = BW / 2).
#pragma clang fp contract(off)

__device__ __forceinline__ double block_sum(double v, double* sh) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < PPR_T / 64; ++w) t += sh[w];      // fixed order
    __syncthreads();
    return t;
}

// ---- every width
// per-block partial (min, max) of the raw scores [gridDim.y][n]; blockIdx.y = query
__global__ __launch_bounds__(PPR_T) void ppr_minmax_partial_batch_kernel(const float* __restrict__ s_all, long long n, float2* __restrict__ part_all) {
    __shared__ float smn[PPR_T / 64], smx[PPR_T / 64];
    const float* __restrict__ s = s_all + (size_t)blockIdx.y * n;
    float2* __restrict__ part = part_all + (size_t)blockIdx.y * PPR_RED_BLOCKS;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (long long i = (long long)blockIdx.x * PPR_T + threadIdx.x; i < n; i += (long long)gridDim.x * PPR_T) { const float v = s[i]; mn = fminf(mn, v); mx = fmaxf(mx, v); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { mn = fminf(mn, __shfl_xor(mn, off)); mx = fmaxf(mx, __shfl_xor(mx, off)); }
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < PPR_T / 64; ++w) { mn = fminf(mn, smn[w]); mx = fmaxf(mx, smx[w]); }
        part[blockIdx.x] = make_float2(mn, mx);
    }
}

// reset[v[i]][q[i]] += w[i] (q == nullptr: query 0).  (vertex, query) pairs are distinct: the host sums duplicates per query first
// (merge_seeds), in input order
__global__ __launch_bounds__(PPR_T) void ppr_seed_batch_kernel(const int* __restrict__ v, const int* __restrict__ q, const double* __restrict__ w, long long n, int bw,
                                                               double* __restrict__ reset) {
    const long long i = (long long)blockIdx.x * PPR_T + threadIdx.x;
    if (i < n) reset[(size_t)v[i] * bw + (q ? q[i] : 0)] += w[i];
}

// mass sitting on vertices without edges: one block per query, fixed order
__global__ __launch_bounds__(PPR_T) void ppr_dangling_batch_kernel(const double* __restrict__ x, const int* __restrict__ dang, long long nd, int bw, double* __restrict__ out) {
    __shared__ double sh[PPR_T / 64];
    const int q = blockIdx.x;
    double acc = 0.0;
    for (long long i = threadIdx.x; i < nd; i += PPR_T) acc += x[(size_t)dang[i] * bw + q];
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) out[q] = t;
}

// y = d * (acc + D * r) + (1 - d) * r
__device__ __forceinline__ double ppr_update(double acc, double D, double r, double d) { return fma(1.0 - d, r, __dmul_rn(d, fma(D, r, acc))); }

// ---- one query (bw == 1)
// reset[vertex_of_row[i]] = min_max_normalize(scores)[i] * pnw  (the reference's fp32 formula, utils/misc_utils.py:141-150;
// applied twice there (ComoRAG.py:963, :1035) — the second application is the identity), then the product in fp64 as
// numpy does for float32 * python float
__global__ __launch_bounds__(PPR_T) void ppr_scatter_kernel(const float* __restrict__ s, long long n, const float2* __restrict__ part, int nparts,
                                                            const int* __restrict__ vertex_of_row, double pnw, double* __restrict__ reset) {
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int b = 0; b < nparts; ++b) { mn = fminf(mn, part[b].x); mx = fmaxf(mx, part[b].y); }
    const float range = mx - mn;
    const long long i = (long long)blockIdx.x * PPR_T + threadIdx.x;
    if (i >= n) return;
    const float norm = range == 0.0f ? 1.0f : (s[i] - mn) / range;
    reset[vertex_of_row[i]] = (double)norm * pnw;
}

// reset <- max(reset, 0) with NaN -> 0 (ComoRAG.py:1090); partial sums per block
__global__ __launch_bounds__(PPR_T) void ppr_clean_sum_kernel(double* __restrict__ r, long long nv, double* __restrict__ part) {
    __shared__ double sh[PPR_T / 64];
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * PPR_T + threadIdx.x; i < nv; i += (long long)gridDim.x * PPR_T) {
        double v = r[i];
        if (!(v >= 0.0)) v = 0.0;
        r[i] = v;
        acc += v;
    }
    const double t = block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = t;
}

// r <- r / sum, x <- r
__global__ __launch_bounds__(PPR_T) void ppr_normalise_kernel(double* __restrict__ r, double* __restrict__ x, long long nv, const double* __restrict__ part, int nparts) {
    double tot = 0.0;
    for (int b = 0; b < nparts; ++b) tot += part[b];
    const long long i = (long long)blockIdx.x * PPR_T + threadIdx.x;
    if (i >= nv) return;
    const double v = tot > 0.0 ? r[i] / tot : 1.0 / (double)nv;
    r[i] = v;
    x[i] = v;
}

// y_i = d * (sum_{j in N(i)} wnorm_ij * x_j + D * r_i) + (1 - d) * r_i
// Three row classes in one launch (block ranges; see cmr_graph): a wave per long row, PPR_LPR lanes per medium row, a thread per
// short row.  Every row has ONE summation order: lanes stride over a row's entries (coalesced col / wnorm reads) and sum theirs in
// ascending order, the partials are combined by a fixed xor tree; a short row adds its four slots in the order stated above —
// reproducible bit for bit.  (With one thread per vertex for every row a step lasted as long as the LONGEST row's chain of dependent
// loads; with eight lanes for every row — round 2 — a 3-entry passage row left five lanes idle and the step ran 150 K waves at 1 M passages.)
#define PPR_LPR 8
#define PPR_ONE_DEG 4
#define PPR_WAVE_DEG 256
// A lane's share of a row: entries e0, e0 + STRIDE, ... < e1, summed in that order.  Four entries per round: their column / weight loads,
// then their four gathers, are independent and in flight together — a lane's chain is (rowptr -> columns -> x) per ROUND, not per
// entry (an entity row of 19 entries on eight lanes was three dependent col -> x round trips; now one).  An absent entry contributes
// fma(0.0, x[0], acc): adding +0.0 changes nothing, so the sum equals the one-entry-at-a-time loop bit for bit.
template <int STRIDE>
__device__ __forceinline__ double ppr_row_sum(long long e0, long long e1, const int* __restrict__ col, const double* __restrict__ wnorm,
                                              const double* __restrict__ x) {
    double acc = 0.0;
    for (long long e = e0; e < e1; e += 4 * STRIDE) {
        int c[4];
        double w[4], xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long ee = e + (long long)u * STRIDE;
            const bool ok = ee < e1;
            c[u] = ok ? col[ee] : 0;
            w[u] = ok ? wnorm[ee] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[u] = x[c[u]];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = fma(w[u], xv[u], acc);
    }
    return acc;
}
__global__ __launch_bounds__(PPR_T) void ppr_step_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ wnorm,
                                                         const int4* __restrict__ ell_col, const double* __restrict__ ell_w,
                                                         const double* __restrict__ x, const double* __restrict__ r, const double* __restrict__ dmass,
                                                         double d, long long n_wave, long long n_oct, long long n_one, unsigned b_wave, unsigned b_oct,
                                                         double* __restrict__ y) {
    const double D = dmass ? dmass[0] : 0.0;
    if (blockIdx.x < b_wave) {                                   // a wave per row
        const long long i = (long long)blockIdx.x * (PPR_T / 64) + (threadIdx.x >> 6);
        const int lane = threadIdx.x & 63;
        double acc = 0.0;
        if (i < n_wave) acc = ppr_row_sum<64>(rowptr[i] + lane, rowptr[i + 1], col, wnorm, x);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (i < n_wave && lane == 0) y[i] = ppr_update(acc, D, r[i], d);
    } else if (blockIdx.x < b_wave + b_oct) {                    // eight lanes per row
        const long long gt = (long long)(blockIdx.x - b_wave) * PPR_T + threadIdx.x;
        const long long i = n_wave + gt / PPR_LPR;
        const int sub = (int)(gt % PPR_LPR);
        const bool in = i < n_wave + n_oct;
        double acc = 0.0;
        if (in) acc = ppr_row_sum<PPR_LPR>(rowptr[i] + sub, rowptr[i + 1], col, wnorm, x);
#pragma unroll
        for (int off = PPR_LPR / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
        if (in && sub == 0) y[i] = ppr_update(acc, D, r[i], d);
    } else {                                                     // a thread per row: four ELL slots
        const long long t = (long long)(blockIdx.x - b_wave - b_oct) * PPR_T + threadIdx.x;
        if (t >= n_one) return;
        const long long i = n_wave + n_oct + t;
        const int4 c = ell_col[t];
        const double2 w01 = reinterpret_cast<const double2*>(ell_w)[2 * t], w23 = reinterpret_cast<const double2*>(ell_w)[2 * t + 1];
        const double x0 = x[c.x], x1 = x[c.y], x2 = x[c.z], x3 = x[c.w];      // four independent gathers in flight
        double acc = __dmul_rn(w01.y, x1);                                    // the multiply is slot 1's
        acc = fma(w01.x, x0, acc);
        acc = fma(w23.x, x2, acc);
        acc = fma(w23.y, x3, acc);
        y[i] = ppr_update(acc, D, r[i], d);
    }
}

// caller's order -> internal order
__global__ __launch_bounds__(PPR_T) void ppr_permute_in_kernel(const double* __restrict__ src, const int* __restrict__ perm, long long nv, double* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * PPR_T + threadIdx.x;
    if (i < nv) dst[perm[i]] = src[i];
}
// dst[i] = src[map[i]]: back to the caller's order (map = perm, n = nv) and the gather of the passage vertices (map = vertex_of_row, n = n_rows)
__global__ __launch_bounds__(PPR_T) void ppr_gather_kernel(const double* __restrict__ src, const int* __restrict__ map, long long n, double* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * PPR_T + threadIdx.x;
    if (i < n) dst[i] = src[map[i]];
}

// ---- a batch (bw == BW in 2 / 4 / 8 / 16)
__device__ __forceinline__ double2 ppr_shfl_xor2(double2 v, int off) { return make_double2(__shfl_xor(v.x, off), __shfl_xor(v.y, off)); }
__device__ __forceinline__ double2 ppr_add2(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 ppr_fma2(double w, double2 x, double2 acc) { return make_double2(fma(w, x.x, acc.x), fma(w, x.y, acc.y)); }
__device__ __forceinline__ double2 ppr_update2(double2 acc, double2 D, double2 r, double d) {
    return make_double2(ppr_update(acc.x, D.x, r.x, d), ppr_update(acc.y, D.y, r.y, d));
}

// ppr_row_sum for a pair of queries: `x` points at this lane's pair of vertex 0, vertices are P double2 apart
template <int STRIDE, int P>
__device__ __forceinline__ double2 ppr_row_sum2(long long e0, long long e1, const int* __restrict__ col, const double* __restrict__ wnorm,
                                                const double2* __restrict__ x) {
    double2 acc = make_double2(0.0, 0.0);
    for (long long e = e0; e < e1; e += 4 * STRIDE) {
        int c[4];
        double w[4];
        double2 xv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long ee = e + (long long)u * STRIDE;
            const bool ok = ee < e1;
            c[u] = ok ? col[ee] : 0;
            w[u] = ok ? wnorm[ee] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) xv[u] = x[(size_t)c[u] * P];
#pragma unroll
        for (int u = 0; u < 4; ++u) acc = ppr_fma2(w[u], xv[u], acc);
    }
    return acc;
}

template <int BW>
__global__ __launch_bounds__(PPR_T) void ppr_step_batch_kernel(const long long* __restrict__ rowptr, const int* __restrict__ col, const double* __restrict__ wnorm,
                                                               const int4* __restrict__ ell_col, const double* __restrict__ ell_w,
                                                               const double2* __restrict__ x, const double2* __restrict__ r, const double2* __restrict__ dmass,
                                                               double d, long long n_wave, long long n_oct, long long n_one, unsigned b_wave, unsigned b_oct,
                                                               double2* __restrict__ y) {
    constexpr int P = BW / 2;                                    // lanes per vertex
    const int pair = threadIdx.x % P;
    const double2 D = dmass ? dmass[pair] : make_double2(0.0, 0.0);
    if (blockIdx.x < b_wave) {                                   // a wave per row: virtual lane v = k * VS + vs, k in this thread
        constexpr int VS = 64 / P;
        const long long i = (long long)blockIdx.x * (PPR_T / 64) + (threadIdx.x >> 6);
        const int vs = (threadIdx.x & 63) / P;
        const bool in = i < n_wave;
        double2 a[P];
#pragma unroll
        for (int k = 0; k < P; ++k) a[k] = in ? ppr_row_sum2<64, P>(rowptr[i] + k * VS + vs, rowptr[i + 1], col, wnorm, x + pair) : make_double2(0.0, 0.0);
#pragma unroll
        for (int off = 32; off >= VS; off >>= 1)                 // the tree's levels between virtual lanes of one thread
#pragma unroll
            for (int k = 0; k < off / VS; ++k) a[k] = ppr_add2(a[k], a[k + off / VS]);
        double2 acc = a[0];
#pragma unroll
        for (int off = VS / 2; off > 0; off >>= 1) acc = ppr_add2(acc, ppr_shfl_xor2(acc, off * P));
        if (in && vs == 0) y[(size_t)i * P + pair] = ppr_update2(acc, D, r[(size_t)i * P + pair], d);
    } else if (blockIdx.x < b_wave + b_oct) {                    // eight virtual lanes per row: lane = sub * P + pair
        const long long gt = (long long)(blockIdx.x - b_wave) * PPR_T + threadIdx.x;
        const long long i = n_wave + gt / (PPR_LPR * P);
        const int sub = (int)(gt % (PPR_LPR * P)) / P;
        const bool in = i < n_wave + n_oct;
        double2 acc = make_double2(0.0, 0.0);
        if (in) acc = ppr_row_sum2<PPR_LPR, P>(rowptr[i] + sub, rowptr[i + 1], col, wnorm, x + pair);
#pragma unroll
        for (int off = PPR_LPR / 2; off > 0; off >>= 1) acc = ppr_add2(acc, ppr_shfl_xor2(acc, off * P));
        if (in && sub == 0) y[(size_t)i * P + pair] = ppr_update2(acc, D, r[(size_t)i * P + pair], d);
    } else {                                                     // P lanes per short row: four ELL slots, no cross-lane reduction
        const long long t = ((long long)(blockIdx.x - b_wave - b_oct) * PPR_T + threadIdx.x) / P;
        if (t >= n_one) return;
        const long long i = n_wave + n_oct + t;
        const int4 c = ell_col[t];
        const double2 w01 = reinterpret_cast<const double2*>(ell_w)[2 * t], w23 = reinterpret_cast<const double2*>(ell_w)[2 * t + 1];
        const double2* xp = x + pair;
        const double2 x0 = xp[(size_t)c.x * P], x1 = xp[(size_t)c.y * P], x2 = xp[(size_t)c.z * P], x3 = xp[(size_t)c.w * P];
        double2 acc = make_double2(__dmul_rn(w01.y, x1.x), __dmul_rn(w01.y, x1.y));      // the multiply is slot 1's, as in ppr_step_kernel
        acc = ppr_fma2(w01.x, x0, acc);
        acc = ppr_fma2(w23.x, x2, acc);
        acc = ppr_fma2(w23.y, x3, acc);
        y[(size_t)i * P + pair] = ppr_update2(acc, D, r[(size_t)i * P + pair], d);
    }
}

// The small kernels.  Each keeps the one-query kernel's block count and thread -> element assignment, so every query's reduction
// has that kernel's order; a thread handles ALL BW queries of its element (one aligned BW * 8-byte run) instead of one block row per query,
// which would read every line BW times.
template <int BW>
__global__ __launch_bounds__(PPR_T) void ppr_clean_sum_batch_kernel(double* __restrict__ r, long long nv, double* __restrict__ part) {
    __shared__ double sh[PPR_T / 64];
    double acc[BW];
#pragma unroll
    for (int q = 0; q < BW; ++q) acc[q] = 0.0;
    for (long long i = (long long)blockIdx.x * PPR_T + threadIdx.x; i < nv; i += (long long)gridDim.x * PPR_T) {
        double2* p = reinterpret_cast<double2*>(r + (size_t)i * BW);
#pragma unroll
        for (int j = 0; j < BW / 2; ++j) {
            double2 v = p[j];
            if (!(v.x >= 0.0)) v.x = 0.0;
            if (!(v.y >= 0.0)) v.y = 0.0;
            p[j] = v;
            acc[2 * j] += v.x;
            acc[2 * j + 1] += v.y;
        }
    }
#pragma unroll
    for (int q = 0; q < BW; ++q) {
        const double t = block_sum(acc[q], sh);
        if (threadIdx.x == 0) part[(size_t)q * PPR_RED_BLOCKS + blockIdx.x] = t;
    }
}

// tot[q] = part[q][0] + part[q][1] + ... from 0.0, the loop every thread of ppr_normalise_kernel runs; (mn, mx)[q] likewise as ppr_scatter_kernel
__global__ void ppr_totals_batch_kernel(const double* __restrict__ part, int nparts, int bw, double* __restrict__ tot) {
    const int q = threadIdx.x;
    if (q >= bw) return;
    double t = 0.0;
    for (int b = 0; b < nparts; ++b) t += part[(size_t)q * PPR_RED_BLOCKS + b];
    tot[q] = t;
}
__global__ void ppr_minmax_final_batch_kernel(const float2* __restrict__ part, int nparts, int nb, float2* __restrict__ fin) {
    const int q = threadIdx.x;
    if (q >= nb) return;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    for (int b = 0; b < nparts; ++b) { mn = fminf(mn, part[(size_t)q * PPR_RED_BLOCKS + b].x); mx = fmaxf(mx, part[(size_t)q * PPR_RED_BLOCKS + b].y); }
    fin[q] = make_float2(mn, mx);
}

template <int BW>
__global__ __launch_bounds__(PPR_T) void ppr_normalise_batch_kernel(double* __restrict__ r, double* __restrict__ x, long long nv, const double* __restrict__ tot) {
    const long long i = (long long)blockIdx.x * PPR_T + threadIdx.x;
    if (i >= nv) return;
    double2* rp = reinterpret_cast<double2*>(r + (size_t)i * BW);
    double2* xp = reinterpret_cast<double2*>(x + (size_t)i * BW);
#pragma unroll
    for (int j = 0; j < BW / 2; ++j) {
        const double t0 = tot[2 * j], t1 = tot[2 * j + 1];
        double2 v = rp[j];
        v.x = t0 > 0.0 ? v.x / t0 : 1.0 / (double)nv;
        v.y = t1 > 0.0 ? v.y / t1 : 1.0 / (double)nv;
        rp[j] = v;
        xp[j] = v;
    }
}

// reset[vertex_of_row[i]][q] = min_max_normalize(scores[q])[i] * pnw (ppr_scatter_kernel's formula); the padding columns nb .. BW - 1 copy column 0
template <int BW>
__global__ __launch_bounds__(PPR_T) void ppr_scatter_batch_kernel(const float* __restrict__ s, long long n, int nb, const float2* __restrict__ fin,
                                                                  const int* __restrict__ vertex_of_row, double pnw, double* __restrict__ reset) {
    const long long i = (long long)blockIdx.x * PPR_T + threadIdx.x;
    if (i >= n) return;
    double v[BW];
#pragma unroll
    for (int q = 0; q < BW; ++q) {
        if (q < nb) {
            const float mn = fin[q].x, mx = fin[q].y;
            const float range = mx - mn;
            const float norm = range == 0.0f ? 1.0f : (s[(size_t)q * n + i] - mn) / range;
            v[q] = (double)norm * pnw;
        } else {
            v[q] = v[0];
        }
    }
    double2* p = reinterpret_cast<double2*>(reset + (size_t)vertex_of_row[i] * BW);
#pragma unroll
    for (int j = 0; j < BW / 2; ++j) p[j] = make_double2(v[2 * j], v[2 * j + 1]);
}

// src [nb][nv] in the caller's order -> dst [nv][BW] internal (padding columns copy column 0)
template <int BW>
__global__ __launch_bounds__(PPR_T) void ppr_permute_in_batch_kernel(const double* __restrict__ src, const int* __restrict__ perm, long long nv, int nb, double* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * PPR_T + threadIdx.x;
    if (i >= nv) return;
    double v[BW];
#pragma unroll
    for (int q = 0; q < BW; ++q) v[q] = src[(size_t)(q < nb ? q : 0) * nv + i];
    double2* p = reinterpret_cast<double2*>(dst + (size_t)perm[i] * BW);
#pragma unroll
    for (int j = 0; j < BW / 2; ++j) p[j] = make_double2(v[2 * j], v[2 * j + 1]);
}
// dst[q][i] = src[map[i]][q] for q < nb (ppr_gather_kernel for a batch)
template <int BW>
__global__ __launch_bounds__(PPR_T) void ppr_gather_batch_kernel(const double* __restrict__ src, const int* __restrict__ map, long long n, int nb, double* __restrict__ dst) {
    const long long i = (long long)blockIdx.x * PPR_T + threadIdx.x;
    if (i >= n) return;
    const double2* p = reinterpret_cast<const double2*>(src + (size_t)map[i] * BW);
#pragma unroll
    for (int j = 0; j < BW / 2; ++j) {
        const double2 v = p[j];
        if (2 * j < nb) dst[(size_t)(2 * j) * n + i] = v.x;
        if (2 * j + 1 < nb) dst[(size_t)(2 * j + 1) * n + i] = v.y;
    }
}

// ------------------------------------------------------------------------------------------ host
static unsigned blocks_for(long long n) { return (unsigned)std::max<long long>(1, (n + PPR_T - 1) / PPR_T); }
static int ppr_width(int nb) { return nb <= 1 ? 1 : nb <= 2 ? 2 : nb <= 4 ? 4 : nb <= 8 ? 8 : 16; }

// The one place a width picks its kernels: `single` for bw == 1, `batch` with the constant BW for the templated ones.
#define PPR_WIDTH_SWITCH(bw, single, batch)                \
    switch (bw) {                                          \
        case 1: { single; } break;                         \
        case 2: { constexpr int BW = 2; batch; } break;    \
        case 4: { constexpr int BW = 4; batch; } break;    \
        case 8: { constexpr int BW = 8; batch; } break;    \
        default: { constexpr int BW = 16; batch; } break;  \
    }

// One set of [nv][bw] vectors out of the graph's pool: the most recently returned one of that width, else a new one (a set per
// concurrent caller and width, allocated on first use).  `out` is grown to out_need doubles.  A failed allocation frees what it
// got and restores the user count.
static int scratch_acquire(cmr_graph* g, int bw, long long out_need, PprScratch** out) {
    *out = nullptr;
    PprScratch* sc = nullptr;
    {
        std::lock_guard<std::mutex> lk(g->mu);
        for (size_t k = g->pool.size(); k-- > 0;)
            if (g->pool[k]->bw == bw) { sc = g->pool[k]; g->pool.erase(g->pool.begin() + (long)k); break; }
        g->users++;
    }
    auto give_up = [&](hipError_t e, const char* what) {
        if (sc) { sc->release(); delete sc; }
        { std::lock_guard<std::mutex> lk(g->mu); g->users--; }
        g->idle.notify_all();
        return cmr_fail(e == hipErrorOutOfMemory ? CMR_ERR_OOM : CMR_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    };
    if (!sc) {
        sc = new PprScratch();
        sc->bw = bw;
        const size_t vec = (size_t)g->nv * bw * 8;
        hipError_t e = hipMalloc((void**)&sc->reset, vec);
        if (e == hipSuccess) e = hipMalloc((void**)&sc->x, vec);
        if (e == hipSuccess) e = hipMalloc((void**)&sc->y, vec);
        if (e == hipSuccess) e = hipMalloc((void**)&sc->red, (size_t)bw * (PPR_RED_BLOCKS + 2) * 8);
        if (e == hipSuccess) e = hipMalloc((void**)&sc->mm, (size_t)bw * (PPR_RED_BLOCKS + 1) * sizeof(float2));
        if (e != hipSuccess) return give_up(e, "PPR scratch");
    }
    if (sc->out_cap < out_need) {
        if (sc->out) (void)hipFree(sc->out);
        sc->out = nullptr; sc->out_cap = 0;
        hipError_t e = hipMalloc((void**)&sc->out, std::max<size_t>((size_t)out_need * 8, 8));
        if (e != hipSuccess) return give_up(e, "PPR output scratch");
        sc->out_cap = out_need;
    }
    *out = sc;
    return CMR_OK;
}
// Back to the pool.  The holder drains its stream first: nothing may still use the scratch when the next caller takes it.
struct ScratchGuard {
    cmr_graph* g; PprScratch* sc;
    ~ScratchGuard() {
        if (!sc) return;
        { std::lock_guard<std::mutex> lk(g->mu); g->pool.push_back(sc); g->users--; }
        g->idle.notify_all();
    }
};

static int ppr_iters(double damping, double tol, int max_iter) {
    int iters = (int)std::ceil(std::log(std::max(tol, 1e-300) / 2.0) / std::log(std::min(std::max(damping, 1e-12), 1.0 - 1e-12)));
    iters = std::max(1, std::min(iters, max_iter > 0 ? max_iter : 1000));
    if (damping <= 0.0) iters = 1;
    return iters;
}

// reset (device, raw) -> normalised -> power iteration -> *result holds the stationary vector (sc->x or sc->y): ONE linear stream
// of launches, the one-query kernels for bw == 1 and the templated ones for a batch
static void ppr_launches_single(cmr_graph* g, PprScratch* sc, double damping, int iters, hipStream_t s, double** result) {
    const int nparts = (int)std::min<long long>(PPR_RED_BLOCKS, blocks_for(g->nv));
    hipLaunchKernelGGL(ppr_clean_sum_kernel, dim3(nparts), dim3(PPR_T), 0, s, sc->reset, g->nv, sc->red);
    hipLaunchKernelGGL(ppr_normalise_kernel, dim3(blocks_for(g->nv)), dim3(PPR_T), 0, s, sc->reset, sc->x, g->nv, sc->red, nparts);
    const unsigned b_wave = g->n_wave ? (unsigned)((g->n_wave + PPR_T / 64 - 1) / (PPR_T / 64)) : 0u;
    const unsigned b_oct = g->n_oct ? blocks_for(g->n_oct * PPR_LPR) : 0u, b_one = g->n_one ? blocks_for(g->n_one) : 0u;
    double *x = sc->x, *y = sc->y;
    for (int it = 0; it < iters; ++it) {
        if (g->n_dangling) hipLaunchKernelGGL(ppr_dangling_batch_kernel, dim3(1), dim3(PPR_T), 0, s, x, g->dangling, g->n_dangling, 1, sc->dmass());
        hipLaunchKernelGGL(ppr_step_kernel, dim3(std::max(1u, b_wave + b_oct + b_one)), dim3(PPR_T), 0, s, g->rowptr, g->col, g->wnorm, g->ell_col, g->ell_w, x,
                           sc->reset, g->n_dangling ? sc->dmass() : nullptr, damping, g->n_wave, g->n_oct, g->n_one, b_wave, b_oct, y);
        std::swap(x, y);
    }
    *result = x;
}
template <int BW>
static void ppr_launches_batch(cmr_graph* g, PprScratch* sc, double damping, int iters, hipStream_t s, double** result) {
    constexpr int P = BW / 2;
    const int nparts = (int)std::min<long long>(PPR_RED_BLOCKS, blocks_for(g->nv));
    hipLaunchKernelGGL(ppr_clean_sum_batch_kernel<BW>, dim3(nparts), dim3(PPR_T), 0, s, sc->reset, g->nv, sc->red);
    hipLaunchKernelGGL(ppr_totals_batch_kernel, dim3(1), dim3(64), 0, s, sc->red, nparts, BW, sc->totals());
    hipLaunchKernelGGL(ppr_normalise_batch_kernel<BW>, dim3(blocks_for(g->nv)), dim3(PPR_T), 0, s, sc->reset, sc->x, g->nv, sc->totals());
    const unsigned b_wave = g->n_wave ? (unsigned)((g->n_wave + PPR_T / 64 - 1) / (PPR_T / 64)) : 0u;
    const unsigned b_oct = g->n_oct ? blocks_for(g->n_oct * PPR_LPR * P) : 0u, b_one = g->n_one ? blocks_for(g->n_one * P) : 0u;
    double *x = sc->x, *y = sc->y;
    for (int it = 0; it < iters; ++it) {
        if (g->n_dangling) hipLaunchKernelGGL(ppr_dangling_batch_kernel, dim3(BW), dim3(PPR_T), 0, s, x, g->dangling, g->n_dangling, BW, sc->dmass());
        hipLaunchKernelGGL(ppr_step_batch_kernel<BW>, dim3(std::max(1u, b_wave + b_oct + b_one)), dim3(PPR_T), 0, s, g->rowptr, g->col, g->wnorm, g->ell_col, g->ell_w,
                           (const double2*)x, (const double2*)sc->reset, g->n_dangling ? (const double2*)sc->dmass() : (const double2*)nullptr, damping,
                           g->n_wave, g->n_oct, g->n_one, b_wave, b_oct, (double2*)y);
        std::swap(x, y);
    }
    *result = x;
}
static void ppr_iterate_launches(cmr_graph* g, PprScratch* sc, double damping, int iters, hipStream_t s, double** result) {
    PPR_WIDTH_SWITCH(sc->bw, ppr_launches_single(g, sc, damping, iters, s, result), ppr_launches_batch<BW>(g, sc, damping, iters, s, result))
}

// The iteration is ~45-90 dependent launches of a few microseconds each: launch-bound.  They are captured ONCE per scratch
// into a hipGraph of one linear stream (every argument is a pointer of this scratch, the graph's CSR arrays or a constant; the width
// is the scratch's) and replayed with a single hipGraphLaunch per call; any other (damping, iteration count) re-captures.  If capture
// or instantiation fails the plain launches run — same kernels, same order, same results.
static int ppr_iterate(cmr_graph* g, PprScratch* sc, double damping, double tol, int max_iter, hipStream_t s, int* iters_out, double** result) {
    const int iters = ppr_iters(damping, tol, max_iter);
    if (iters_out) *iters_out = iters;
    if (g->use_graph && (!sc->iter_exec || sc->iter_damping != damping || sc->iter_count != iters)) {
        if (sc->iter_exec) { (void)hipGraphExecDestroy(sc->iter_exec); sc->iter_exec = nullptr; }
        hipGraph_t graph = nullptr;
        if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            double* res = nullptr;
            ppr_iterate_launches(g, sc, damping, iters, s, &res);
            if (hipStreamEndCapture(s, &graph) == hipSuccess && graph) {
                if (hipGraphInstantiate(&sc->iter_exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                    sc->iter_damping = damping; sc->iter_count = iters; sc->iter_result = res;
                } else {
                    sc->iter_exec = nullptr;
                }
                (void)hipGraphDestroy(graph);
            }
        }
        (void)hipGetLastError();                 // a failed capture must not poison the plain path below
        if (!sc->iter_exec) g->use_graph = false;
    }
    if (g->use_graph && sc->iter_exec) {
        HIP_TRY(hipGraphLaunch(sc->iter_exec, s));
        *result = sc->iter_result;
        return CMR_OK;
    }
    ppr_iterate_launches(g, sc, damping, iters, s, result);
    HIP_TRY(hipGetLastError());
    return CMR_OK;
}

// The launches around the iteration that differ by width.
// src [nb][nv] in the caller's order -> sc->reset in the internal order
static void launch_permute_in(cmr_graph* g, PprScratch* sc, const double* src, int nb, hipStream_t s) {
    PPR_WIDTH_SWITCH(sc->bw, hipLaunchKernelGGL(ppr_permute_in_kernel, dim3(blocks_for(g->nv)), dim3(PPR_T), 0, s, src, g->perm, g->nv, sc->reset),
                     hipLaunchKernelGGL(ppr_permute_in_batch_kernel<BW>, dim3(blocks_for(g->nv)), dim3(PPR_T), 0, s, src, g->perm, g->nv, nb, sc->reset))
}
// dst[q][i] = src[map[i]][q] for q < nb
static void launch_gather(PprScratch* sc, const double* src, const int* map, long long n, int nb, double* dst, hipStream_t s) {
    PPR_WIDTH_SWITCH(sc->bw, hipLaunchKernelGGL(ppr_gather_kernel, dim3(blocks_for(n)), dim3(PPR_T), 0, s, src, map, n, dst),
                     hipLaunchKernelGGL(ppr_gather_batch_kernel<BW>, dim3(blocks_for(n)), dim3(PPR_T), 0, s, src, map, n, nb, dst))
}
// scores [nb][n] -> per-query min / max -> min_max(score) * pnw into the passages' vertices of sc->reset
static void launch_scatter(cmr_graph* g, PprScratch* sc, const float* scores, long long n, int nb, double pnw, hipStream_t s) {
    const int nparts = (int)std::min<long long>(PPR_RED_BLOCKS, blocks_for(n));
    hipLaunchKernelGGL(ppr_minmax_partial_batch_kernel, dim3(nparts, nb), dim3(PPR_T), 0, s, scores, n, sc->mm);
    PPR_WIDTH_SWITCH(sc->bw,
                     hipLaunchKernelGGL(ppr_scatter_kernel, dim3(blocks_for(n)), dim3(PPR_T), 0, s, scores, n, sc->mm, nparts, g->vertex_of_row, pnw, sc->reset),
                     hipLaunchKernelGGL(ppr_minmax_final_batch_kernel, dim3(1), dim3(64), 0, s, sc->mm, nparts, nb, sc->mm_final());
                     hipLaunchKernelGGL(ppr_scatter_batch_kernel<BW>, dim3(blocks_for(n)), dim3(PPR_T), 0, s, scores, n, nb, sc->mm_final(), g->vertex_of_row, pnw, sc->reset))
}

// ---- the ranking tail (the sort: sort_kernels.hip).  What a ranked call asks for: the first n_out ranks of every query by
// descending score, ties by ascending row, without the [nb, n_rows] doubles going to the host first.
struct PprRankOut { int64_t n_out; int64_t* ids; };

static int ensure_rank(PprScratch* sc, long long n, int nb) {
    const size_t need = cmr_sort_workspace_bytes(n, nb, 8);
    if (need <= sc->rank_cap) return CMR_OK;
    if (sc->rank) HIP_TRY(hipFree(sc->rank));
    sc->rank = nullptr; sc->rank_cap = 0;
    const hipError_t e = hipMalloc(&sc->rank, need);
    if (e != hipSuccess) return cmr_fail(e == hipErrorOutOfMemory ? CMR_ERR_OOM : CMR_ERR_HIP, "PPR ranking workspace: %s", hipGetErrorString(e));
    sc->rank_cap = need;
    return CMR_OK;
}
// sc->out [nb][n] -> the host's ids [nb][n_out] and scores [nb][n_out]: the sort's launches and two copies on `s`
static int rank_and_copy(PprScratch* sc, long long n, int nb, const PprRankOut& rk, double* out_scores, hipStream_t s) {
    int64_t* ids_dev = nullptr;
    double* scores_dev = nullptr;
    HIP_TRY(cmr_launch_sort_scores_f64(sc->out, n, nb, rk.n_out, sc->rank, &ids_dev, &scores_dev, s));
    HIP_TRY(hipMemcpyAsync(rk.ids, ids_dev, (size_t)nb * rk.n_out * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(out_scores, scores_dev, (size_t)nb * rk.n_out * 8, hipMemcpyDeviceToHost, s));
    return CMR_OK;
}
// a ranked call's own argument checks: integers and pointers (`early`), then against the passage map
static int rank_check_early(const PprRankOut* rk) {
    if (!rk) return CMR_OK;
    if (!rk->ids) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (rk->n_out < 1) return cmr_fail(CMR_ERR_INVALID, "n_out must be >= 1 (got %lld)", (long long)rk->n_out);
    return CMR_OK;
}
static int rank_check_rows(const PprRankOut* rk, const cmr_graph* g) {
    if (!rk) return CMR_OK;
    if (rk->n_out > g->n_rows) return cmr_fail(CMR_ERR_INVALID, "n_out = %lld exceeds the %lld passage rows", (long long)rk->n_out, g->n_rows);
    if (g->n_rows >= (1ll << 32)) return cmr_fail(CMR_ERR_UNSUPPORTED, "the ranking's payload is a 32-bit row: %lld rows", g->n_rows);
    return CMR_OK;
}

static int ensure_seeds(PprScratch* sc, long long n) {
    if (n <= sc->seed_cap) return CMR_OK;
    for (void* p : {(void*)sc->seed_v, (void*)sc->seed_q, (void*)sc->seed_w})
        if (p) HIP_TRY(hipFree(p));
    sc->seed_v = nullptr; sc->seed_q = nullptr; sc->seed_w = nullptr; sc->seed_cap = 0;
    HIP_TRY(hipMalloc((void**)&sc->seed_v, (size_t)n * 4));
    HIP_TRY(hipMalloc((void**)&sc->seed_q, (size_t)n * 4));
    HIP_TRY(hipMalloc((void**)&sc->seed_w, (size_t)n * 8));
    sc->seed_cap = n;
    return CMR_OK;
}

// Duplicate seed vertices are SUMMED on the host, in input order: the seed kernel then adds every vertex once — no lost update,
// no atomics, one fixed summation order.  (This is the sparse API's own rule.  The reference's loop ASSIGNS:
// `phrase_weights[phrase_id] = fact_score` (ComoRAG.py:1019-1021, the last fact that names a phrase wins, then `/= num_chunk`);
// comorag_amd/hooks.py resolves that on the host and passes distinct vertices, so the rule here never meets a duplicate there.
// A caller of the sparse C-ABI who wants last-wins must resolve duplicates before the call.)
static void merge_seeds(const int32_t* v, const double* w, int n, std::vector<int>& ov, std::vector<double>& ow) {
    std::vector<std::pair<int, int>> order((size_t)n);
    for (int i = 0; i < n; ++i) order[i] = {v[i], i};
    std::stable_sort(order.begin(), order.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
    ov.clear(); ow.clear();
    for (int i = 0; i < n; ++i) {
        if (!ov.empty() && ov.back() == order[i].first) ow.back() += w[order[i].second];
        else { ov.push_back(order[i].first); ow.push_back(w[order[i].second]); }
    }
}

// cmr_graph_ppr (nb == 1), cmr_graph_ppr_batch and, with `rk`, cmr_graph_ppr_ranked_batch: integers and pointers are judged before the
// handle is touched, every device call comes after both.  A batch of one IS the single call: width 1, the one-query kernels.  Unranked:
// out_scores [nb][nv], every vertex in the caller's order.  Ranked: the passage rows' scores, gathered as the fused call gathers them, then
// ranked — rk->ids and out_scores [nb][n_out].
static int ppr_graph_run(cmr_graph* g, const double* reset, int nb, double damping, double tol, int max_iter, double* out_scores, int32_t* iters,
                         const PprRankOut* rk = nullptr) {
    if (!g || !reset || !out_scores) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (nb < 1) return cmr_fail(CMR_ERR_INVALID, "nb must be >= 1 (got %d)", nb);
    if (nb > CMR_PPR_MAX_BATCH) return cmr_fail(CMR_ERR_UNSUPPORTED, "nb = %d exceeds CMR_PPR_MAX_BATCH (%d): split the batch", nb, CMR_PPR_MAX_BATCH);
    int rc = rank_check_early(rk);
    if (rc) return rc;
    if (rk && !g->vertex_of_row) return cmr_fail(CMR_ERR_INVALID, "cmr_graph_set_passage_vertices was not called");
    if ((rc = rank_check_rows(rk, g))) return rc;
    HIP_TRY(hipSetDevice(g->device));
    PprScratch* sc = nullptr;
    rc = scratch_acquire(g, ppr_width(nb), rk ? (long long)nb * g->n_rows : 0, &sc);
    if (rc) return rc;
    ScratchGuard guard{g, sc};
    if (rk && (rc = ensure_rank(sc, g->n_rows, nb))) return rc;      // before the first launch: growing it frees and allocates
    if (!sc->own) HIP_TRY(hipStreamCreateWithFlags(&sc->own, hipStreamNonBlocking));
    hipStream_t s = sc->own;                                // concurrent callers do not queue behind each other on the null stream
    const long long nv = g->nv;
    auto body = [&]() -> int {
        // the caller's vertex order on both sides of the ABI, the internal (degree-class) order between them: the caller's [nb][nv]
        // rows are staged in y (nv * bw >= nv * nb doubles) and transposed into the internal [nv][bw] order
        HIP_TRY(hipMemcpyAsync(sc->y, reset, (size_t)nb * nv * 8, hipMemcpyHostToDevice, s));
        launch_permute_in(g, sc, sc->y, nb, s);
        double* res = nullptr;
        int rc_ = ppr_iterate(g, sc, damping, tol, max_iter, s, iters, &res);
        if (rc_) return rc_;
        if (rk) {
            // (the map cannot be replaced meanwhile: cmr_graph_set_passage_vertices waits for the scratch's holder)
            const long long n = g->n_rows;
            if (rk->n_out > n || (long long)nb * n > sc->out_cap || cmr_sort_workspace_bytes(n, nb, 8) > sc->rank_cap)
                return cmr_fail(CMR_ERR_INVALID, "the passage-vertex map changed during the call");
            launch_gather(sc, res, g->vertex_of_row, n, nb, sc->out, s);
            HIP_TRY(hipGetLastError());
            return rank_and_copy(sc, n, nb, *rk, out_scores, s);
        }
        double* tmp = res == sc->x ? sc->y : sc->x;
        launch_gather(sc, res, g->perm, nv, nb, tmp, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out_scores, tmp, (size_t)nb * nv * 8, hipMemcpyDeviceToHost, s));
        return CMR_OK;
    };
    rc = body();
    const hipError_t es = hipStreamSynchronize(s);          // also on error paths: nothing may still use the scratch when it goes back
    if (!rc && es != hipSuccess) rc = cmr_fail(CMR_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(es));
    return rc;
}

// cmr_index_ppr (nb == 1, seed_offsets = {0, n_seeds}) and cmr_index_ppr_batch: plain integers and pointers first, the handles'
// contents after them, every device call after both.
static int ppr_index_run(cmr_index_t* idx, cmr_graph* g, const float* q_f32, int nb, const int32_t* seed_offsets, const int32_t* seed_vertices,
                         const double* seed_weights, double passage_node_weight, double damping, double tol, int max_iter, double* out_doc_scores, int32_t* iters,
                         const PprRankOut* rk = nullptr) {
    if (!idx || !g || !q_f32 || !out_doc_scores || !seed_offsets) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (nb < 1) return cmr_fail(CMR_ERR_INVALID, "nb must be >= 1 (got %d)", nb);
    if (nb > CMR_PPR_MAX_BATCH) return cmr_fail(CMR_ERR_UNSUPPORTED, "nb = %d exceeds CMR_PPR_MAX_BATCH (%d): split the batch", nb, CMR_PPR_MAX_BATCH);
    if (int rc_rk = rank_check_early(rk)) return rc_rk;
    if (seed_offsets[0] < 0) return cmr_fail(CMR_ERR_INVALID, "seed_offsets[0] is negative");
    for (int b = 0; b < nb; ++b)
        if (seed_offsets[b + 1] < seed_offsets[b]) return cmr_fail(CMR_ERR_INVALID, "seed_offsets is not ascending at query %d", b);
    const int n_seeds = seed_offsets[nb];
    if (n_seeds > seed_offsets[0] && (!seed_vertices || !seed_weights)) return cmr_fail(CMR_ERR_INVALID, "NULL seed arrays with %d seeds", n_seeds);
    if (!g->vertex_of_row) return cmr_fail(CMR_ERR_INVALID, "cmr_graph_set_passage_vertices was not called");
    {
        const long long rows = cmr_index_row_count(idx);
        if (rows != g->n_rows) return cmr_fail(CMR_ERR_INVALID, "index has %lld rows, the passage-vertex map %lld", rows, g->n_rows);
    }
    if (int rc_rk = rank_check_rows(rk, g)) return rc_rk;
    for (int i = seed_offsets[0]; i < n_seeds; ++i)
        if (seed_vertices[i] < 0 || seed_vertices[i] >= g->nv) return cmr_fail(CMR_ERR_INVALID, "seed vertex %d outside the graph", seed_vertices[i]);
    const int bw = ppr_width(nb);
    // per query: duplicates summed in input order (merge_seeds), distinct vertices after it, so their order no longer matters; the
    // padding columns nb .. bw - 1 get column 0's seeds, as they get its scores
    std::vector<int> sv, sq, mv;
    std::vector<double> sw, mw;
    for (int q = 0; q < bw; ++q) {
        const int b = q < nb ? q : 0;
        const int o = seed_offsets[b], n = seed_offsets[b + 1] - o;
        merge_seeds(n ? seed_vertices + o : nullptr, n ? seed_weights + o : nullptr, n, mv, mw);
        for (size_t k = 0; k < mv.size(); ++k) { sv.push_back(g->perm_h[mv[k]]); sq.push_back(q); sw.push_back(mw[k]); }
    }
    const long long ns = (long long)sv.size();
    PprScratch* sc = nullptr;
    int rc = scratch_acquire(g, bw, (long long)nb * g->n_rows, &sc);
    if (rc) return rc;
    ScratchGuard guard{g, sc};
    if (rk && (rc = ensure_rank(sc, g->n_rows, nb))) return rc;      // before the first launch: growing it frees and allocates
    float* scores = nullptr;
    long long n = 0;
    void* st = nullptr;
    rc = cmr_index_scores_to_device_batch(idx, q_f32, nb, &scores, &n, &st);       // one scan of nb queries; the [nb, n] scores stay in HBM (index lock held until release)
    if (rc) return rc;
    hipStream_t s = (hipStream_t)st;
    auto body = [&]() -> int {
        if (n != g->n_rows) return cmr_fail(CMR_ERR_INVALID, "index has %lld rows, the passage-vertex map %lld", n, g->n_rows);
        int rc_ = ensure_seeds(sc, std::max<long long>(ns, 1));
        if (rc_) return rc_;
        if (ns) {
            HIP_TRY(hipMemcpyAsync(sc->seed_v, sv.data(), (size_t)ns * 4, hipMemcpyHostToDevice, s));
            if (bw > 1) HIP_TRY(hipMemcpyAsync(sc->seed_q, sq.data(), (size_t)ns * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(sc->seed_w, sw.data(), (size_t)ns * 8, hipMemcpyHostToDevice, s));
        }
        HIP_TRY(hipMemsetAsync(sc->reset, 0, (size_t)g->nv * bw * 8, s));
        if (n) launch_scatter(g, sc, scores, n, nb, passage_node_weight, s);
        if (ns) hipLaunchKernelGGL(ppr_seed_batch_kernel, dim3(blocks_for(ns)), dim3(PPR_T), 0, s, sc->seed_v, bw > 1 ? sc->seed_q : nullptr, sc->seed_w, ns, bw, sc->reset);
        double* res = nullptr;
        rc_ = ppr_iterate(g, sc, damping, tol, max_iter, s, iters, &res);
        if (rc_) return rc_;
        if (n) launch_gather(sc, res, g->vertex_of_row, n, nb, sc->out, s);
        HIP_TRY(hipGetLastError());
        if (rk) {       // the ranking tail: out_doc_scores is [nb][n_out]
            if (rk->n_out > n) return cmr_fail(CMR_ERR_INVALID, "n_out = %lld exceeds the %lld passage rows", (long long)rk->n_out, n);
            if (cmr_sort_workspace_bytes(n, nb, 8) > sc->rank_cap) return cmr_fail(CMR_ERR_INVALID, "the passage-vertex map changed during the call");
            return rank_and_copy(sc, n, nb, *rk, out_doc_scores, s);
        }
        HIP_TRY(hipMemcpyAsync(out_doc_scores, sc->out, (size_t)nb * n * 8, hipMemcpyDeviceToHost, s));
        return CMR_OK;
    };
    rc = body();
    // Whatever happened, the stream is drained before the workspace and the scratch go back: kernels enqueued ahead of a
    // failing call would otherwise still be running on buffers the next caller reuses.
    const hipError_t es = hipStreamSynchronize(s);
    const int rc_rel = cmr_index_scores_release(idx);       // CMR_ERR_NONFINITE if any query held NaN / Inf
    if (rc) return rc;
    if (es != hipSuccess) return cmr_fail(CMR_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(es));
    return rc_rel;
}

// ------------------------------------------------------------------------------------------ C-ABI
extern "C" {

int32_t cmr_graph_create(int32_t device_id, int64_t n_vertices, int64_t n_edges, const int32_t* src, const int32_t* dst, const double* weight,
                         cmr_graph_t** out) {
    if (!out) return cmr_fail(CMR_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n_vertices <= 0 || n_vertices >= (1ll << 31) || n_edges < 0 || (n_edges > 0 && (!src || !dst))) return cmr_fail(CMR_ERR_INVALID, "bad graph arguments");
    HIP_TRY(hipSetDevice(device_id));
    // symmetric CSR on the host: every undirected edge (u, v) contributes v to u's row and u to v's row (a self-loop once,
    // with its weight counted once in the strength), rows in ascending neighbour order so the sums have one fixed order
    std::vector<double> strength((size_t)n_vertices, 0.0);
    std::vector<long long> deg((size_t)n_vertices + 1, 0);
    for (int64_t e = 0; e < n_edges; ++e) {
        const int u = src[e], v = dst[e];
        if (u < 0 || v < 0 || u >= n_vertices || v >= n_vertices) return cmr_fail(CMR_ERR_INVALID, "edge %lld has a vertex outside [0, %lld)", (long long)e, (long long)n_vertices);
        const double w = weight ? weight[e] : 1.0;
        if (!(w >= 0.0)) return cmr_fail(CMR_ERR_INVALID, "edge %lld has a negative or NaN weight", (long long)e);
        strength[u] += w; deg[u + 1]++;
        if (u != v) { strength[v] += w; deg[v + 1]++; }
    }
    // degree classes and the internal order: long rows, medium rows, short rows — each class in the caller's order
    std::vector<int> perm((size_t)n_vertices);
    long long n_wave = 0, n_oct = 0, n_one = 0;
    for (int64_t i = 0; i < n_vertices; ++i) {
        const long long dg = deg[i + 1];
        if (dg > PPR_WAVE_DEG) ++n_wave; else if (dg > PPR_ONE_DEG) ++n_oct; else ++n_one;
    }
    {
        long long at_w = 0, at_o = n_wave, at_1 = n_wave + n_oct;
        for (int64_t i = 0; i < n_vertices; ++i) {
            const long long dg = deg[i + 1];
            perm[i] = (int)(dg > PPR_WAVE_DEG ? at_w++ : dg > PPR_ONE_DEG ? at_o++ : at_1++);
        }
    }
    for (int64_t i = 0; i < n_vertices; ++i) deg[i + 1] += deg[i];
    const long long ne = deg[n_vertices];
    std::vector<std::pair<int, double>> ent((size_t)ne);          // (INTERNAL neighbour, weight) by the caller's row
    std::vector<long long> fill(deg.begin(), deg.end() - 1);
    for (int64_t e = 0; e < n_edges; ++e) {
        const int u = src[e], v = dst[e];
        const double w = weight ? weight[e] : 1.0;
        ent[fill[u]++] = {perm[v], w};
        if (u != v) ent[fill[v]++] = {perm[u], w};
    }
    std::vector<double> strength_int((size_t)n_vertices);
    for (int64_t i = 0; i < n_vertices; ++i) strength_int[perm[i]] = strength[i];
    // internal CSR of the long and medium rows, ELL records of the short ones; a row's entries in ascending INTERNAL neighbour order
    // (stable: parallel edges keep their input order) — the one summation order of the row
    const long long n_csr = n_wave + n_oct;
    std::vector<long long> rowptr((size_t)n_csr + 1, 0);
    for (int64_t i = 0; i < n_vertices; ++i)
        if (perm[i] < n_csr) rowptr[perm[i] + 1] = deg[i + 1] - deg[i];
    for (long long i = 0; i < n_csr; ++i) rowptr[i + 1] += rowptr[i];
    std::vector<int> col((size_t)rowptr[n_csr]);
    std::vector<double> wn((size_t)rowptr[n_csr]);
    std::vector<int> ecol((size_t)n_one * 4, 0);
    std::vector<double> ew((size_t)n_one * 4, 0.0);
    std::vector<int> dang;
    for (int64_t i = 0; i < n_vertices; ++i) {
        std::stable_sort(ent.begin() + deg[i], ent.begin() + deg[i + 1], [](const std::pair<int, double>& a, const std::pair<int, double>& b) { return a.first < b.first; });
        const int pi = perm[i];
        for (long long e = deg[i]; e < deg[i + 1]; ++e) {
            const int j = ent[e].first;
            const double wv = strength_int[j] > 0.0 ? ent[e].second / strength_int[j] : 0.0;      // mass leaving j along this edge
            if (pi < n_csr) { col[rowptr[pi] + (e - deg[i])] = j; wn[rowptr[pi] + (e - deg[i])] = wv; }
            else { ecol[(size_t)(pi - n_csr) * 4 + (e - deg[i])] = j; ew[(size_t)(pi - n_csr) * 4 + (e - deg[i])] = wv; }
        }
    }
    for (int64_t i = 0; i < n_vertices; ++i)
        if (!(strength[i] > 0.0)) dang.push_back(perm[i]);
    std::sort(dang.begin(), dang.end());
    cmr_graph* g = new cmr_graph();
    g->device = device_id; g->nv = n_vertices; g->ne = ne; g->n_dangling = (long long)dang.size();
    g->n_wave = n_wave; g->n_oct = n_oct; g->n_one = n_one;
    auto up = [&](void** p, const void* h, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 16));
        if (e != hipSuccess) return e;
        return bytes ? hipMemcpy(*p, h, bytes, hipMemcpyHostToDevice) : hipSuccess;
    };
    hipError_t e = up((void**)&g->rowptr, rowptr.data(), (size_t)(n_csr + 1) * 8);
    if (e == hipSuccess) e = up((void**)&g->col, col.data(), col.size() * 4);
    if (e == hipSuccess) e = up((void**)&g->wnorm, wn.data(), wn.size() * 8);
    if (e == hipSuccess) e = up((void**)&g->ell_col, ecol.data(), ecol.size() * 4);
    if (e == hipSuccess) e = up((void**)&g->ell_w, ew.data(), ew.size() * 8);
    if (e == hipSuccess) e = up((void**)&g->dangling, dang.data(), dang.size() * 4);
    if (e == hipSuccess) e = up((void**)&g->perm, perm.data(), perm.size() * 4);
    if (e != hipSuccess) { cmr_graph_destroy(g); return cmr_fail(e == hipErrorOutOfMemory ? CMR_ERR_OOM : CMR_ERR_HIP, "graph upload: %s", hipGetErrorString(e)); }
    g->perm_h = std::move(perm);
    *out = g;
    return CMR_OK;
}

int32_t cmr_graph_destroy(cmr_graph_t* g) {
    if (!g) return CMR_OK;
    (void)hipSetDevice(g->device);
    (void)hipDeviceSynchronize();
    for (void* p : {(void*)g->rowptr, (void*)g->col, (void*)g->wnorm, (void*)g->dangling, (void*)g->vertex_of_row, (void*)g->ell_col, (void*)g->ell_w, (void*)g->perm})
        if (p) (void)hipFree(p);
    for (PprScratch* sc : g->pool) { sc->release(); delete sc; }
    delete g;
    return CMR_OK;
}

int32_t cmr_graph_set_passage_vertices(cmr_graph_t* g, const int32_t* vertex_of_row, int64_t n_rows) {
    if (!g || (n_rows > 0 && !vertex_of_row) || n_rows < 0) return cmr_fail(CMR_ERR_INVALID, "bad argument");
    for (int64_t i = 0; i < n_rows; ++i)
        if (vertex_of_row[i] < 0 || vertex_of_row[i] >= g->nv) return cmr_fail(CMR_ERR_INVALID, "row %lld maps to vertex %d outside the graph", (long long)i, vertex_of_row[i]);
    HIP_TRY(hipSetDevice(g->device));
    std::unique_lock<std::mutex> lk(g->mu);
    g->idle.wait(lk, [&] { return g->users == 0; });       // no query may be reading the old map
    if (g->vertex_of_row) HIP_TRY(hipFree(g->vertex_of_row));
    g->vertex_of_row = nullptr; g->n_rows = 0;
    HIP_TRY(hipMalloc((void**)&g->vertex_of_row, std::max<size_t>((size_t)n_rows * 4, 8)));
    if (n_rows) {
        std::vector<int> internal((size_t)n_rows);
        for (int64_t i = 0; i < n_rows; ++i) internal[i] = g->perm_h[vertex_of_row[i]];
        HIP_TRY(hipMemcpy(g->vertex_of_row, internal.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice));
    }
    g->n_rows = n_rows;
    return CMR_OK;
}

int32_t cmr_graph_ppr(cmr_graph_t* g, const double* reset, double damping, double tol, int32_t max_iter, double* out_scores, int32_t* iters) {
    return ppr_graph_run(g, reset, 1, damping, tol, max_iter, out_scores, iters);
}

int32_t cmr_graph_ppr_batch(cmr_graph_t* g, const double* reset, int32_t nb, double damping, double tol, int32_t max_iter, double* out_scores,
                            int32_t* iters) {
    return ppr_graph_run(g, reset, nb, damping, tol, max_iter, out_scores, iters);
}

int32_t cmr_graph_ppr_ranked_batch(cmr_graph_t* g, const double* reset, int32_t nb, double damping, double tol, int32_t max_iter, int64_t n_out,
                                   int64_t* out_ids, double* out_scores, int32_t* iters) {
    const PprRankOut rk{n_out, out_ids};
    return ppr_graph_run(g, reset, nb, damping, tol, max_iter, out_scores, iters, &rk);
}

// ---- combined cmr_index_ppr / cmr_index_ppr_ranked calls (combine.h): concurrent single calls on one index, one graph and one
// parameter set run as ONE cmr_index_ppr_batch / cmr_index_ppr_ranked_batch, whose rows hold the bits of the single calls
struct CombinedPpr {
    cmr_index_t* idx; cmr_graph* g; const float* q; const int32_t* sv; const double* sw; int n_seeds;
    double pnw, damping, tol; int max_iter; double* out; int32_t* iters;
    int64_t n_out; int64_t* out_ids;       // a ranked call: out is [n_out]; unranked: n_out = 0, out is [n_rows]
};

static void combined_ppr_run(void* ctx, cmr_combine::Request** reqs, int n) {
    const int dim = (int)(intptr_t)ctx;
    const CombinedPpr* a0 = (const CombinedPpr*)reqs[0]->args;
    auto answer = [](cmr_combine::Request* r, int rc) { r->rc = rc; if (rc) r->err = cmr_last_error(); };
    const bool ranked = a0->n_out > 0;
    if (n == 1) {       // the caller's own call, its own arguments
        const int32_t seed_offsets[2] = {0, a0->n_seeds};
        const PprRankOut rk{a0->n_out, a0->out_ids};
        answer(reqs[0], ppr_index_run(a0->idx, a0->g, a0->q, 1, seed_offsets, a0->sv, a0->sw, a0->pnw, a0->damping, a0->tol, a0->max_iter, a0->out, a0->iters,
                                      ranked ? &rk : nullptr));
        return;
    }
    // the participants' seeds in the batch call's CSR form; the row count the results are scattered by is the one the call agreed
    // with (ppr_index_run fails when index and passage-vertex map disagree — for everybody: they share both)
    const long long rows = a0->g->n_rows, per = ranked ? a0->n_out : rows;       // doubles per participant (n_out is part of the key)
    std::vector<float> q((size_t)n * dim);
    std::vector<int32_t> off((size_t)n + 1, 0), sv;
    std::vector<double> sw, out((size_t)n * std::max<long long>(per, 1));
    std::vector<int64_t> ids(ranked ? (size_t)n * per : 0);
    for (int i = 0; i < n; ++i) {
        const CombinedPpr* a = (const CombinedPpr*)reqs[i]->args;
        memcpy(q.data() + (size_t)i * dim, a->q, (size_t)dim * 4);
        sv.insert(sv.end(), a->sv, a->sv + a->n_seeds);
        sw.insert(sw.end(), a->sw, a->sw + a->n_seeds);
        off[i + 1] = (int32_t)sv.size();
    }
    int32_t it = 0;
    const PprRankOut rk{a0->n_out, ids.data()};
    int rc = ppr_index_run(a0->idx, a0->g, q.data(), n, off.data(), sv.data(), sw.data(), a0->pnw, a0->damping, a0->tol, a0->max_iter, out.data(), &it,
                           ranked ? &rk : nullptr);
    if (!rc && a0->g->n_rows != rows) rc = cmr_fail(CMR_ERR_INVALID, "the passage-vertex map changed during the call");
    for (int i = 0; i < n; ++i) {
        const CombinedPpr* a = (const CombinedPpr*)reqs[i]->args;
        answer(reqs[i], rc);
        if (rc) continue;
        memcpy(a->out, out.data() + (size_t)i * per, (size_t)per * 8);
        if (ranked) memcpy(a->out_ids, ids.data() + (size_t)i * per, (size_t)per * 8);
        if (a->iters) *a->iters = it;
    }
}

// cmr_index_ppr (rk == nullptr) and cmr_index_ppr_ranked: through the combiner where the index has one, else the single call
static int index_ppr_single(cmr_index_t* idx, cmr_graph_t* g, const float* q_f32, const int32_t* seed_vertices, const double* seed_weights, int32_t n_seeds,
                            double passage_node_weight, double damping, double tol, int32_t max_iter, double* out_doc_scores, int32_t* iters, const PprRankOut* rk) {
    if (n_seeds < 0) return cmr_fail(CMR_ERR_INVALID, "bad argument");
    int dim = 0, dtype = 0;
    const int W = cmr_index_combine_width(idx, &dim, &dtype);
    if (W) {
        // what needs no lock is judged here; a call that would be refused, or whose query is not finite (the batch kernels carry one flag per
        // launch), takes the single call below and gets its error there
        bool joins = g && q_f32 && out_doc_scores && (n_seeds == 0 || (seed_vertices && seed_weights)) && cmr_combine::all_finite(q_f32, (size_t)dim, dtype);
        // (g->n_rows is read without the graph's mutex, as the row-count check of ppr_index_run reads it: a map replaced meanwhile can only
        // send a call the wrong way here — ppr_index_run judges it again, with the scratch held)
        if (rk) joins = joins && rk->ids && rk->n_out >= 1 && rk->n_out <= g->n_rows && g->n_rows < (1ll << 32);
        for (int i = 0; joins && i < n_seeds; ++i) joins = seed_vertices[i] >= 0 && seed_vertices[i] < g->nv;
        if (joins) {
            CombinedPpr a{idx, g, q_f32, seed_vertices, seed_weights, n_seeds, passage_node_weight, damping, tol, max_iter, out_doc_scores, iters,
                          rk ? rk->n_out : 0, rk ? rk->ids : nullptr};
            cmr_combine::Request r;
            r.args = &a;
            cmr_combine::Key key;
            // kind 3: unranked; kind 4 with n_out (< 2^32) above it: ranked calls share a batch only with ranked calls of the same n_out
            key.w[0] = rk ? (4ull | ((uint64_t)rk->n_out << 8)) : 3ull; key.w[1] = (uint64_t)(uintptr_t)g; key.w[2] = cmr_combine::Key::bits(passage_node_weight); key.w[3] = cmr_combine::Key::bits(damping);
            key.w[4] = cmr_combine::Key::bits(tol); key.w[5] = (uint64_t)(int64_t)max_iter;
            cmr_index_combine_submit(idx, key, &r, W, combined_ppr_run, (void*)(intptr_t)dim);
            return r.rc ? cmr_fail(r.rc, "%s", r.err.c_str()) : CMR_OK;
        }
    }
    const int32_t seed_offsets[2] = {0, n_seeds};
    return ppr_index_run(idx, g, q_f32, 1, seed_offsets, seed_vertices, seed_weights, passage_node_weight, damping, tol, max_iter, out_doc_scores, iters, rk);
}

int32_t cmr_index_ppr(cmr_index_t* idx, cmr_graph_t* g, const float* q_f32, const int32_t* seed_vertices, const double* seed_weights, int32_t n_seeds,
                      double passage_node_weight, double damping, double tol, int32_t max_iter, double* out_doc_scores, int32_t* iters) {
    return index_ppr_single(idx, g, q_f32, seed_vertices, seed_weights, n_seeds, passage_node_weight, damping, tol, max_iter, out_doc_scores, iters, nullptr);
}

int32_t cmr_index_ppr_ranked(cmr_index_t* idx, cmr_graph_t* g, const float* q_f32, const int32_t* seed_vertices, const double* seed_weights, int32_t n_seeds,
                             double passage_node_weight, double damping, double tol, int32_t max_iter, int64_t n_out, int64_t* out_ids, double* out_scores,
                             int32_t* iters) {
    const PprRankOut rk{n_out, out_ids};
    return index_ppr_single(idx, g, q_f32, seed_vertices, seed_weights, n_seeds, passage_node_weight, damping, tol, max_iter, out_scores, iters, &rk);
}

int32_t cmr_index_ppr_ranked_batch(cmr_index_t* idx, cmr_graph_t* g, const float* q_f32, int32_t nb, const int32_t* seed_offsets, const int32_t* seed_vertices,
                                   const double* seed_weights, double passage_node_weight, double damping, double tol, int32_t max_iter, int64_t n_out,
                                   int64_t* out_ids, double* out_scores, int32_t* iters) {
    const PprRankOut rk{n_out, out_ids};
    return ppr_index_run(idx, g, q_f32, nb, seed_offsets, seed_vertices, seed_weights, passage_node_weight, damping, tol, max_iter, out_scores, iters, &rk);
}

int32_t cmr_index_ppr_batch(cmr_index_t* idx, cmr_graph_t* g, const float* q_f32, int32_t nb, const int32_t* seed_offsets, const int32_t* seed_vertices,
                            const double* seed_weights, double passage_node_weight, double damping, double tol, int32_t max_iter, double* out_doc_scores,
                            int32_t* iters) {
    return ppr_index_run(idx, g, q_f32, nb, seed_offsets, seed_vertices, seed_weights, passage_node_weight, damping, tol, max_iter, out_doc_scores, iters);
}

}  // extern "C"
