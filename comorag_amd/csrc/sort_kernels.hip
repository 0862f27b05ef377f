// The complete rankings' sort: every row of every segment by descending score, ties by ascending row.
//   fp32 scores (cmr_index_sorted_scores; ComoRAG.dense_passage_retrieval returns ALL N ids by descending score, ComoRAG.py:964-966, and
//                graph_search_with_fact_entities consumes every pair, :1034-1042): 32-bit keys, 4-bit digits, one segment per call
//   fp64 scores (the ranked PageRank calls; np.argsort(doc_scores)[::-1] and doc_scores[sorted_doc_ids.tolist()], ComoRAG.py:1101-1105,
//                without the [nb, n_rows] doubles going to the host first): 64-bit keys, 8-bit digits, a segment per query of the batch
// One segmented, stable LSD radix sort over the complemented order-preserving code of the score with the row (uint32) as payload, 8 passes of
// histogram per tile -> one exclusive scan over a segment's [digit][tile] counters -> stable scatter.  blockIdx.y = segment: one set of launches
// serves the batch, and a segment's tiles, counters and order are those of its single call.  Payloads start ascending, every pass is stable:
// equal scores come by ascending row.  No floating-point operation beyond the key's canonicalisation.
#include <utility>

#include "../../include/comorag_hip.h"
#include "cmr_kernels.h"

#define SORT_T 256                           // threads of every workgroup but the scan's
#define SORT_TILE CMR_PPR_RANK_TILE          // keys per workgroup and pass

// ascending key = descending score: the complement of the order-preserving code of the score.
// float: cmr_score_code's canonicalisation (v + 0.0f: -0.0 counts as +0.0; a NaN keeps the place its bits give it)
__device__ __forceinline__ unsigned sort_key(float v) {
    const unsigned u = __float_as_uint(v + 0.0f);
    return ~((u & 0x80000000u) ? ~u : (u | 0x80000000u));
}
// double: -0.0 counts as +0.0; NaN (ppr_update on a cleaned reset vector yields none) sorts behind everything, so the order stays total
__device__ __forceinline__ u64 sort_key(double v) {
    u64 u = (u64)__double_as_longlong(v);
    if (v != v) return ~0ull;
    if (u == 0x8000000000000000ull) u = 0ull;
    return ~((u >> 63) ? ~u : (u | 0x8000000000000000ull));
}

template <typename S, typename K>
__global__ __launch_bounds__(SORT_T) void sort_init_kernel(const S* __restrict__ scores, unsigned n, K* __restrict__ key, unsigned* __restrict__ val) {
    const size_t i = (size_t)blockIdx.x * SORT_T + threadIdx.x;
    if (i >= n) return;
    const size_t at = (size_t)blockIdx.y * n + i;
    key[at] = sort_key(scores[at]);
    val[at] = (unsigned)i;
}

// hist[segment][digit][tile] = keys of the tile with that digit
template <typename K, int BITS>
__global__ __launch_bounds__(SORT_T) void sort_hist_kernel(const K* __restrict__ key, unsigned n, int shift, unsigned ntiles, unsigned* __restrict__ hist) {
    constexpr unsigned NDIG = 1u << BITS;
    __shared__ unsigned cnt[NDIG];
    for (unsigned d = threadIdx.x; d < NDIG; d += SORT_T) cnt[d] = 0;
    __syncthreads();
    const K* __restrict__ k = key + (size_t)blockIdx.y * n;
    const size_t base = (size_t)blockIdx.x * SORT_TILE;
    for (unsigned j = threadIdx.x; j < SORT_TILE; j += SORT_T)
        if (base + j < n) atomicAdd(&cnt[(unsigned)(k[base + j] >> shift) & (NDIG - 1)], 1u);
    __syncthreads();
    for (unsigned d = threadIdx.x; d < NDIG; d += SORT_T) hist[((size_t)blockIdx.y * NDIG + d) * ntiles + blockIdx.x] = cnt[d];
}

// exclusive scan of a segment's m = digits * ntiles counters, digit-major: a workgroup per segment (fp32: m is ~8 K at 1 M rows, ~78 K at 10 M)
__global__ __launch_bounds__(1024) void sort_scan_kernel(unsigned* __restrict__ hist_all, unsigned m) {
    __shared__ unsigned wsum[16];
    __shared__ unsigned carry_s;
    unsigned* __restrict__ hist = hist_all + (size_t)blockIdx.x * m;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (unsigned base = 0; base < m; base += 1024 * 8) {
        unsigned v[8], local = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const unsigned i = base + tid * 8 + j; v[j] = i < m ? hist[i] : 0u; local += v[j]; }
        unsigned incl = local;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const unsigned o = __shfl_up(incl, off); if (lane >= off) incl += o; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned wbase = 0;
        for (unsigned w = 0; w < wave; ++w) wbase += wsum[w];
        unsigned run = carry_s + wbase + incl - local;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const unsigned i = base + tid * 8 + j; if (i < m) hist[i] = run; run += v[j]; }
        __syncthreads();
        if (tid == 1023) carry_s = run;
        __syncthreads();
    }
}

// Stable scatter of one tile: slices of SORT_T keys in order, waves of a slice in order, lanes of a wave by ballot rank.  The lanes that hold a
// lane's digit are the AND over its BITS bits of ballot(bit) or its complement: BITS ballots, whatever the digit.
template <typename K, int BITS>
__global__ __launch_bounds__(SORT_T) void sort_scatter_kernel(const K* __restrict__ key_in, const unsigned* __restrict__ val_in, unsigned n, int shift, unsigned ntiles,
                                                              const unsigned* __restrict__ offs, K* __restrict__ key_out, unsigned* __restrict__ val_out) {
    constexpr unsigned NDIG = 1u << BITS;
    __shared__ unsigned run[NDIG];                  // where the tile's next key of a digit goes
    __shared__ unsigned wcnt[SORT_T / 64][NDIG];    // the current slice's keys per wave and digit
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t seg = (size_t)blockIdx.y * n;
    for (unsigned d = tid; d < NDIG; d += SORT_T) {
        run[d] = offs[((size_t)blockIdx.y * NDIG + d) * ntiles + blockIdx.x];
#pragma unroll
        for (int w = 0; w < SORT_T / 64; ++w) wcnt[w][d] = 0;
    }
    __syncthreads();
    const u64 lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (unsigned s = 0; s < SORT_TILE; s += SORT_T) {
        const size_t first = (size_t)blockIdx.x * SORT_TILE + s;
        if (first >= n) break;                      // the whole workgroup: the tile ends here
        const size_t i = first + tid;
        const bool ok = i < n;
        const K k = ok ? key_in[seg + i] : (K)0;
        const unsigned d = (unsigned)(k >> shift) & (NDIG - 1);
        u64 peers = __ballot(ok);
#pragma unroll
        for (int bit = 0; bit < BITS; ++bit) {
            const bool on = (d >> bit) & 1u;
            const u64 b = __ballot(on);
            peers &= on ? b : ~b;
        }
        const unsigned rank = (unsigned)__popcll(peers & lt);
        if (ok && rank == 0) wcnt[wave][d] = (unsigned)__popcll(peers);
        __syncthreads();
        if (ok) {
            unsigned pos = run[d] + rank;
            for (unsigned w = 0; w < wave; ++w) pos += wcnt[w][d];
            key_out[seg + pos] = k;                 // pos < n: an exclusive prefix of the segment's n keys plus the keys ahead of this one
            val_out[seg + pos] = val_in[seg + i];
        }
        __syncthreads();
        for (unsigned e = tid; e < NDIG; e += SORT_T) {
            unsigned t = 0;
#pragma unroll
            for (int w = 0; w < SORT_T / 64; ++w) { t += wcnt[w][e]; wcnt[w][e] = 0; }
            run[e] += t;
        }
        __syncthreads();
    }
}

// rank r of segment b: the row (+ id_base) and the bits of its score, gathered from the unranked scores — never recomputed
template <typename S>
__global__ __launch_bounds__(SORT_T) void sort_finish_kernel(const unsigned* __restrict__ val, const S* __restrict__ scores, unsigned n, unsigned n_out, long long id_base,
                                                             int64_t* __restrict__ out_ids, S* __restrict__ out_scores) {
    const size_t r = (size_t)blockIdx.x * SORT_T + threadIdx.x;
    if (r >= n_out) return;
    const unsigned id = val[(size_t)blockIdx.y * n + r];
    out_ids[(size_t)blockIdx.y * n_out + r] = (int64_t)id + id_base;
    out_scores[(size_t)blockIdx.y * n_out + r] = scores[(size_t)blockIdx.y * n + id];
}

// ------------------------------------------------------------------------------------------ host
// Workspace of nb segments of n rows: two key buffers and two payload buffers (the passes alternate) and the counters.
//   fp32 (score_bytes 4): 16 B per row + 64 B per tile + 256 spare bytes
//   fp64 (score_bytes 8): 24 B per row and query + 1 KiB per tile and query
static unsigned sort_tiles(long long n) { return (unsigned)((n + SORT_TILE - 1) / SORT_TILE); }
size_t cmr_sort_workspace_bytes(long long n, int nb, int score_bytes) {
    const size_t digits = score_bytes == 4 ? 16 : 256;
    return (size_t)nb * ((size_t)n * (2 * score_bytes + 8) + (size_t)sort_tiles(n) * digits * 4) + (score_bytes == 4 ? 256 : 0);
}

// scores [nb][n] -> out_ids, out_scores [nb][n_out]: 2 + 3 * passes launches on `s`.  out_ids / out_scores may lie over the key buffers.
template <typename S, typename K, int BITS>
static hipError_t sort_enqueue(const S* scores, long long n, int nb, long long n_out, long long id_base, void* workspace, int64_t* out_ids, S* out_scores,
                               hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n >= (1ll << 32)) return hipErrorInvalidValue;       // the payload is a 32-bit row
    const size_t rows = (size_t)nb * n;
    const unsigned un = (unsigned)n, ntiles = sort_tiles(n);
    K *ki = (K*)workspace, *ko = ki + rows;
    unsigned *vi = (unsigned*)(ko + rows), *vo = vi + rows, *hist = vo + rows;
    hipLaunchKernelGGL((sort_init_kernel<S, K>), dim3((un + SORT_T - 1) / SORT_T, nb), dim3(SORT_T), 0, s, scores, un, ki, vi);
    for (int shift = 0; shift < (int)sizeof(K) * 8; shift += BITS) {
        hipLaunchKernelGGL((sort_hist_kernel<K, BITS>), dim3(ntiles, nb), dim3(SORT_T), 0, s, ki, un, shift, ntiles, hist);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(nb), dim3(1024), 0, s, hist, ntiles << BITS);
        hipLaunchKernelGGL((sort_scatter_kernel<K, BITS>), dim3(ntiles, nb), dim3(SORT_T), 0, s, ki, vi, un, shift, ntiles, hist, ko, vo);
        std::swap(ki, ko);
        std::swap(vi, vo);
    }
    // the order is in vi; both key buffers are dead
    hipLaunchKernelGGL(sort_finish_kernel<S>, dim3(((unsigned)n_out + SORT_T - 1) / SORT_T, nb), dim3(SORT_T), 0, s, vi, scores, un, (unsigned)n_out, id_base, out_ids,
                       out_scores);
    return hipGetLastError();
}

// Ready-made 64-bit keys with a 32-bit payload each (the range search's hits, range_kernels.hip): one segment of n pairs, stable, ascending by
// the 8-bit digit positions of `digits` (bit p = bits [8p, 8p + 8) of the key), lowest position first; a position left out must hold one
// value in every key.  The passes alternate between the two buffer pairs: the sorted pairs end in (*key_out, *val_out), one of them.
// hist: cmr_sort_keys64_hist_bytes(n).  The kernels are the fp64 ranking's.
size_t cmr_sort_keys64_hist_bytes(long long n) { return (size_t)sort_tiles(n) * 256 * sizeof(unsigned); }
hipError_t cmr_launch_sort_keys64(u64* key_a, u64* key_b, unsigned* val_a, unsigned* val_b, unsigned* hist, long long n, unsigned digits, u64** key_out,
                                  unsigned** val_out, hipStream_t s) {
    *key_out = key_a;
    *val_out = val_a;
    if (n <= 0) return hipSuccess;
    if (n >= (1ll << 32)) return hipErrorInvalidValue;
    const unsigned un = (unsigned)n, ntiles = sort_tiles(n);
    u64 *ki = key_a, *ko = key_b;
    unsigned *vi = val_a, *vo = val_b;
    for (int p = 0; p < 8; ++p) {
        if (!((digits >> p) & 1u)) continue;
        const int shift = 8 * p;
        hipLaunchKernelGGL((sort_hist_kernel<u64, 8>), dim3(ntiles, 1), dim3(SORT_T), 0, s, ki, un, shift, ntiles, hist);
        hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 0, s, hist, ntiles << 8);
        hipLaunchKernelGGL((sort_scatter_kernel<u64, 8>), dim3(ntiles, 1), dim3(SORT_T), 0, s, ki, vi, un, shift, ntiles, hist, ko, vo);
        std::swap(ki, ko);
        std::swap(vi, vo);
    }
    *key_out = ki;
    *val_out = vi;
    return hipGetLastError();
}

// scores [n] (device) -> out_ids [n], out_scores [n] sorted descending (ties: ascending row)
hipError_t cmr_launch_sort_scores(const float* scores, long long n, long long id_base, void* workspace, int64_t* out_ids, float* out_scores, hipStream_t s) {
    return sort_enqueue<float, unsigned, 4>(scores, n, 1, n, id_base, workspace, out_ids, out_scores, s);
}

// scores [nb][n] (device) -> the first n_out ranks of every query, left in the workspace: the ids [nb][n_out] over the second (dead) key
// buffer at *ids_at, their scores over the first at *scores_at
hipError_t cmr_launch_sort_scores_f64(const double* scores, long long n, int nb, long long n_out, void* workspace, int64_t** ids_at, double** scores_at,
                                      hipStream_t s) {
    *scores_at = (double*)workspace;
    *ids_at = (int64_t*)workspace + (size_t)nb * n;
    return sort_enqueue<double, u64, 8>(scores, n, nb, n_out, 0, workspace, *ids_at, *scores_at, s);
}
