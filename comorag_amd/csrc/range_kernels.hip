// Range search (cmr_index_range_search / _count): every row of a materialised score block [nb, ld] at or above a bound, per
// query.  The synonymy join reads neighbours down to a similarity threshold (ComoRAG.add_synonymy_edges, ComoRAG.py:670-712, through
// retrieve_knn, utils/embed_utils.py:8-97: 2047 neighbours per entity, consumed until the first score below 0.8); the threshold search
// (cmr_index_search_min_score) caps a list at CMR_MAX_K and cannot say that it did.  The pieces between the scores and the sort:
//   count    grid of (query, tile of CMR_RANGE_TILE rows): hits per tile by wave64 ballots, one uint32 per (query, tile)
//   offsets  one workgroup: exclusive prefix of the counters in query-major order (+ the total behind them) and the per-query counts
//   compact  the same grid: a tile's hits go to offset[query][tile] + rank, ranks from the same ballots — within a query the hits lie by
//            ascending row, no atomic decides a position; a hit is (query in group << 32 | complemented score code, row)
//   finish   behind the stable sort of the pairs (sort_kernels.hip, cmr_launch_sort_keys64): row + id base and the score's bits, gathered
//            from the block — never decoded from the key
// The comparison is the threshold search's: the order-preserving code of the fp32 bits behind cmr_make_key's canonicalisation (v + 0.0f:
// -0.0 and +0.0 are one value).  No floating-point operation beyond that.
// Filtered range search (cmr_index_range_search_masked / _ids, _count_*): masked variants of count and compact — the same
// bodies with MASKED set, where a hit also needs its bit in the query's allow words; offsets, sort and finish are shared.  The unmasked
// kernels are the MASKED = false instantiations: no word is loaded, no branch is added.
#include "../../include/comorag_hip.h"
#include "cmr_kernels.h"

#define RANGE_T 256                          // threads of the tile kernels: two float4 loads per lane cover a tile
#define RANGE_HALF (RANGE_T * 4)             // rows one float4 load per lane covers
static_assert(2 * RANGE_HALF == CMR_RANGE_TILE, "a tile is two float4 loads per lane");

// hi 32 bits of cmr_make_key: order-preserving code of the score
__device__ __forceinline__ unsigned range_code(float v) {
    const unsigned u = __float_as_uint(v + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the lane's four consecutive rows of half h of the tile: their codes, and bit j set where row first + j (< n) is a hit.
// ld % 4 == 0 and first % 4 == 0: the load is 16-byte aligned and stays inside the row's ld floats when first < n.
__device__ __forceinline__ unsigned range_flags(const float* __restrict__ row, size_t first, size_t n, unsigned lo, unsigned (&code)[4]) {
    if (first >= n) { code[0] = code[1] = code[2] = code[3] = 0; return 0u; }
    const float4 v = *reinterpret_cast<const float4*>(row + first);
    code[0] = range_code(v.x); code[1] = range_code(v.y); code[2] = range_code(v.z); code[3] = range_code(v.w);
    unsigned f = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) f |= (first + j < n && code[j] >= lo) ? (1u << j) : 0u;
    return f;
}

// filtered range search: the allow bits of the lane's four rows.  first % 4 == 0, so the four rows share one word of the
// query's mask (one uint32 per 32-row panel): one load, the nibble at bit (first & 31).  first >= n loads nothing — first < n means
// word first >> 5 < ceil(n / 32), the mask's length.
__device__ __forceinline__ unsigned range_allow(const unsigned* __restrict__ words, size_t first, size_t n) {
    return first < n ? (words[first >> 5] >> (unsigned)(first & 31)) & 0xFu : 0u;
}

// cnt[query][tile] = hits of the tile.  blockIdx.x = query * ntiles + tile
// MASKED: a hit also needs its allow bit.  words + (mq0 + query) * stride is the query's mask: stride 0 = one mask for every query; mq0 =
// the index, in `words`, of the mask of the block's query 0 (a block starts anywhere in the call's batch: never derived from blockIdx)
template <bool MASKED>
__device__ __forceinline__ void range_count_body(const float* __restrict__ scores, long long ld, size_t n, unsigned lo, unsigned ntiles, unsigned* __restrict__ cnt,
                                                 const unsigned* __restrict__ words, long long stride, unsigned mq0) {
    __shared__ unsigned wsum[RANGE_T / 64];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned q = blockIdx.x / ntiles, tile = blockIdx.x % ntiles;
    const float* __restrict__ row = scores + (size_t)q * ld;
    const unsigned* __restrict__ wq = MASKED ? words + (size_t)(mq0 + q) * (size_t)stride : nullptr;
    unsigned c = 0;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        unsigned code[4];
        const size_t first = (size_t)tile * CMR_RANGE_TILE + h * RANGE_HALF + tid * 4;
        unsigned f = range_flags(row, first, n, lo, code);
        if constexpr (MASKED) f &= range_allow(wq, first, n);
#pragma unroll
        for (int j = 0; j < 4; ++j) c += (unsigned)__popcll(__ballot((f >> j) & 1u));
    }
    if (lane == 0) wsum[wave] = c;
    __syncthreads();
    if (tid == 0) cnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
__global__ __launch_bounds__(RANGE_T) void range_count_kernel(const float* __restrict__ scores, long long ld, size_t n, unsigned lo, unsigned ntiles,
                                                              unsigned* __restrict__ cnt) {
    range_count_body<false>(scores, ld, n, lo, ntiles, cnt, nullptr, 0, 0u);
}
__global__ __launch_bounds__(RANGE_T) void range_count_masked_kernel(const float* __restrict__ scores, long long ld, size_t n, unsigned lo, unsigned ntiles,
                                                                     unsigned* __restrict__ cnt, const unsigned* __restrict__ words, long long stride, unsigned mq0) {
    range_count_body<true>(scores, ld, n, lo, ntiles, cnt, words, stride, mq0);
}

// cnt[0, m) -> its exclusive prefix in place, cnt[m] = the total; counts[q] = hits of query q (m = nb * ntiles).  One workgroup.
__global__ __launch_bounds__(1024) void range_offsets_kernel(unsigned* __restrict__ cnt, unsigned m, unsigned ntiles, unsigned nb, long long* __restrict__ counts) {
    __shared__ unsigned wsum[16];
    __shared__ unsigned carry_s;
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (unsigned base = 0; base < m; base += 1024 * 8) {
        unsigned v[8], local = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const unsigned i = base + tid * 8 + j; v[j] = i < m ? cnt[i] : 0u; local += v[j]; }
        unsigned incl = local;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const unsigned o = __shfl_up(incl, off); if (lane >= off) incl += o; }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned wbase = 0;
        for (unsigned w = 0; w < wave; ++w) wbase += wsum[w];
        unsigned run = carry_s + wbase + incl - local;
#pragma unroll
        for (int j = 0; j < 8; ++j) { const unsigned i = base + tid * 8 + j; if (i < m) cnt[i] = run; run += v[j]; }
        __syncthreads();
        if (tid == 1023) carry_s = run;
        __syncthreads();
    }
    if (tid == 0) cnt[m] = carry_s;
    __syncthreads();                        // the prefix is written (this workgroup's own global stores)
    for (unsigned q = tid; q < nb; q += 1024) counts[q] = (long long)(cnt[(size_t)(q + 1) * ntiles] - cnt[(size_t)q * ntiles]);
}

// the hits of queries [q_first, q_first + group queries) of the block, compacted: blockIdx.x = (query - q_first) * ntiles + tile.
// cap = the group's hits (offs[(q_first + queries) * ntiles] - offs[q_first * ntiles]): no store at or beyond it.
// MASKED: the count kernel's words, stride and mq0 — query q of the block (q_first + the group's) reads the mask at index mq0 + q
template <bool MASKED>
__device__ __forceinline__ void range_compact_body(const float* __restrict__ scores, long long ld, size_t n, unsigned lo, unsigned ntiles,
                                                   const unsigned* __restrict__ offs, unsigned q_first, unsigned cap, u64* __restrict__ key,
                                                   unsigned* __restrict__ val, const unsigned* __restrict__ words, long long stride, unsigned mq0) {
    __shared__ unsigned wcnt[2][RANGE_T / 64];
    const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned qg = blockIdx.x / ntiles, tile = blockIdx.x % ntiles, q = q_first + qg;
    const float* __restrict__ row = scores + (size_t)q * ld;
    const unsigned* __restrict__ wq = MASKED ? words + (size_t)(mq0 + q) * (size_t)stride : nullptr;
    const u64 lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    unsigned code[2][4], f[2], before[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const size_t first = (size_t)tile * CMR_RANGE_TILE + h * RANGE_HALF + tid * 4;
        f[h] = range_flags(row, first, n, lo, code[h]);
        if constexpr (MASKED) f[h] &= range_allow(wq, first, n);
        unsigned b = 0, tot = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u64 bal = __ballot((f[h] >> j) & 1u);
            b += (unsigned)__popcll(bal & lt);      // hits of the lanes below: their rows are all below this lane's
            tot += (unsigned)__popcll(bal);
        }
        before[h] = b;
        if (lane == 0) wcnt[h][wave] = tot;
    }
    __syncthreads();
    unsigned pos = offs[(size_t)q * ntiles + tile] - offs[(size_t)q_first * ntiles];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        unsigned at = pos + before[h];
        for (unsigned w = 0; w < wave; ++w) at += wcnt[h][w];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((f[h] >> j) & 1u) {
                if (at < cap) {
                    key[at] = ((u64)qg << 32) | (u64)(~code[h][j]);
                    val[at] = (unsigned)((size_t)tile * CMR_RANGE_TILE + h * RANGE_HALF + tid * 4 + j);
                }
                ++at;
            }
#pragma unroll
        for (int w = 0; w < RANGE_T / 64; ++w) pos += wcnt[h][w];
    }
}
__global__ __launch_bounds__(RANGE_T) void range_compact_kernel(const float* __restrict__ scores, long long ld, size_t n, unsigned lo, unsigned ntiles,
                                                                const unsigned* __restrict__ offs, unsigned q_first, unsigned cap,
                                                                u64* __restrict__ key, unsigned* __restrict__ val) {
    range_compact_body<false>(scores, ld, n, lo, ntiles, offs, q_first, cap, key, val, nullptr, 0, 0u);
}
__global__ __launch_bounds__(RANGE_T) void range_compact_masked_kernel(const float* __restrict__ scores, long long ld, size_t n, unsigned lo, unsigned ntiles,
                                                                       const unsigned* __restrict__ offs, unsigned q_first, unsigned cap, u64* __restrict__ key,
                                                                       unsigned* __restrict__ val, const unsigned* __restrict__ words, long long stride, unsigned mq0) {
    range_compact_body<true>(scores, ld, n, lo, ntiles, offs, q_first, cap, key, val, words, stride, mq0);
}

// sorted pair i of the group: its row (+ id_base) and the bits of its score, gathered from the block
__global__ __launch_bounds__(RANGE_T) void range_finish_kernel(const u64* __restrict__ key, const unsigned* __restrict__ val, unsigned hits, const float* __restrict__ scores,
                                                               long long ld, unsigned q_first, long long id_base, int64_t* __restrict__ out_ids,
                                                               float* __restrict__ out_scores) {
    const size_t i = (size_t)blockIdx.x * RANGE_T + threadIdx.x;
    if (i >= hits) return;
    const unsigned q = q_first + (unsigned)(key[i] >> 32), r = val[i];
    out_ids[i] = (int64_t)r + id_base;
    out_scores[i] = scores[(size_t)q * ld + r];
}

// ------------------------------------------------------------------------------------------ host
static unsigned range_tiles(long long n) { return (unsigned)((n + CMR_RANGE_TILE - 1) / CMR_RANGE_TILE); }

unsigned cmr_range_bound_code(float min_score) {
    if (min_score == __builtin_inff()) return 0xFFFFFFFFu;          // above the code of every score
    unsigned u;
    __builtin_memcpy(&u, &min_score, 4);
    if (u == 0x80000000u) u = 0u;                                   // -0.0 counts as +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

size_t cmr_range_counter_bytes(long long n, int nb) { return ((size_t)nb * range_tiles(n) + 1) * sizeof(unsigned); }

hipError_t cmr_launch_range_count(const float* scores, long long ld, long long n, int nb, unsigned lo, unsigned* cnt, long long* counts, hipStream_t s,
                                  const CmrRangeMask* mask) {
    if (n <= 0 || nb <= 0) return hipSuccess;
    if (n >= (1ll << 32) || (ld & 3)) return hipErrorInvalidValue;
    if (mask && (!mask->words || mask->stride < 0 || mask->q0 < 0)) return hipErrorInvalidValue;
    const unsigned ntiles = range_tiles(n);
    const unsigned long long m = (unsigned long long)nb * ntiles;
    if (m >= (1ull << 31)) return hipErrorInvalidValue;
    if (mask)
        hipLaunchKernelGGL(range_count_masked_kernel, dim3((unsigned)m), dim3(RANGE_T), 0, s, scores, ld, (size_t)n, lo, ntiles, cnt, mask->words, mask->stride,
                           (unsigned)mask->q0);
    else
        hipLaunchKernelGGL(range_count_kernel, dim3((unsigned)m), dim3(RANGE_T), 0, s, scores, ld, (size_t)n, lo, ntiles, cnt);
    hipLaunchKernelGGL(range_offsets_kernel, dim3(1), dim3(1024), 0, s, cnt, (unsigned)m, ntiles, (unsigned)nb, counts);
    return hipGetLastError();
}

hipError_t cmr_launch_range_compact(const float* scores, long long ld, long long n, unsigned lo, const unsigned* offs, int q_first, int nq_group, long long hits,
                                    u64* key, unsigned* val, hipStream_t s, const CmrRangeMask* mask) {
    if (hits <= 0 || nq_group <= 0) return hipSuccess;
    if (n >= (1ll << 32) || hits >= (1ll << 32) || (ld & 3)) return hipErrorInvalidValue;
    if (mask && (!mask->words || mask->stride < 0 || mask->q0 < 0)) return hipErrorInvalidValue;
    const unsigned ntiles = range_tiles(n);
    if (mask)
        hipLaunchKernelGGL(range_compact_masked_kernel, dim3((unsigned)nq_group * ntiles), dim3(RANGE_T), 0, s, scores, ld, (size_t)n, lo, ntiles, offs,
                           (unsigned)q_first, (unsigned)hits, key, val, mask->words, mask->stride, (unsigned)mask->q0);
    else
        hipLaunchKernelGGL(range_compact_kernel, dim3((unsigned)nq_group * ntiles), dim3(RANGE_T), 0, s, scores, ld, (size_t)n, lo, ntiles, offs, (unsigned)q_first,
                           (unsigned)hits, key, val);
    return hipGetLastError();
}

hipError_t cmr_launch_range_finish(const u64* key, const unsigned* val, long long hits, const float* scores, long long ld, int q_first, long long id_base,
                                   int64_t* out_ids, float* out_scores, hipStream_t s) {
    if (hits <= 0) return hipSuccess;
    hipLaunchKernelGGL(range_finish_kernel, dim3((unsigned)((hits + RANGE_T - 1) / RANGE_T)), dim3(RANGE_T), 0, s, key, val, (unsigned)hits, scores, ld, (unsigned)q_first,
                       id_base, out_ids, out_scores);
    return hipGetLastError();
}
