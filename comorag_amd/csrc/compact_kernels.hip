// Row removal by stable in-place compaction (cmr_index_remove_ids): a prefix sum over the keep words, then the
// corpus' 16-byte slots (any dtype: a row is 2 * ks slots at a fixed stride, see convert_rows_kernel) and the fp32 shadow's rows
// move towards the front chunk by chunk through a bounded staging buffer.  Launch A(c) reads the source panels of chunk c and
// writes the kept rows' slots into the staging buffer at their destination position; launch B(c) copies them from there into the
// corpus.  Everything is ordered by the ONE stream the launches go to: no workgroup ever waits for another one.
//   kept_before[p] = kept rows in front of panel p (exclusive prefix of the words' popcounts), kept_before[npanels] = all of them;
//   a kept row r of panel p moves to j = kept_before[p] + popc(word[p] & ((1 << (r & 31)) - 1)) <= r.
// B(c) writes the destination rows [D_c, D_c + kept_c) with D_c = kept_before[first panel of chunk c]; D_c + kept_c = D_(c+1) <=
// 32 * (first panel of chunk c + 1): rows of source chunks <= c only, all of which A(0..c) have read earlier on the stream.
#include <algorithm>

#include "cmr_device.h"
#include "cmr_internal.h"
#include "cmr_kernels.h"

namespace {

constexpr int kScanThreads = 1024;

// One workgroup walks the words in tiles of kScanThreads: wave-level inclusive scan by shuffles, the 16 wave totals through the LDS,
// the running total carried from tile to tile.  info[0] = kept rows, info[1] = the first removed row (the first clear bit below
// `size`; `size` when there is none).  Bits at or beyond `size` are zero in the words (row_mask_fill) and are not "removed rows".
__global__ __launch_bounds__(kScanThreads) void keep_prefix_kernel(const unsigned* __restrict__ words, long long n_words, long long size,
                                                                   unsigned* __restrict__ kept_before, long long* __restrict__ info) {
    __shared__ unsigned wave_sum[kScanThreads / 64];
    __shared__ unsigned long long first_clear[kScanThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned carry = 0;
    unsigned long long first = (unsigned long long)size;
    for (long long p0 = 0; p0 < n_words; p0 += kScanThreads) {
        const long long p = p0 + tid;
        const unsigned w = p < n_words ? words[p] : 0u;
        if (p < n_words) {
            const long long rows_here = size - p * 32 >= 32 ? 32 : size - p * 32;      // (> 0: n_words = ceil(size / 32))
            const unsigned full = rows_here >= 32 ? 0xFFFFFFFFu : (1u << (unsigned)rows_here) - 1u;
            const unsigned gone = full & ~w;
            if (gone) first = min(first, (unsigned long long)(p * 32 + __ffs((int)gone) - 1));
        }
        const unsigned c = (unsigned)__popc(w);
        unsigned incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        unsigned before = carry, total = 0;
#pragma unroll
        for (int v = 0; v < kScanThreads / 64; ++v) {
            const unsigned sv = wave_sum[v];
            if (v < wave) before += sv;
            total += sv;
        }
        if (p < n_words) kept_before[p] = before + incl - c;
        carry += total;
        __syncthreads();
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) first = min(first, (unsigned long long)__shfl_xor((long long)first, d, 64));
    if (lane == 0) first_clear[wave] = first;
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < kScanThreads / 64; ++v) first = min(first, first_clear[v]);
        kept_before[n_words] = carry;
        info[0] = (long long)carry;
        info[1] = (long long)first;
    }
}

// A(c): one wave per (source panel, k-step block) of the panels [p_first, p_end); lane = half * 32 + row of the panel, adjacent lanes on
// adjacent slots.  stage holds the destination panels from panel kept_before[p_first] / 32 on, in the corpus' own slot order.
__global__ __launch_bounds__(256) void compact_stage_kernel(const uint4* __restrict__ corpus, const unsigned* __restrict__ words,
                                                            const unsigned* __restrict__ kept_before, long long p_first, long long p_end, int ks_total,
                                                            long long stage_panels, uint4* __restrict__ stage) {
    const long long wv = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63, r = lane & 31;
    const long long panel = p_first + wv / ks_total;
    const int ks = (int)(wv % ks_total);
    if (panel >= p_end) return;
    const unsigned w = words[panel];
    if (!((w >> r) & 1u)) return;
    const uint4 v = corpus[((size_t)panel * ks_total + ks) * 64 + lane];
    const long long j = (long long)kept_before[panel] + __popc(w & ((1u << r) - 1u));
    const long long jp = (j >> 5) - ((long long)kept_before[p_first] >> 5);
    if (jp < 0 || jp >= stage_panels) return;      // (cannot happen: a chunk's destination rows span at most its panels + 1)
    stage[((size_t)jp * ks_total + ks) * 64 + (lane & 32) + (int)(j & 31)] = v;
}

// B(c): the slots of the destination rows [D, D + kept) with D = kept_before[p_first], kept = kept_before[p_end] - D, from the staging
// buffer into the corpus; one wave per (destination panel, k-step block) of the stage_panels panels from panel D / 32 on.  A slot
// outside the row range is neither read nor written: a destination panel that two chunks share is written in disjoint slots.
__global__ __launch_bounds__(256) void compact_place_kernel(uint4* __restrict__ corpus, const unsigned* __restrict__ kept_before, long long p_first,
                                                            long long p_end, int ks_total, long long stage_panels, const uint4* __restrict__ stage) {
    const long long wv = ((long long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    const long long jp = wv / ks_total;
    const int ks = (int)(wv % ks_total);
    if (jp >= stage_panels) return;
    const long long d0 = kept_before[p_first], d1 = kept_before[p_end];
    const long long panel = (d0 >> 5) + jp, j = panel * 32 + (lane & 31);
    if (j < d0 || j >= d1) return;
    corpus[((size_t)panel * ks_total + ks) * 64 + lane] = stage[((size_t)jp * ks_total + ks) * 64 + lane];
}

// The fp32 shadow, row-major [*, dim], at row granularity: T = float4 when dim is a multiple of 4 (vpr = dim / 4 elements per row),
// else float.  A: the kept rows of the panels [p_first, p_end) to stage row j - D; B: stage rows [0, kept) to shadow rows [D, D + kept).
template <typename T>
__global__ __launch_bounds__(256) void shadow_stage_kernel(const T* __restrict__ shadow, const unsigned* __restrict__ words,
                                                           const unsigned* __restrict__ kept_before, long long p_first, long long p_end, int vpr,
                                                           long long stage_rows, T* __restrict__ stage) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = p_first * 32 + i / vpr;
    const int e = (int)(i % vpr);
    if (row >= p_end * 32) return;
    const unsigned w = words[row >> 5];
    const int r = (int)(row & 31);
    if (!((w >> r) & 1u)) return;
    const long long j = (long long)kept_before[row >> 5] + __popc(w & ((1u << r) - 1u)) - (long long)kept_before[p_first];
    if (j < 0 || j >= stage_rows) return;          // (cannot happen: a chunk keeps at most its own rows)
    stage[(size_t)j * vpr + e] = shadow[(size_t)row * vpr + e];
}
template <typename T>
__global__ __launch_bounds__(256) void shadow_place_kernel(T* __restrict__ shadow, const unsigned* __restrict__ kept_before, long long p_first,
                                                           long long p_end, int vpr, const T* __restrict__ stage) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long d0 = kept_before[p_first], d1 = kept_before[p_end];
    if (i >= (d1 - d0) * vpr) return;
    shadow[(size_t)d0 * vpr + i] = stage[i];
}

}  // namespace

hipError_t cmr_launch_keep_prefix(const unsigned* words, long long n_words, long long size, unsigned* kept_before, long long* info, hipStream_t s) {
    hipLaunchKernelGGL(keep_prefix_kernel, dim3(1), dim3(kScanThreads), 0, s, words, n_words, size, kept_before, info);
    return hipGetLastError();
}

hipError_t cmr_launch_compact_chunk(void* corpus, int ks, const unsigned* words, const unsigned* kept_before, long long p_first, long long p_end,
                                    void* stage, long long stage_panels, hipStream_t s) {
    if (p_end <= p_first) return hipSuccess;
    if (p_end - p_first + 1 > stage_panels) return hipErrorInvalidValue;
    const long long waves_a = (p_end - p_first) * ks, waves_b = (p_end - p_first + 1) * ks;
    hipLaunchKernelGGL(compact_stage_kernel, dim3((unsigned)((waves_a + 3) / 4)), dim3(256), 0, s, (const uint4*)corpus, words, kept_before, p_first, p_end,
                       ks, p_end - p_first + 1, (uint4*)stage);
    hipLaunchKernelGGL(compact_place_kernel, dim3((unsigned)((waves_b + 3) / 4)), dim3(256), 0, s, (uint4*)corpus, kept_before, p_first, p_end, ks,
                       p_end - p_first + 1, (const uint4*)stage);
    return hipGetLastError();
}

hipError_t cmr_launch_compact_shadow_chunk(float* shadow, int dim, const unsigned* words, const unsigned* kept_before, long long p_first,
                                           long long p_end, void* stage, long long stage_rows, hipStream_t s) {
    if (p_end <= p_first) return hipSuccess;
    if ((p_end - p_first) * CMR_PANEL_ROWS > stage_rows) return hipErrorInvalidValue;
    const bool v4 = dim % 4 == 0;
    const int vpr = v4 ? dim / 4 : dim;
    const long long items = (p_end - p_first) * CMR_PANEL_ROWS * vpr;
    const dim3 grid((unsigned)((items + 255) / 256)), block(256);
    if (v4) {
        hipLaunchKernelGGL(shadow_stage_kernel<float4>, grid, block, 0, s, (const float4*)shadow, words, kept_before, p_first, p_end, vpr, stage_rows, (float4*)stage);
        hipLaunchKernelGGL(shadow_place_kernel<float4>, grid, block, 0, s, (float4*)shadow, kept_before, p_first, p_end, vpr, (const float4*)stage);
    } else {
        hipLaunchKernelGGL(shadow_stage_kernel<float>, grid, block, 0, s, (const float*)shadow, words, kept_before, p_first, p_end, vpr, stage_rows, (float*)stage);
        hipLaunchKernelGGL(shadow_place_kernel<float>, grid, block, 0, s, (float*)shadow, kept_before, p_first, p_end, vpr, (const float*)stage);
    }
    return hipGetLastError();
}
