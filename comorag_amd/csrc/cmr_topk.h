// The slow path of the top-k scans: candidate keys of one 32x32 score tile into the (wave, query) lists, and the compaction of a list
// that is nearly full.  Shared by scan_kernels.hip and prefilter_kernels.hip.
#pragma once
#include "cmr_device.h"

// Slow path, part 1 (inline, a handful of registers, no waits on global memory): push the keys of
// one 32x32 score tile that beat the lane's threshold into the (wave, query) lists.  Returns the
// mask of this tile's queries whose list is nearly full.
// `valid`: bit i = row row0 + i of the tile may be pushed for THIS LANE's query (lane & 31).  The corpus' last, partial panel is
// topk_tail_mask(row0, nrows); a filtered scan ANDs its panel's word of the caller's allow bitmap into it — one word for the
// whole wave (shared mask) or a word per query column (per-query masks): the shift and the compile-time bit tests below are
// per lane either way.
__device__ __forceinline__ unsigned topk_tail_mask(long long row0, long long nrows) {
    const long long left = nrows - row0;
    return left >= 32 ? 0xFFFFFFFFu : left <= 0 ? 0u : (1u << (int)left) - 1u;
}
template <int CAP>
__device__ __forceinline__ u64 topk_push(const f32x16& acc, long long row0, unsigned valid, u64 tau_key, int* cnt_t,
                                         u64* list_t, int lane) {
    const int ql = lane & 31;
    const unsigned hrow = 4u * (unsigned)(lane >> 5);
    // this lane's rows of the panel are (r & 3) + 8 * (r >> 2) + hrow: shifted by hrow once, the bit of accumulator register r sits at a
    // compile-time position (sixteen lane-dependent masks 1 << row would be loop-invariant values hipcc keeps in registers across the scan)
    const unsigned vh = valid >> hrow;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = acc[r];
        const long long row = row0 + (r & 3) + 8 * (r >> 2) + hrow;
        const u64 key = cmr_make_key(v, (unsigned)row);
        if ((vh & (1u << ((r & 3) + 8 * (r >> 2)))) && v == v && key > tau_key) {
            const int slot = atomicAdd(&cnt_t[ql], 1);  // ds_add_rtn_u32; <= 32 pushes per query per panel
            list_t[(size_t)ql * CAP + slot] = key;
        }
    }
    // LDS ops of one wave complete in order, so the counters are current without any fence.  The
    // pushed keys themselves are only read back by a compaction, which fences (s_waitcnt vmcnt(0))
    // itself — a fence on every slow-path entry would drain the load ring / DMA ring each time.
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int c = __hip_atomic_load(&cnt_t[ql], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __ballot(c > CAP - 32) & 0xFFFFFFFFull;
}

// Slow path, part 2 (rare): compact every list in `need` to its k best keys (rank by counting; keys
// are unique so ranks are a permutation) and raise the owning lanes' thresholds.
template <int CAP>
__device__ __forceinline__ void topk_compact(u64 need, int k, u64& tau_key, float& tau_f, int* cnt_t, u64* list_t, u64* stage,
                                             int lane) {
    constexpr int EPL = CAP / 64;
    const int ql = lane & 31;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // pushes landed (same-CU L1 is coherent)
    while (need) {
        const int j = __ffsll((long long)need) - 1;
        need &= need - 1;
        const int n = __builtin_amdgcn_readfirstlane(
            __hip_atomic_load(&cnt_t[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
        u64* L = list_t + (size_t)j * CAP;
        u64 e[EPL];
        int rk[EPL];
#pragma unroll
        for (int i = 0; i < EPL; ++i) {
            const int idx = lane + 64 * i;
            e[i] = idx < n ? L[idx] : 0ull;
            stage[idx] = e[i];
            rk[i] = 0;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        for (int jj = 0; jj < n; ++jj) {
            const u64 kj = stage[jj];  // uniform address: LDS broadcast
#pragma unroll
            for (int i = 0; i < EPL; ++i) rk[i] += (kj > e[i]) ? 1 : 0;
        }
#pragma unroll
        for (int i = 0; i < EPL; ++i) {
            const int idx = lane + 64 * i;
            if (idx < n && rk[i] < k) L[rk[i]] = e[i];
            if (idx < n && rk[i] == k - 1) stage[CAP] = e[i];
        }
        if (lane == 0) __hip_atomic_store(&cnt_t[j], n < k ? n : k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        if (n >= k) {
            const u64 nt = stage[CAP];
            // (never downwards: with the finishing stage a list still holds what the wave pushed before it adopted the published
            // threshold — the k-th best of THAT is no bound worth having)
            if (ql == j && nt > tau_key) { tau_key = nt; tau_f = cmr_key_score(nt); }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
}

template <int CAP>
__device__ __forceinline__ void topk_slow_path(const f32x16& acc, long long row0, unsigned valid, int k,
                                               u64& tau_key, float& tau_f, int* cnt_t, u64* list_t,
                                               u64* stage, int lane) {
    const u64 need = topk_push<CAP>(acc, row0, valid, tau_key, cnt_t, list_t, lane);
    if (need) topk_compact<CAP>(need, k, tau_key, tau_f, cnt_t, list_t, stage, lane);
}
