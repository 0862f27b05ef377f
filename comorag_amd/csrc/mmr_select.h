// Greedy maximal-marginal-relevance selection on host arrays (include/comorag_hip.h: cmr_mmr_select).  Plain C++, no
// HIP: the shard path of cmr_mindex_search_mmr / cmr_mindex_mmr_select runs it, tools/mmr_selftest.cpp drives it without a device, and
// mmr_select_kernel (mmr_kernels.hip) is the same arithmetic on the device — fp32, both products rounded before the subtraction, no
// fused multiply-add, IEEE comparisons, ties to the lowest position.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace cmr_mmr {

// One query.  rel [F], gram [F, F] (gram[s * F + c] = pair(ids[s], ids[c])), ids [F]; out_ids / out_scores [k], in pick order, -1 / -inf
// padded.  A position is void when its id is negative, when an earlier position carries the same id, or when extra_void (may be NULL)
// marks it; void positions are never picked and never penalise.
inline void select_one(const float* rel, const float* gram, const int64_t* ids, int F, int k, float lam32, const unsigned char* extra_void,
                       int64_t* out_ids, float* out_scores) {
#if defined(__clang__)
#pragma clang fp contract(off)      // (hipcc contracts a * b - c * d by default, on the host too)
    typedef float rounded_t;
#else
    typedef volatile float rounded_t;   // another compiler: each product goes through memory, so it is rounded before the subtraction
#endif
    std::vector<unsigned char> open((size_t)F);      // non-void and not picked yet
    std::vector<float> pen((size_t)F, -INFINITY);
    for (int p = 0; p < F; ++p) {
        bool v = ids[p] < 0 || (extra_void && extra_void[p]);
        for (int e = 0; e < p && !v; ++e) v = ids[e] == ids[p];
        open[p] = !v;
    }
    const float oml = 1.0f - lam32;
    int n = 0;
    for (; n < k; ++n) {
        int best = -1;
        float bv = 0.0f;
        for (int c = 0; c < F; ++c) {
            if (!open[c]) continue;
            float val = rel[c];
            if (n > 0) {
                rounded_t a = lam32 * rel[c];
                rounded_t b = oml * pen[c];
                val = a - b;
            }
            if (best < 0 || val > bv) { best = c; bv = val; }
        }
        if (best < 0) break;
        out_ids[n] = ids[best];
        out_scores[n] = rel[best];
        open[best] = 0;
        const float* g = gram + (size_t)best * F;
        for (int c = 0; c < F; ++c) pen[c] = g[c] > pen[c] ? g[c] : pen[c];
    }
    for (; n < k; ++n) { out_ids[n] = -1; out_scores[n] = -INFINITY; }
}

// nq queries: rel [nq, F], gram [nq, F, F], ids [nq, F] -> out_ids / out_scores [nq, k]
inline void select(const float* rel, const float* gram, const int64_t* ids, int nq, int F, int k, float lam32, int64_t* out_ids,
                   float* out_scores) {
    for (int q = 0; q < nq; ++q)
        select_one(rel + (size_t)q * F, gram + (size_t)q * F * F, ids + (size_t)q * F, F, k, lam32, nullptr, out_ids + (size_t)q * k,
                   out_scores + (size_t)q * k);
}

// the argument rules every MMR entry point checks before it looks at its handle: 0 = fine, 1 = invalid, 2 = unsupported (F too large)
inline int check_args(int nq, int F, int k, double lam, int max_f) {
    if (nq < 1 || k < 1 || k > F) return 1;
    if (!(lam >= 0.0 && lam <= 1.0)) return 1;      // (refuses NaN too)
    if (F > max_f) return 2;
    return 0;
}

inline bool any_nan(const float* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (v[i] != v[i]) return true;
    return false;
}

}  // namespace cmr_mmr
