// Diversified top-k (maximal marginal relevance) on the device: DESIGN.md §4.20, include/comorag_hip.h: cmr_index_search_mmr,
// cmr_index_mmr_select, cmr_index_pair_scores.
//   mmr_rows_kernel    candidate ids -> local rows, void positions (negative, not held, repeated) -> -1
//   mmr_gram_kernel    per query the pair scores G[F][F] of its candidates, in 32 x 32 MFMA tiles with the scan's score bits
//   mmr_select_kernel  the greedy selection, one wave per query (the host twin: mmr_select.h)
#include <algorithm>

#include "cmr_device.h"
#include "cmr_kernels.h"

namespace {

// global id -> local row (-1: not a row of this index).  nb <= 1: local = gid - id_base; otherwise through the block table
// [local0[nb] | global0[nb]], as the exact re-score translates its candidates.
__device__ __forceinline__ long long mmr_local_row(long long gid, long long nrows, long long id_base, const long long* __restrict__ tab, int nb) {
    if (gid < 0) return -1;
    long long r;
    if (nb <= 1) r = gid - id_base;
    else {
        int lo = 0, hi = nb - 1;               // last block with global0 <= gid
        if (tab[nb] > gid) return -1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tab[nb + mid] <= gid) lo = mid; else hi = mid - 1;
        }
        const long long len = (lo + 1 < nb ? tab[lo + 1] : nrows) - tab[lo];
        const long long off = gid - tab[nb + lo];
        if (off >= len) return -1;
        r = tab[lo] + off;
    }
    return (r >= 0 && r < nrows) ? r : -1;
}

// one thread per (query, position): ids [nq, F] -> rows [nq, F]
__global__ __launch_bounds__(256) void mmr_rows_kernel(const int64_t* __restrict__ ids, long long total, int F, long long nrows, long long id_base,
                                                       const long long* __restrict__ tab, int nb, long long* __restrict__ rows) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int p = (int)(i % F);
    const int64_t* const mine = ids + (i - p);
    const int64_t id = mine[p];
    long long r = mmr_local_row(id, nrows, id_base, tab, nb);
    for (int e = 0; e < p && r >= 0; ++e) if (mine[e] == id) r = -1;      // an earlier position carries the same id
    rows[i] = r;
}

// One wave per (query, 32 x 32 tile) of G.  Lane l gathers the 16-byte pieces of corpus row rows[32 tc + (l & 31)] straight from the
// panels — slot (row & 31) + 32 (l >> 5) of every block of the row's panel — which IS the A-operand of a panel made of those 32
// candidates (q8_rescore_kernel gathers its candidates the same way).  The B-operand — the "query" side, positions 32 ts + (l & 31) —
// is the same gather (a stored row's slot is its query fragment: rounding an already rounded value changes nothing), or, with `qfrag`,
// a fragment buffer in prep_queries_kernel's layout [q * T + ts][ks][64] (the shard path: rows another shard may hold, sent as fp32
// queries).  Then the scan's chain: zero accumulator, CmrBlk<DT>::mma(corpus block, query block, acc) for ks = 0 .. KS - 1 ascending.  An
// element of the result depends on its own row and column only, so G[s][c] has the bits cmr_index_scores returns for (query = stored
// row s, corpus row c).  Void rows load nothing and give -inf rows and columns.
template <int DT>
__global__ __launch_bounds__(64) void mmr_gram_kernel(const v4u* __restrict__ corpus, const v4u* __restrict__ qfrag, const long long* __restrict__ rows,
                                                      int q0, int F, int T, int KS, float* __restrict__ out) {
    const int lane = threadIdx.x;
    const int q = q0 + blockIdx.y;
    const int tc = blockIdx.x % T, ts = blockIdx.x / T;
    const long long* const qrows = rows + (size_t)q * F;
    const int ca = tc * 32 + (lane & 31), sb = ts * 32 + (lane & 31);
    const long long ra = ca < F ? qrows[ca] : -1;
    const long long rb = sb < F ? qrows[sb] : -1;
    const bool have_a = ra >= 0;
    const bool have_b = qfrag ? sb < F : rb >= 0;
    const unsigned half = 32u * (unsigned)(lane >> 5);
    const v4u* const asrc = corpus + (have_a ? (size_t)(ra >> 5) * KS * 64 + (size_t)(ra & 31) + half : 0);
    const v4u* const bsrc = qfrag ? qfrag + ((size_t)q * T + ts) * KS * 64 + lane
                                  : corpus + (have_b ? (size_t)(rb >> 5) * KS * 64 + (size_t)(rb & 31) + half : 0);
    const v4u zero = {0u, 0u, 0u, 0u};
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int ks0 = 0; ks0 < KS; ks0 += 8) {      // (KS is a multiple of 8: rows are padded to 128 elements)
        v4u a[8], b[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            a[u] = have_a ? asrc[(size_t)(ks0 + u) * 64] : zero;
            b[u] = have_b ? bsrc[(size_t)(ks0 + u) * 64] : zero;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = CmrBlk<DT>::mma(a[u], b[u], acc);
    }
    const int ok_a = have_a ? 1 : 0;
    float* const o = out + ((size_t)q * F + (sb < F ? sb : 0)) * F;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = cmr_acc_row(r, lane);
        const int c = tc * 32 + i;
        const int col_ok = __shfl(ok_a, i);
        if (sb < F && c < F) o[c] = (col_ok && have_b) ? acc[r] : -__builtin_inff();
    }
}

// One wave per query; lane l owns positions l and l + 64 (F <= 128).  val = (lam * rel) - ((1 - lam) * pen), each product rounded
// to fp32 before the subtraction; the argmax over (val, lowest position) is a butterfly over the wave, so every lane ends with the
// same winner and no atomic decides a pick.  pen folds row G[winner][.] after each pick.
__global__ __launch_bounds__(64) void mmr_select_kernel(const int64_t* __restrict__ ids, const float* __restrict__ rel, const long long* __restrict__ rows,
                                                        const float* __restrict__ gram, int F, int k, float lam32, int64_t* __restrict__ out_ids,
                                                        float* __restrict__ out_scores) {
    const int lane = threadIdx.x;
    const size_t q = blockIdx.x;
    const int64_t* const qi = ids + q * F;
    const float* const qr = rel + q * F;
    const long long* const qrow = rows + q * F;
    const float* const G = gram + q * F * F;
    const int p0 = lane, p1 = lane + 64;
    bool open0 = p0 < F && qrow[p0] >= 0, open1 = p1 < F && qrow[p1] >= 0;
    const float rel0 = p0 < F ? qr[p0] : 0.0f, rel1 = p1 < F ? qr[p1] : 0.0f;
    float pen0 = -__builtin_inff(), pen1 = -__builtin_inff();
    const float oml = __fsub_rn(1.0f, lam32);
    int n = 0;
    for (; n < k; ++n) {
        const float v0 = n == 0 ? rel0 : __fsub_rn(__fmul_rn(lam32, rel0), __fmul_rn(oml, pen0));
        const float v1 = n == 0 ? rel1 : __fsub_rn(__fmul_rn(lam32, rel1), __fmul_rn(oml, pen1));
        int have = open0 ? 1 : 0;
        float bv = v0;
        int bp = p0;
        if (open1 && (!have || v1 > bv)) { have = 1; bv = v1; bp = p1; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int oh = __shfl_xor(have, off);
            const float ov = __shfl_xor(bv, off);
            const int op = __shfl_xor(bp, off);
            if (oh && (!have || ov > bv || (ov == bv && op < bp))) { have = 1; bv = ov; bp = op; }
        }
        if (!have) break;      // (wave-uniform: every lane holds the same reduction)
        if (lane == 0) { out_ids[q * k + n] = qi[bp]; out_scores[q * k + n] = qr[bp]; }
        if (bp == p0) open0 = false;
        if (bp == p1) open1 = false;
        const float* const g = G + (size_t)bp * F;
        if (p0 < F) { const float x = g[p0]; pen0 = x > pen0 ? x : pen0; }
        if (p1 < F) { const float x = g[p1]; pen1 = x > pen1 ? x : pen1; }
    }
    for (int j = n + lane; j < k; j += 64) { out_ids[q * k + j] = -1; out_scores[q * k + j] = -__builtin_inff(); }
}

}  // namespace

// ------------------------------------------------------------------------------------------ host
hipError_t cmr_launch_mmr_rows(const int64_t* ids, int nq, int F, long long nrows, long long id_base, const long long* tab, int nb, long long* rows,
                               hipStream_t s) {
    const long long total = (long long)nq * F;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(mmr_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, ids, total, F, nrows, id_base, tab, nb, rows);
    return hipGetLastError();
}

// qfrag: nullptr (both operands gathered from the panels) or fragments [nq * T][KS][64] of the padded candidate rows, T = ceil(F / 32)
hipError_t cmr_launch_mmr_gram(int dtype, const void* corpus, const void* qfrag, const long long* rows, int nq, int F, int dpad, float* out,
                               hipStream_t s) {
    if (nq <= 0 || F <= 0 || F > 128) return hipErrorInvalidValue;
    const int T = (F + 31) / 32;
    const int KS = dtype == CMR_DT_F32 ? dpad / 8 : dpad / 16;
    if (KS % 8) return hipErrorInvalidValue;
    const v4u* c = reinterpret_cast<const v4u*>(corpus);
    const v4u* f = reinterpret_cast<const v4u*>(qfrag);
    for (int q0 = 0; q0 < nq; q0 += 32768) {
        const dim3 grid((unsigned)(T * T), (unsigned)std::min(32768, nq - q0)), block(64);
        switch (dtype) {
            case CMR_DT_BF16: hipLaunchKernelGGL(mmr_gram_kernel<CMR_DT_BF16>, grid, block, 0, s, c, f, rows, q0, F, T, KS, out); break;
            case CMR_DT_F16:  hipLaunchKernelGGL(mmr_gram_kernel<CMR_DT_F16>, grid, block, 0, s, c, f, rows, q0, F, T, KS, out); break;
            case CMR_DT_F32:  hipLaunchKernelGGL(mmr_gram_kernel<CMR_DT_F32>, grid, block, 0, s, c, f, rows, q0, F, T, KS, out); break;
            default: return hipErrorInvalidValue;
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t cmr_launch_mmr_select(const int64_t* ids, const float* rel, const long long* rows, const float* gram, int nq, int F, int k, float lam32,
                                 int64_t* out_ids, float* out_scores, hipStream_t s) {
    if (nq <= 0 || F <= 0 || F > 128 || k <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mmr_select_kernel, dim3((unsigned)nq), dim3(64), 0, s, ids, rel, rows, gram, F, k, lam32, out_ids, out_scores);
    return hipGetLastError();
}
