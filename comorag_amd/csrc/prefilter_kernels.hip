// Certified int8 pre-filter of the pipelined 16-bit top-k scan.
//
// The corpus keeps a half-size companion: every stored row x quantised to int8 with a scale of its own, m = rint(x / a),
// a = max|x| / 127, and b >= ||x - a m|| beside it.  A batch's main pass streams the companion instead of the 16-bit panels
// (q8_filter_kernel) and records the (row, query) pairs whose 16-bit score could still beat the query's sampling threshold — decided
// with a proven bound on |scan score - int8 score| — with their upper and lower bounds.  q8_tighten_kernel raises every query's
// threshold to the k-th largest LOWER bound among its pairs (k distinct rows score at least that much, so a row whose upper bound
// is strictly below it cannot be among the k best) and marks the rows still standing in a bit mask per panel, q8_expand_kernel
// lists the marked rows, and those few are scored again from the 16-bit panels by the scan's own MFMA chain (q8_rescore_kernel),
// so the candidate lists hold the same keys, bit for bit, that scan_kernel would have pushed for those rows.
// merge_query_kernel then selects as ever.
//
// Layout.  One int8 block = 1 KiB = the A-operand of v_mfma_i32_32x32x32_i8 for 32 rows x 32 k in lane order; a panel of 32
// rows is dpad / 32 blocks.  Lane l of block kb holds row (l & 31) and the sixteen k of the lane's OWN slots in the 16-bit
// blocks 2 kb and 2 kb + 1 (bytes 0..7: k = 32 kb + 8 (l >> 5) + e, bytes 8..15: k = 32 kb + 16 + 8 (l >> 5) + e): the
// quantiser reads and writes perfectly coalesced, and integer sums do not care about the order.  Queries are packed alike.
#include "cmr_device.h"
#include "cmr_kernels.h"
#include "cmr_topk.h"

typedef __attribute__((ext_vector_type(16))) int i32x16;
typedef __attribute__((ext_vector_type(4))) int i32x4;

namespace {

template <int DT> __device__ __forceinline__ float q8_elem(unsigned short h) { return DT == CMR_DT_BF16 ? cmr_bf2f(h) : cmr_h2f(h); }
template <int DT> __device__ __forceinline__ unsigned short q8_round(float f) { return DT == CMR_DT_BF16 ? cmr_f2bf(f) : cmr_f2h(f); }

// the eight 16-bit elements of one lane slot as fp32
template <int DT> __device__ __forceinline__ void q8_unpack(const v4u& v, float (&x)[8]) {
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = q8_elem<DT>((unsigned short)(w[e >> 1] >> (16 * (e & 1))));
}

// d >= 0 -> the smallest float that is not below it
__device__ __forceinline__ float q8_up(double d) {
    float f = (float)d;
    if ((double)f < d) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}

__device__ __forceinline__ int q8_clamp(float v) { return (int)fminf(fmaxf(rintf(v), -127.0f), 127.0f); }

// ------------------------------------------------------------------------------------------ companion
// One wave per panel: per row the scale a = max|x| / 127, the int8 row m = rint(x / a) and b >= ||x - a m|| (fp64 sum of the
// exact differences, rounded up); rows at or beyond nrows count as zero rows.  stats[0] / stats[1]: atomicMax (float bits,
// values >= 0) of ||x|| / of b over the rows written.
template <int DT>
__global__ __launch_bounds__(256) void q8_quantise_kernel(const v4u* __restrict__ corpus, int KS, long long panel0, long long npanels, long long nrows,
                                                          v4u* __restrict__ q8, float2* __restrict__ scales, float* __restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const long long pi = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pi >= npanels) return;
    const long long P = panel0 + pi;
    const long long row = P * CMR_PANEL_ROWS + (lane & 31);
    const bool live = row < nrows;
    const v4u* src = corpus + (size_t)P * KS * 64 + lane;
    float mx = 0.0f;
    for (int ks = 0; ks < KS; ++ks) {
        float x[8];
        q8_unpack<DT>(src[(size_t)ks * 64], x);
#pragma unroll
        for (int e = 0; e < 8; ++e) mx = fmaxf(mx, fabsf(x[e]));
    }
    if (!live) mx = 0.0f;
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float a = mx / 127.0f;
    double se = 0.0, sx = 0.0;
    const int KB = KS / 2;
    for (int kb = 0; kb < KB; ++kb) {
        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            float x[8];
            q8_unpack<DT>(src[(size_t)(2 * kb + half) * 64], x);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float xv = live ? x[e] : 0.0f;
                const int m = a > 0.0f ? q8_clamp(xv / a) : 0;
                const double d = (double)xv - (double)a * (double)m;
                se += d * d;
                sx += (double)xv * (double)xv;
                const int b = 8 * half + e;
                w[b >> 2] |= (unsigned)(m & 255) << (8 * (b & 3));
            }
        }
        q8[((size_t)P * KB + kb) * 64 + lane] = (v4u){w[0], w[1], w[2], w[3]};
    }
    se += __shfl_xor(se, 32);
    sx += __shfl_xor(sx, 32);
    const float b = q8_up(sqrt(se)), nx = q8_up(sqrt(sx));
    if (lane < 32) scales[P * CMR_PANEL_ROWS + lane] = make_float2(a, b);
    float wb = b, wn = nx;
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) { wb = fmaxf(wb, __shfl_xor(wb, off)); wn = fmaxf(wn, __shfl_xor(wn, off)); }
    if (lane == 0) {
        atomicMax(reinterpret_cast<int*>(stats), __float_as_int(wn));
        atomicMax(reinterpret_cast<int*>(stats) + 1, __float_as_int(wb));
    }
}

// ------------------------------------------------------------------------------------------ queries
// One workgroup per query slot: the query as prep_queries_kernel rounds it (q~), in two int8 parts n_hi = rint(q~ / a_q),
// n_lo = rint((q~ / a_q - n_hi) 254), a_q = max|q~| / 127, packed in block order ([part][tile][kb][lane]), and the query's
// constants (a_q, B_q, c_q): with Q^ = a_q (n_hi + n_lo / 254) and f = q~ - Q^,
//   |scan score - int8 score| <= B_q b_r + c_q,   B_q = ||Q^||,   c_q = (||f|| + gamma ||q~|| + 2^-20 ||Q^||) M_x
// (gamma = dpad 2^-23: the scan's fp32 accumulation; the 2^-20 term: the fp32 evaluation of the int8 score and of
// the kept-test — a handful of roundings of values below 2 ||Q^|| M_x), everything rounded up by (1 + 1e-5) (+ 1e-7 for c_q).
template <int DT>
__global__ __launch_bounds__(256) void q8_pack_queries_kernel(const float* __restrict__ q, int nq, int dim, int dpad, int tiles,
                                                              const float* __restrict__ stats, signed char* __restrict__ qpack,
                                                              float4* __restrict__ qconst) {
    __shared__ float s_mx[4];
    __shared__ double s_sum[3][4];
    const int qi = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int KB = dpad / 32;
    const bool live = qi < nq;
    const float* src = q + (size_t)qi * dim;
    float mx = 0.0f;
    if (live)
        for (int k = tid; k < dim; k += 256) mx = fmaxf(mx, fabsf(q8_elem<DT>(q8_round<DT>(src[k]))));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if (lane == 0) s_mx[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
    const float a = mx / 127.0f;
    double sQ = 0.0, sf = 0.0, sq = 0.0;
    const int t = qi >> 5, col = qi & 31;
    for (int k = tid; k < dpad; k += 256) {
        const float x = (live && k < dim) ? q8_elem<DT>(q8_round<DT>(src[k])) : 0.0f;
        int hi = 0, lo = 0;
        if (a > 0.0f) {
            const float u = x / a;
            hi = q8_clamp(u);
            lo = q8_clamp((u - (float)hi) * 254.0f);
        }
        const double Q = (double)a * ((double)hi + (double)lo / 254.0);
        const double f = (double)x - Q;
        sQ += Q * Q; sf += f * f; sq += (double)x * (double)x;
        const int kb = k >> 5, w = k & 31;
        const int h = (w & 15) >> 3, e = (w & 7) + ((w >> 4) << 3);
        const size_t at = (((size_t)t) * KB + kb) * 1024 + (size_t)(col + 32 * h) * 16 + e;
        qpack[at] = (signed char)hi;
        qpack[(size_t)tiles * KB * 1024 + at] = (signed char)lo;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { sQ += __shfl_xor(sQ, off); sf += __shfl_xor(sf, off); sq += __shfl_xor(sq, off); }
    if (lane == 0) { s_sum[0][wave] = sQ; s_sum[1][wave] = sf; s_sum[2][wave] = sq; }
    __syncthreads();
    if (tid == 0) {
        const double nQ = sqrt(s_sum[0][0] + s_sum[0][1] + s_sum[0][2] + s_sum[0][3]);
        const double nf = sqrt(s_sum[1][0] + s_sum[1][1] + s_sum[1][2] + s_sum[1][3]);
        const double nq2 = sqrt(s_sum[2][0] + s_sum[2][1] + s_sum[2][2] + s_sum[2][3]);
        const double Mx = (double)stats[0];
        const double gamma = (double)dpad * (1.0 / 8388608.0);
        const double c = (nf + gamma * nq2 + nQ * (1.0 / 1048576.0)) * Mx * (1.0 + 1e-5) + 1e-7;
        qconst[qi] = make_float4(a, q8_up(nQ * (1.0 + 1e-5)), q8_up(c), 0.0f);
    }
}

// ------------------------------------------------------------------------------------------ filter
struct FilterP {
    const v4u* q8;
    const float4* scales4;     // (a, b) pairs, two rows per float4
    const v4u* qpack;
    const float4* qconst;
    const u64* tau_init;       // per-query threshold keys of the sampling passes, or nullptr (nothing to filter by)
    long long nrows;
    int npanels, KB, nq, keep_all;
    v4u* wrec;                 // [W][wave_cap] records (row, ub, lb, query slot): wave gw of the grid owns row gw
    unsigned* wcnt;            // [W] records offered by each wave (written by every wave of the grid; may run past wave_cap)
    unsigned wave_cap;         // 0: no records, every hit is kept directly
    unsigned* keep;            // [npanels] row masks: every panel's word is written (the rows kept directly, usually none)
    int s_run, s_stride, s_nruns;      // sample mode: wave gw < s_nruns takes the s_run panels from gw * s_stride (s_stride >= s_run)
};

// 8 waves per workgroup, each with a contiguous panel range; the two int8 parts of the query tiles in LDS.  Corpus blocks
// stream through two register buffers of CH blocks (plain non-temporal loads, the compiler counts them): one is in flight
// while the other feeds the MFMAs — two per block and query tile, hi and lo part.  The scheduling barrier that ends load()
// is what makes that true in the ISA: without it the compiler sinks the next buffer's loads behind most of the step's MFMAs
// (it likes the registers as ds_read temporaries) and the wave drains its one buffer while it computes.
// Panel epilogue: the kept-test on every accumulator element (the padding rows of the corpus' last panel masked out: a zero row
// scores 0 and must not reach the threshold selection), __any; on a hit, per accumulator row and tile, a ballot: the hitting
// lanes take consecutive slots of the WAVE's own record area — a wave-uniform count, no atomic, nothing to wait for, so the
// corpus loads stay in flight across it — and store (row, ub, lb, query slot); q8_bucket_kernel sorts the records into the
// queries' lists afterwards.  A hit that finds the wave's area full is kept directly: its row bit goes into the panel's word of
// keep[], which the panel's wave — every panel has exactly one — writes for every panel of its range, so the masks need no
// clearing between batches.  Nor do the counts: every wave of the grid stores its own on leaving, a wave without panels a 0.
// SAMPLE (the level-1 sampling pass of a pre-filtered batch, in front of the main pass): the same loop, kept-test and records over ONE
// run of s_run consecutive panels per wave, run gw starting at panel gw * s_stride — s_stride >= s_run, so no (row, query) pair is
// evaluated twice — against the level-0 sampling threshold.  It writes no keep[] word, and a hit that finds the wave's area full is
// dropped: q8_select_kernel takes the k-th largest lb of whatever was recorded, and any k distinct real rows certify it.
template <int NQT, int CH, bool SAMPLE>
__global__ __launch_bounds__(CMR_SCAN_THREADS, 1) void q8_filter_kernel(FilterP P) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int KB = P.KB;
    v4u* qf = reinterpret_cast<v4u*>(smem);       // [part][tile][kb][64]
    for (int i = tid; i < 2 * NQT * KB * 64; i += CMR_SCAN_THREADS) qf[i] = P.qpack[i];
    __syncthreads();

    const int W = gridDim.x * CMR_SCAN_WAVES;
    const int gw = blockIdx.x * CMR_SCAN_WAVES + wave;
    int p0, p1;
    if (SAMPLE) {      // (a run that the corpus' end cuts is shorter; a wave beyond the runs, or whose run would start behind the end, has none)
        const long long s0 = (long long)gw * P.s_stride;
        p0 = (int)(s0 < P.npanels ? s0 : P.npanels);
        p1 = gw < P.s_nruns ? (P.npanels - p0 < P.s_run ? P.npanels : p0 + P.s_run) : p0;
    } else {
        p0 = (int)(((long long)gw * P.npanels) / W);
        p1 = (int)(((long long)(gw + 1) * P.npanels) / W);
    }
    if (p1 <= p0) {
        if (lane == 0) P.wcnt[gw] = 0u;
        return;
    }

    float aq[NQT], Bq[NQT], cq[NQT], tau[NQT];
    bool alive[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const int qi = t * 32 + (lane & 31);
        alive[t] = qi < P.nq;
        const float4 c = P.qconst[qi];
        aq[t] = c.x; Bq[t] = c.y; cq[t] = c.z;
        tau[t] = -__builtin_inff();
        if (alive[t] && P.tau_init && !P.keep_all) {
            const u64 key = P.tau_init[qi];
            if (key) tau[t] = cmr_key_score(key);
        }
    }

    i32x16 acc[2][NQT];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int t = 0; t < NQT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[h][t][r] = 0;

    // the panel's 32 (a, b) pairs as this lane's accumulator rows want them: rows 8 g + 4 (lane >> 5) + 0..3, g = 0..3 — loaded one
    // panel ahead, so that the epilogue never waits for them
    float4 sc[8];
    auto load_scales = [&](int p) {
        const float4* s = P.scales4 + (size_t)p * 16 + 2 * (lane >> 5);
#pragma unroll
        for (int g = 0; g < 4; ++g) { sc[2 * g] = s[4 * g]; sc[2 * g + 1] = s[4 * g + 1]; }
    };
    load_scales(p0);

    v4u* const wr = P.wrec + (size_t)gw * P.wave_cap;
    unsigned nrec = 0u;                     // records this wave has offered (wave-uniform)
    const int hrow = 4 * (lane >> 5);

    const int CPP = KB / CH;
    const long long nchunks = (long long)(p1 - p0) * CPP;
    const v4u* src = P.q8 + (size_t)p0 * KB * 64 + lane;
    int ci = 0, p = p0;
    v4u bufA[CH], bufB[CH];
    auto load = [&](v4u (&b)[CH]) {
#pragma unroll
        for (int u = 0; u < CH; ++u) b[u] = __builtin_nontemporal_load(&src[(size_t)u * 64]);
        src += (size_t)CH * 64;
        __builtin_amdgcn_sched_barrier(0);      // the loads are issued HERE, in front of the other buffer's MFMAs
    };
    auto step = [&](const v4u (&b)[CH]) {
        const v4u* qg = qf + (size_t)ci * CH * 64 + lane;
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const i32x4 a = __builtin_bit_cast(i32x4, b[u]);
#pragma unroll
            for (int t = 0; t < NQT; ++t) {
                acc[0][t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, __builtin_bit_cast(i32x4, qg[((size_t)t * KB + u) * 64]), acc[0][t], 0, 0, 0);
                acc[1][t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, __builtin_bit_cast(i32x4, qg[((size_t)(NQT + t) * KB + u) * 64]), acc[1][t], 0, 0, 0);
            }
        }
        if (++ci < CPP) return;
        ci = 0;
        // kept-test: bit r + 16 t of `hit`
        unsigned hit = 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float4 s4 = sc[2 * (r >> 2) + ((r & 3) >> 1)];
            const float ar = (r & 1) ? s4.z : s4.x, br = (r & 1) ? s4.w : s4.y;
#pragma unroll
            for (int t = 0; t < NQT; ++t) {
                const float ti = fmaf((float)acc[1][t][r], 1.0f / 254.0f, (float)acc[0][t][r]);
                const float ub = fmaf(ar * aq[t], ti, fmaf(Bq[t], br, cq[t]));
                if (alive[t] && !(ub < tau[t])) hit |= 1u << (r + 16 * t);
            }
        }
        const long long left = P.nrows - (long long)p * CMR_PANEL_ROWS;
        if (left < CMR_PANEL_ROWS) {            // the corpus' last panel: its padding rows are neither recorded nor kept
            const int lim = (int)(left > 0 ? left : 0) - hrow;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if ((r & 3) + 8 * (r >> 2) >= lim) hit &= ~(0x10001u << r);
        }
        unsigned rows = 0u;        // the rows of this panel that are kept without a record
        if (!SAMPLE && P.keep_all) rows = left < CMR_PANEL_ROWS ? (left > 0 ? (1u << left) - 1u : 0u) : ~0u;
        else if (__any(hit != 0u)) {
            const unsigned row0 = (unsigned)p * CMR_PANEL_ROWS + (unsigned)hrow;
            // (bits of the lane's accumulator rows WITHOUT the lane half's offset: row i = (r & 3) + 8 (r >> 2) + hrow, shifted once below)
            if (!SAMPLE && P.wave_cap == 0u) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (hit & (0x10001u << r)) rows |= 1u << ((r & 3) + 8 * (r >> 2));
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float4 s4 = sc[2 * (r >> 2) + ((r & 3) >> 1)];
                    const float ar = (r & 1) ? s4.z : s4.x, br = (r & 1) ? s4.w : s4.y;
#pragma unroll
                    for (int t = 0; t < NQT; ++t) {
                        const bool h = (hit & (1u << (r + 16 * t))) != 0u;
                        const u64 m = __ballot(h);
                        if (m == 0ull) continue;
                        const unsigned slot = nrec + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
                        nrec += (unsigned)__popcll(m);
                        if (!h) continue;
                        if (slot >= P.wave_cap) {
                            if (!SAMPLE) rows |= 1u << ((r & 3) + 8 * (r >> 2));
                            continue;
                        }
                        const float ti = fmaf((float)acc[1][t][r], 1.0f / 254.0f, (float)acc[0][t][r]);
                        const float e = fmaf(Bq[t], br, cq[t]);
                        const float ub = fmaf(ar * aq[t], ti, e), lb = fmaf(ar * aq[t], ti, -e);
                        wr[slot] = (v4u){row0 + (unsigned)((r & 3) + 8 * (r >> 2)), __float_as_uint(ub), __float_as_uint(lb),
                                         (unsigned)(t * 32 + (lane & 31))};
                    }
                }
            }
            if (!SAMPLE) {
                rows <<= hrow;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) rows |= (unsigned)__shfl_xor((int)rows, off);
            }
        }
        if (!SAMPLE && lane == 0) P.keep[p] = rows;
        ++p;
        load_scales(p < P.npanels ? p : P.npanels - 1);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int t = 0; t < NQT; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[h][t][r] = 0;
    };

    load(bufA);
    for (long long c = 0; c < nchunks; c += 2) {
        load(bufB);            // (the last one may read a chunk past the range: the companion carries the corpus' tail slack)
        step(bufA);
        if (c + 1 < nchunks) {
            load(bufA);
            step(bufB);
        }
    }
    if (lane == 0) P.wcnt[gw] = nrec;
}

// ------------------------------------------------------------------------------------------ bucket
struct BucketP {
    const v4u* wrec;
    const unsigned* wcnt;
    unsigned wave_cap;
    int W;
    v4u* pair;                 // [nq slots][pcap] records (row, ub, lb, 0)
    unsigned* pair_cnt;        // [nq slots] pairs offered per query (zeroed before the filter; may run past pcap)
    unsigned pcap;
    unsigned* keep;            // nullptr: a record beyond pcap is dropped
};

#define Q8_BUCKET_WAVES 4
// The filter's records, wave area by wave area, into the queries' lists: one wave per area, min(wcnt, wave_cap) records each.  A
// workgroup first counts its records per query in LDS, then takes ONE range per query from pair_cnt[] (the queries' counters share
// two cache lines: a global atomic per record — a quarter of a million a batch — would queue up on them) and hands the range's
// slots out from LDS again.  A slot at or beyond pcap: the list is full, the row is kept directly — its bit is OR-ed into keep[] as
// q8_tighten_kernel does it.  Which record gets which slot is arbitrary, as it was when the filter took the slots itself; the
// tightening is valid for any subset.  No wait on another workgroup; every loop runs to a count read once.
__global__ __launch_bounds__(Q8_BUCKET_WAVES * 64) void q8_bucket_kernel(BucketP P) {
    __shared__ unsigned s_cnt[64], s_base[64];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = blockIdx.x * Q8_BUCKET_WAVES + (tid >> 6);
    if (tid < 64) s_cnt[tid] = 0u;
    __syncthreads();
    unsigned c = 0u;
    if (w < P.W) { const unsigned offered = P.wcnt[w]; c = offered < P.wave_cap ? offered : P.wave_cap; }
    const v4u* rec = P.wrec + (size_t)(w < P.W ? w : 0) * P.wave_cap;
    for (unsigned i = lane; i < c; i += 64u) atomicAdd(&s_cnt[rec[i].w & 63u], 1u);
    __syncthreads();
    if (tid < 64) {
        const unsigned n = s_cnt[tid];
        s_base[tid] = n ? atomicAdd(&P.pair_cnt[tid], n) : 0u;
        s_cnt[tid] = 0u;
    }
    __syncthreads();
    for (unsigned i = lane; i < c; i += 64u) {
        const v4u v = rec[i];
        const unsigned q = v.w & 63u;
        const unsigned slot = s_base[q] + atomicAdd(&s_cnt[q], 1u);
        if (slot < P.pcap) P.pair[(size_t)q * P.pcap + slot] = (v4u){v.x, v.y, v.z, 0u};
        else if (P.keep) atomicOr(&P.keep[v.x >> 5], 1u << (v.x & 31u));      // (no keep[]: the sample's records — one beyond the list is dropped)
    }
}

// ------------------------------------------------------------------------------------------ tighten
struct TightenP {
    const v4u* pair;
    const unsigned* pair_cnt;
    unsigned pcap;
    const u64* tau_init;       // the sampling thresholds the filter tested against, or nullptr
    int k;
    unsigned* keep;
    float* tau_out;            // [nq] the threshold each query ended with (diagnostics)
    u64* key_out;              // select form: [nq] the threshold key the main pass takes as its tau_init
};

// the order-preserving 32-bit image of a non-NaN float, and back
__device__ __forceinline__ unsigned q8_f2ord(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float q8_ord2f(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u); }

// One workgroup per query.  The c = min(pair_cnt, pcap) stored pairs belong to c distinct real rows, and every one of them scores
// at least its lb in the 16-bit scan; so with c >= k the k-th largest (non-NaN) lb is a score that k rows reach, and a row whose ub
// is STRICTLY below it is beaten by k others whatever the tie-breaking (a subset of the query's pairs — an overflowed list — only
// gives a smaller k-th largest, which is as valid).  Radix select, four passes of 8 bits over the image of lb with a 256-bin
// histogram in LDS; then every stored pair that still stands sets its row's bit in keep[] (the OR also folds the queries that hit one
// row into one candidate).  Every loop runs to a count read once.
// SELECT (behind the int8 sample, in front of the main pass): the same selection over the sample's records and nothing else — no loop over
// the pairs, no keep[].  The k-th largest lb, tau_s, is written as a threshold KEY: the smallest key with score tau_s, minus 1
// (cmr_launch_fill_threshold's construction), so that key > tau <=> score >= tau_s and a row tied with tau_s stays; the key written is
// the larger of that and the level-0 key in tau_init[q], and the level-0 key alone with fewer than k usable records.
template <bool SELECT>
__device__ __forceinline__ void q8_tighten_body(const TightenP& P) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_bin, s_need;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const unsigned offered = P.pair_cnt[q];
    const unsigned c = offered < P.pcap ? offered : P.pcap;
    const v4u* pr = P.pair + (size_t)q * P.pcap;
    float tau = -__builtin_inff();
    if (P.tau_init) {
        const u64 key = P.tau_init[q];
        if (key) tau = cmr_key_score(key);
    }
    if (c >= (unsigned)P.k) {
        unsigned prefix = 0u, mask = 0u, need = (unsigned)P.k;
        bool found = true;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0u;
            __syncthreads();
            for (unsigned i = tid; i < c; i += 256u) {
                const float lb = __uint_as_float(pr[i].z);
                if (lb == lb) {
                    const unsigned u = q8_f2ord(lb);
                    if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
                }
            }
            __syncthreads();
            if (tid < 64) {      // bins in descending order, four per lane: the bin in which the running count reaches `need`
                unsigned h[4], sum = 0u;
#pragma unroll
                for (int j = 0; j < 4; ++j) { h[j] = hist[255 - (4 * lane + j)]; sum += h[j]; }
                unsigned incl = sum;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) { const unsigned o = (unsigned)__shfl_up((int)incl, off); if (lane >= off) incl += o; }
                const u64 reach = __ballot(incl >= need);
                if (reach == 0ull) { if (lane == 0) s_bin = 0xFFFFFFFFu; }      // fewer than k lower bounds that are numbers
                else if (lane == __ffsll((long long)reach) - 1) {
                    unsigned before = incl - sum;
                    int j = 0;
#pragma unroll
                    for (int t = 0; t < 3; ++t) if (j == t && before + h[t] < need) { before += h[t]; j = t + 1; }
                    s_bin = 255u - (unsigned)(4 * lane + j);
                    s_need = need - before;
                }
            }
            __syncthreads();
            const unsigned bin = s_bin;
            if (bin == 0xFFFFFFFFu) { found = false; break; }
            need = s_need;
            prefix |= bin << shift;
            mask |= 255u << shift;
        }
        if (SELECT) {
            if (tid == 0) {
                u64 key = P.tau_init ? P.tau_init[q] : 0ull;
                if (found) {
                    const u64 ks = cmr_make_key(q8_ord2f(prefix), 0xFFFFFFFFu) - 1ull;
                    key = ks > key ? ks : key;
                }
                P.key_out[q] = key;
            }
            return;
        }
        if (found) tau = fmaxf(tau, q8_ord2f(prefix));
    }
    if (SELECT) {
        if (tid == 0) P.key_out[q] = P.tau_init ? P.tau_init[q] : 0ull;
        return;
    }
    for (unsigned i = tid; i < c; i += 256u) {
        const v4u v = pr[i];
        if (!(__uint_as_float(v.y) < tau)) atomicOr(&P.keep[v.x >> 5], 1u << (v.x & 31u));
    }
    if (tid == 0) P.tau_out[q] = tau;
}
__global__ __launch_bounds__(256) void q8_tighten_kernel(TightenP P) { q8_tighten_body<false>(P); }
__global__ __launch_bounds__(256) void q8_select_kernel(TightenP P) { q8_tighten_body<true>(P); }

// ------------------------------------------------------------------------------------------ expand
// keep[0 .. npanels) -> the rows of the set bits in cand_row[], counted in *n_cand (zeroed in front of the launch) with one
// atomicAdd per wave that has any
__global__ __launch_bounds__(256) void q8_expand_kernel(const unsigned* __restrict__ keep, int npanels, unsigned* __restrict__ cand_row, unsigned* n_cand) {
    const int lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned m = p < npanels ? keep[p] : 0u;
    const int c = __popc(m);
    int incl = c;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off); if (lane >= off) incl += o; }
    const int total = __builtin_amdgcn_readlane(incl, 63);
    if (total == 0) return;
    unsigned base = 0u;
    if (lane == 0) base = atomicAdd(n_cand, (unsigned)total);
    base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
    unsigned at = base + (unsigned)(incl - c);
    const unsigned row0 = (unsigned)p * CMR_PANEL_ROWS;
    for (unsigned b = m; b; b &= b - 1u) cand_row[at++] = row0 + (unsigned)(__ffs((int)b) - 1);
}

// ------------------------------------------------------------------------------------------ re-score
// the scan's topk_push for a tile whose 32 rows are 32 CANDIDATES: row i of the tile is the row lane i holds in `myrow`
// (0xFFFFFFFF: no candidate — pushes nothing)
template <int CAP>
__device__ __forceinline__ u64 rescore_push(const f32x16& acc, unsigned myrow, long long nrows, u64 tau_key, int* cnt_t, u64* list_t, int lane) {
    const int ql = lane & 31;
    const int hrow = 4 * (lane >> 5);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float v = acc[r];
        const unsigned row = (unsigned)__shfl((int)myrow, (r & 3) + 8 * (r >> 2) + hrow);
        const u64 key = cmr_make_key(v, row);
        if ((long long)row < nrows && v == v && key > tau_key) {
            const int slot = atomicAdd(&cnt_t[ql], 1);
            list_t[(size_t)ql * CAP + slot] = key;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int c = __hip_atomic_load(&cnt_t[ql], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __ballot(c > CAP - 32) & 0xFFFFFFFFull;
}

struct RescoreP {
    const v4u* corpus;
    const v4u* qfrag;          // the 16-bit query fragments of prep_queries_kernel: [tile][ks][64]
    const unsigned* cand_row;
    const unsigned* n_cand;
    const u64* tau_init;
    long long nrows;
    int KS, nq, k;
    u64* lists;                // [W'][NQT * 32][CAP]
    int* cnt;                  // [W'][NQT * 32]
};

#define Q8_RESCORE_WAVES 4
// A fixed grid; wave w takes the groups of 32 candidates w, w + W', ...  Lane l gathers the 16-byte pieces of row
// cand_row[32 p + (l & 31)] straight from the 16-bit panels — its slot (row & 31) + 32 (l >> 5) of every block of the row's panel —
// which IS the A-operand of a panel made of the 32 candidates, and runs the scan's chain on it: zero accumulator, then
// CmrBlk<DT>::mma(corpus block, query block, acc) for ks = 0 .. KS - 1 ascending, one chain per query tile.  An element of the MFMA
// result depends on its own row and column only, so every score has the bits scan_kernel computes for that (row, query).
template <int DT, int NQT, int CAP>
__global__ __launch_bounds__(Q8_RESCORE_WAVES * 64) void q8_rescore_kernel(RescoreP P) {
    constexpr int NQ = NQT * 32;
    __shared__ int cnt_all[Q8_RESCORE_WAVES * NQ];
    __shared__ u64 stage_all[Q8_RESCORE_WAVES * (CAP + 2)];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < Q8_RESCORE_WAVES * NQ; i += Q8_RESCORE_WAVES * 64) cnt_all[i] = 0;
    __syncthreads();
    int* cnt_w = cnt_all + wave * NQ;
    u64* stage = stage_all + wave * (CAP + 2);
    const int Wn = gridDim.x * Q8_RESCORE_WAVES;
    const int gw = blockIdx.x * Q8_RESCORE_WAVES + wave;
    u64* list_w = P.lists + (size_t)gw * NQ * CAP;
    const int KS = P.KS;

    float tau_f[NQT];
    u64 tau_key[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const int q = t * 32 + (lane & 31);
        tau_key[t] = 0ull;
        tau_f[t] = -__builtin_inff();
        if (q >= P.nq) { tau_key[t] = ~0ull; tau_f[t] = __builtin_inff(); }
        else if (P.tau_init) {
            tau_key[t] = P.tau_init[q];
            if (tau_key[t]) tau_f[t] = cmr_key_score(tau_key[t]);
        }
    }
    const unsigned n_cand = *P.n_cand;
    const unsigned ngroups = (n_cand + 31u) / 32u;
    for (unsigned g = (unsigned)gw; g < ngroups; g += (unsigned)Wn) {
        const unsigned ci = g * 32u + (unsigned)(lane & 31);
        const unsigned myrow = ci < n_cand ? P.cand_row[ci] : 0xFFFFFFFFu;
        const unsigned lrow = ((long long)myrow < P.nrows) ? myrow : 0u;
        const v4u* src = P.corpus + (size_t)(lrow >> 5) * KS * 64 + (lrow & 31u) + 32u * (unsigned)(lane >> 5);
        const v4u* qg = P.qfrag + lane;
        f32x16 acc[NQT];
#pragma unroll
        for (int t = 0; t < NQT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
        for (int ks0 = 0; ks0 < KS; ks0 += 8) {
            v4u a[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) a[u] = src[(size_t)(ks0 + u) * 64];
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int t = 0; t < NQT; ++t) acc[t] = CmrBlk<DT>::mma(a[u], qg[((size_t)t * KS + ks0 + u) * 64], acc[t]);
        }
#pragma unroll
        for (int t = 0; t < NQT; ++t) {
            float mx = acc[t][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) mx = fmaxf(mx, acc[t][r]);
            if (__any(mx >= tau_f[t])) {
                const u64 need = rescore_push<CAP>(acc[t], myrow, P.nrows, tau_key[t], cnt_w + t * 32, list_w + (size_t)t * 32 * CAP, lane);
                if (need) topk_compact<CAP>(need, P.k, tau_key[t], tau_f[t], cnt_w + t * 32, list_w + (size_t)t * 32 * CAP, stage, lane);
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    for (int q = lane; q < NQ; q += 64) P.cnt[(size_t)gw * NQ + q] = __hip_atomic_load(&cnt_w[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

}  // namespace

// ------------------------------------------------------------------------------------------ host
hipError_t cmr_launch_q8_quantise(int dtype, const void* corpus, int dpad, long long panel0, long long npanels, long long nrows, void* q8,
                                  float2* scales, float* stats, hipStream_t s) {
    if (npanels <= 0) return hipSuccess;
    const dim3 grid((unsigned)((npanels + 3) / 4)), block(256);
    const v4u* c = reinterpret_cast<const v4u*>(corpus);
    v4u* o = reinterpret_cast<v4u*>(q8);
    switch (dtype) {
        case CMR_DT_BF16: hipLaunchKernelGGL(q8_quantise_kernel<CMR_DT_BF16>, grid, block, 0, s, c, dpad / 16, panel0, npanels, nrows, o, scales, stats); break;
        case CMR_DT_F16:  hipLaunchKernelGGL(q8_quantise_kernel<CMR_DT_F16>, grid, block, 0, s, c, dpad / 16, panel0, npanels, nrows, o, scales, stats); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t cmr_launch_q8_pack_queries(int dtype, const float* q, int nq, int dim, int dpad, int tiles, const float* stats, void* qpack,
                                      float4* qconst, hipStream_t s) {
    const dim3 grid(tiles * 32), block(256);
    signed char* o = reinterpret_cast<signed char*>(qpack);
    switch (dtype) {
        case CMR_DT_BF16: hipLaunchKernelGGL(q8_pack_queries_kernel<CMR_DT_BF16>, grid, block, 0, s, q, nq, dim, dpad, tiles, stats, o, qconst); break;
        case CMR_DT_F16:  hipLaunchKernelGGL(q8_pack_queries_kernel<CMR_DT_F16>, grid, block, 0, s, q, nq, dim, dpad, tiles, stats, o, qconst); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

size_t cmr_q8_filter_lds(int dpad, int nqt) { return (size_t)2 * nqt * (dpad / 32) * 1024; }

// sample = true: the level-1 sampling pass (the a.s_* fields: grid, runs, record areas, the level-0 keys as thresholds)
hipError_t cmr_launch_q8_filter(const CmrQ8Args& a, hipStream_t s, bool sample) {
    FilterP p;
    p.q8 = reinterpret_cast<const v4u*>(a.q8); p.scales4 = reinterpret_cast<const float4*>(a.scales);
    p.qpack = reinterpret_cast<const v4u*>(a.qpack); p.qconst = a.qconst; p.tau_init = sample ? a.s_tau0 : a.tau_init;
    p.nrows = a.nrows; p.npanels = a.npanels; p.KB = a.dpad / 32; p.nq = a.nq; p.keep_all = sample ? 0 : a.keep_all;
    p.wrec = reinterpret_cast<v4u*>(sample ? a.s_wrec : a.wrec); p.wcnt = sample ? a.s_wcnt : a.wcnt;
    p.wave_cap = (unsigned)(sample ? a.s_wave_cap : a.wave_cap); p.keep = sample ? nullptr : a.keep;
    p.s_run = a.s_run; p.s_stride = a.s_stride; p.s_nruns = a.s_nruns;
    if (sample && (a.s_run < 1 || a.s_stride < a.s_run || a.s_nruns > a.s_grid * CMR_SCAN_WAVES || a.s_wave_cap < 1 || a.s_grid < 1)) return hipErrorInvalidValue;
    const int grid = sample ? a.s_grid : a.grid;
    const size_t lds = cmr_q8_filter_lds(a.dpad, a.nqt);
    auto launch = [&](auto kern) -> hipError_t {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(CMR_SCAN_THREADS), lds, s, p);
        return hipGetLastError();
    };
    const bool ch8 = p.KB % 8 == 0;
    if (sample) {
        if (a.nqt == 2) return ch8 ? launch(q8_filter_kernel<2, 8, true>) : launch(q8_filter_kernel<2, 4, true>);
        if (a.nqt == 1) return ch8 ? launch(q8_filter_kernel<1, 8, true>) : launch(q8_filter_kernel<1, 4, true>);
        return hipErrorInvalidValue;
    }
    if (a.nqt == 2) return ch8 ? launch(q8_filter_kernel<2, 8, false>) : launch(q8_filter_kernel<2, 4, false>);
    if (a.nqt == 1) return ch8 ? launch(q8_filter_kernel<1, 8, false>) : launch(q8_filter_kernel<1, 4, false>);
    return hipErrorInvalidValue;
}

// sample = true: the sample's wave areas into the sample's lists, nothing kept directly
hipError_t cmr_launch_q8_bucket(const CmrQ8Args& a, hipStream_t s, bool sample) {
    BucketP p;
    if (sample) {
        p.wrec = reinterpret_cast<const v4u*>(a.s_wrec); p.wcnt = a.s_wcnt; p.wave_cap = (unsigned)a.s_wave_cap; p.W = a.s_grid * CMR_SCAN_WAVES;
        p.pair = reinterpret_cast<v4u*>(a.s_pair); p.pair_cnt = a.s_pair_cnt; p.pcap = (unsigned)a.s_pcap; p.keep = nullptr;
    } else {
        p.wrec = reinterpret_cast<const v4u*>(a.wrec); p.wcnt = a.wcnt; p.wave_cap = (unsigned)a.wave_cap; p.W = a.grid * CMR_SCAN_WAVES;
        p.pair = reinterpret_cast<v4u*>(a.pair); p.pair_cnt = a.pair_cnt; p.pcap = (unsigned)a.pcap; p.keep = a.keep;
    }
    hipLaunchKernelGGL(q8_bucket_kernel, dim3((p.W + Q8_BUCKET_WAVES - 1) / Q8_BUCKET_WAVES), dim3(Q8_BUCKET_WAVES * 64), 0, s, p);
    return hipGetLastError();
}

hipError_t cmr_launch_q8_tighten(const CmrQ8Args& a, hipStream_t s) {
    TightenP p;
    p.pair = reinterpret_cast<const v4u*>(a.pair); p.pair_cnt = a.pair_cnt; p.pcap = (unsigned)a.pcap; p.tau_init = a.tau_init; p.k = a.k;
    p.keep = a.keep; p.tau_out = a.tau_tight; p.key_out = nullptr;
    hipLaunchKernelGGL(q8_tighten_kernel, dim3(a.nq), dim3(256), 0, s, p);
    return hipGetLastError();
}

// the sample's lists -> per query max(key of the k-th largest lb, level-0 key a.s_tau0[q]) in a.s_tau_out[q]
hipError_t cmr_launch_q8_select(const CmrQ8Args& a, hipStream_t s) {
    TightenP p;
    p.pair = reinterpret_cast<const v4u*>(a.s_pair); p.pair_cnt = a.s_pair_cnt; p.pcap = (unsigned)a.s_pcap; p.tau_init = a.s_tau0; p.k = a.k;
    p.keep = nullptr; p.tau_out = nullptr; p.key_out = a.s_tau_out;
    hipLaunchKernelGGL(q8_select_kernel, dim3(a.nq), dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t cmr_launch_q8_expand(const CmrQ8Args& a, hipStream_t s) {
    hipLaunchKernelGGL(q8_expand_kernel, dim3((a.npanels + 255) / 256), dim3(256), 0, s, (const unsigned*)a.keep, a.npanels, a.cand_row, a.n_cand);
    return hipGetLastError();
}

hipError_t cmr_launch_q8_rescore(const CmrQ8Args& a, hipStream_t s) {
    RescoreP p;
    p.corpus = reinterpret_cast<const v4u*>(a.corpus); p.qfrag = reinterpret_cast<const v4u*>(a.qfrag);
    p.cand_row = a.cand_row; p.n_cand = a.n_cand; p.tau_init = a.tau_init; p.nrows = a.nrows; p.KS = a.dpad / 16; p.nq = a.nq; p.k = a.k;
    p.lists = a.lists; p.cnt = a.cnt;
    auto launch = [&](auto kern) -> hipError_t {
        hipLaunchKernelGGL(kern, dim3(a.rescore_grid), dim3(Q8_RESCORE_WAVES * 64), 0, s, p);
        return hipGetLastError();
    };
#define RCASE(DT, NQT, CAP) if (a.dtype == DT && a.nqt == NQT && a.cap == CAP) return launch(q8_rescore_kernel<DT, NQT, CAP>);
    RCASE(CMR_DT_BF16, 1, 128) RCASE(CMR_DT_BF16, 1, 256) RCASE(CMR_DT_BF16, 2, 128) RCASE(CMR_DT_BF16, 2, 256)
    RCASE(CMR_DT_F16, 1, 128) RCASE(CMR_DT_F16, 1, 256) RCASE(CMR_DT_F16, 2, 128) RCASE(CMR_DT_F16, 2, 256)
#undef RCASE
    return hipErrorInvalidValue;
}
int cmr_q8_rescore_waves(void) { return Q8_RESCORE_WAVES; }
