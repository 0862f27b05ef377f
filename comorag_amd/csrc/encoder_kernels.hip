// Encoder-side gfx950 kernels of libcomorag_hip.so: the two memory-/latency-shaped pieces of a BERT layer that are not GEMMs.
//
//   attn_fwd_kernel   softmax(Q K^T / sqrt(HD)) V of one (sequence, head, 128-query block) per workgroup, heads HD = 64 or 32 wide, 16-bit in / out,
//                     fp32 scores and accumulators, keys beyond the sequence's length masked (right-padded mini-batches).
//                     Replaces the scaled-dot-product-attention call inside transformers' BertSelfAttention, i.e. part of
//                     `self.embedding_model(**inputs)` at embedding_model/BGEEmbedding.py:119.
//   attn_fwd_f32_kernel   the same for fp32 tensors, fp32 end to end, both products on the exact f32-input MFMA (comment at the kernel).
//   add_ln_kernel     LayerNorm(y + bias + residual) * gamma + beta, one wave per token: BertSelfOutput / BertOutput minus
//                     their GEMM (dense bias add, residual add and LayerNorm are three kernels and five passes over the
//                     activations in PyTorch; here one read of y and the residual, one write).
//   embed_ln_kernel   BertEmbeddings: the word / position / token-type gathers, their sum and the LayerNorm in one pass.
// The LayerNorm and embedding kernels are templates over the element type: bf16, fp16 and — written unrounded, 16-byte lane vectors of
// four floats — fp32 (EncVec below).
//
// Attention layout.  Q, K, V are column slices of ONE packed projection output qkv[b*L, 3*hidden] (the host side multiplies by
// the concatenated query/key/value weights once): head h reads columns h*HD (Q), hidden + h*HD (K), 2*hidden + h*HD (V); below for HD = 64.
// A wave owns 32 query rows.  Scores are computed TRANSPOSED, S^T = K Q^T (A operand = a 32-key tile read from LDS, B operand
// = the wave's Q rows, loaded once from global memory in MFMA lane order), so that in the 32x32 accumulator layout
// (cmr_acc_row) lane l holds column q = l & 31: every softmax statistic of a query row is lane-local except one cross-half
// max.  The same registers, converted to 16 bits, ARE the B operand of O^T = V^T P^T: k-slot e of lane half g is key
// acc_row(8*s + e, g) — a permutation of the 16 keys of a k-step, applied identically to the A operand by reading V^T from
// LDS at [d][16*s + 4*g + {0..3}] and [d][16*s + 8 + 4*g + {0..3}].  V is transposed on its way into LDS (two keys per thread,
// eight packed 4-byte writes); K goes in row-major.  Both are double-buffered 64-key chunks: the global loads of chunk c + 1
// are in flight while chunk c is multiplied, one barrier per chunk.  35 KiB of LDS per workgroup: several workgroups share a
// CU, so one's exponentials overlap another's MFMAs (the 64-wide head makes the softmax, not the matrix pipe, the longer leg).
#include "cmr_device.h"
#include "cmr_internal.h"
#include "cmr_kernels.h"

typedef __attribute__((ext_vector_type(2))) __bf16 enc_bf16x2;
typedef __attribute__((ext_vector_type(2))) _Float16 enc_f16x2;

template <int DT> __device__ __forceinline__ unsigned enc_pack2(float a, float b) {   // round-to-nearest-even, a in the low half
    if constexpr (DT == CMR_DT_BF16) {
        enc_bf16x2 t;
        t[0] = (__bf16)a;
        t[1] = (__bf16)b;
        return __builtin_bit_cast(unsigned, t);
    } else {
        enc_f16x2 t;
        t[0] = (_Float16)a;
        t[1] = (_Float16)b;
        return __builtin_bit_cast(unsigned, t);
    }
}
template <int DT> __device__ __forceinline__ void enc_unpack2(unsigned u, float& a, float& b) {
    if constexpr (DT == CMR_DT_BF16) {
        a = __uint_as_float(u << 16);
        b = __uint_as_float(u & 0xFFFF0000u);
    } else {
        enc_f16x2 t = __builtin_bit_cast(enc_f16x2, u);
        a = (float)t[0];
        b = (float)t[1];
    }
}

// One lane-vector of four / eight elements of a row: 8 / 16 bytes of a 16-bit tensor; four floats (16 bytes) / two such vectors of an
// fp32 one.  enc_get* widen to fp32 (exact), enc_put* round once (16-bit) or store the floats as they are (fp32).
struct enc_f32x8 { float4 lo, hi; };
template <int DT> struct EncVec { typedef uint2 V4; typedef uint4 V8; };
template <> struct EncVec<CMR_DT_F32> { typedef float4 V4; typedef enc_f32x8 V8; };
template <int DT> __device__ __forceinline__ void enc_get4(float (&t)[4], typename EncVec<DT>::V4 a) {
    if constexpr (DT == CMR_DT_F32) {
        t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
    } else {
        enc_unpack2<DT>(a.x, t[0], t[1]);
        enc_unpack2<DT>(a.y, t[2], t[3]);
    }
}
template <int DT> __device__ __forceinline__ void enc_get8(float (&t)[8], typename EncVec<DT>::V8 a) {
    if constexpr (DT == CMR_DT_F32) {
        t[0] = a.lo.x; t[1] = a.lo.y; t[2] = a.lo.z; t[3] = a.lo.w;
        t[4] = a.hi.x; t[5] = a.hi.y; t[6] = a.hi.z; t[7] = a.hi.w;
    } else {
        enc_unpack2<DT>(a.x, t[0], t[1]);
        enc_unpack2<DT>(a.y, t[2], t[3]);
        enc_unpack2<DT>(a.z, t[4], t[5]);
        enc_unpack2<DT>(a.w, t[6], t[7]);
    }
}
template <int DT> __device__ __forceinline__ typename EncVec<DT>::V4 enc_put4(float a, float b, float c, float d) {
    if constexpr (DT == CMR_DT_F32) {
        return make_float4(a, b, c, d);
    } else {
        uint2 w;
        w.x = enc_pack2<DT>(a, b);
        w.y = enc_pack2<DT>(c, d);
        return w;
    }
}
template <int DT> __device__ __forceinline__ typename EncVec<DT>::V8 enc_put8(const float (&t)[8]) {
    if constexpr (DT == CMR_DT_F32) {
        enc_f32x8 w;
        w.lo = make_float4(t[0], t[1], t[2], t[3]);
        w.hi = make_float4(t[4], t[5], t[6], t[7]);
        return w;
    } else {
        uint4 w;
        w.x = enc_pack2<DT>(t[0], t[1]);
        w.y = enc_pack2<DT>(t[2], t[3]);
        w.z = enc_pack2<DT>(t[4], t[5]);
        w.w = enc_pack2<DT>(t[6], t[7]);
        return w;
    }
}

// ------------------------------------------------------------------------------------------------ attention
#define ATT_CHUNK 64          // keys per LDS chunk
#define ATT_QBLOCK 128        // query rows per workgroup of the 4-wave kernel (4 waves x 32); the 8-wave kernel takes 256
#define ATT_KSTR 72           // K rows in LDS: 64 elements + 8 of padding (144 B: ds_read_b128 of 16 consecutive rows hit 16 different 16-B slots)
#ifndef ATT_VTR
#define ATT_VTR 1             // 1: V goes into LDS ROW-MAJOR (two 16-byte writes per thread, as K) and the PV step reads its A operands with
#endif                        //    ds_read_b64_tr_b16 (gfx950's transposing LDS read); 0: V transposed on its way in (eight 4-byte writes per thread)
#if ATT_VTR && defined(ATT_VSTR_OVERRIDE)
#define ATT_VSTR ATT_VSTR_OVERRIDE
#elif ATT_VTR
#define ATT_VSTR 88           // V rows in LDS: 64 d + 24 of padding (176 B).  Measured, us per layer at 32 x 512 x 12 heads bf16 / 16 heads fp16 (gpurun_out/r5x):
                              // 72: 46.8 / 59.7   80: 48.3 / 61.8   88: 46.2 / 59.6   96: 47.4 / 60.9   104: 48.7 / 63.7   112: 49.0 / 62.1   136: 48.5 / 62.3
#else
#define ATT_VSTR 68           // V^T rows in LDS: 64 keys + 4 (136 B: ds_read_b64 of 32 consecutive d rows hit 32 different bank pairs)
#endif
// Round 6, measured with the kernel's own duration (rocprofv3 --kernel-trace, tools/attn_variants.sh; 32 x 512 x 12 heads bf16, full and ragged
// mini-batches averaged, two runs on one box): round 5's kernel 41.6 / 40.9 us; + packed softmax arithmetic (ATT_PK) 39.5 / 40.3 — kept;
// + unpadded XOR-swizzled K / V rows written through registers (ATT_SWZL: SQ_LDS_BANK_CONFLICT 37 K -> 0, LDS-array cycles -41 %) 41.1 / 41.4;
// + the chunks by LDS-DMA instead of registers (ATT_DMA: VGPRs 120 -> 112, no ds_write) 42.0 / 41.6.  Neither the bank conflicts nor the
// register staging is what bounds this kernel: the swizzle's address arithmetic costs a VALU-bound loop more than the conflicts did.
#ifndef ATT_PK
#define ATT_PK 1              // 1: the softmax's multiply-adds and sums two scores per instruction (v_pk_fma_f32 / v_pk_add_f32)
#endif
#ifndef ATT_DMA
#define ATT_DMA 0             // 1 (needs ATT_VTR): K / V chunks go HBM / L2 -> LDS by LDS-DMA (global_load_lds_dwordx4: no staging registers, no ds_write),
#endif                        //    rows unpadded (128 B) and XOR-swizzled by 16-byte segment so that both read patterns stay conflict-free; 0: through registers
#ifndef ATT_SWZL
#define ATT_SWZL 0            // 1 (needs ATT_VTR): K / V rows in LDS unpadded and XOR-swizzled by 16-byte segment (ATT_SWZ below) — no bank conflict on either read;
#endif                        //    0: padded rows (ATT_KSTR / ATT_VSTR).  ATT_DMA implies it (a DMA instruction lands 1 KiB lane-linear: no padding possible)
#if ATT_DMA && !ATT_SWZL
#undef ATT_SWZL
#define ATT_SWZL 1
#endif
#if ATT_SWZL && !ATT_VTR
#error "the swizzled layout stages V row-major: it needs ATT_VTR"
#endif
typedef short att_v4s __attribute__((ext_vector_type(4)));
#define ATT_NEG (-1.0e30f)
#ifndef ATT_MIN_WG
#define ATT_MIN_WG 2          // workgroups per CU the register budget is held to (__launch_bounds__)
#endif
#ifndef ATT_ABL
#define ATT_ABL 0             // development ablations (wrong results): 1 no v_exp, 2 no QK^T MFMAs, 3 no PV MFMAs, 4 no K / V staging after chunk 0 and no barrier, 5 no barrier, 6 no V^T stores, 7 no K / V global loads
#endif
#ifndef ATT_SKIP_RESCALE
#define ATT_SKIP_RESCALE 0    // 1: a chunk that raises no query's running maximum (wave-uniform test) skips the 32 accumulator multiplies by 1.0 (measured SLOWER: 54 vs 50 us)
#endif

// NW = waves per workgroup.  4: 128 query rows share a staged K / V chunk.  8: 256 rows do — the chunk's staging (global -> registers
// -> LDS, one barrier) is the longest leg of this kernel (26 % at 4 waves: DESIGN 4.10) and costs the same per chunk however many
// query rows consume it; every thread then stages ONE 16-byte segment of K and of V instead of two.  Used for sequences of >= 256
// (padded) tokens; shorter mini-batches keep 4 waves (half of an 8-wave workgroup would hold padding rows only).
//
// HD = head width, 64 or 32 (bge-small / MiniLM / e5-small: 384 hidden, 12 heads).  Same algorithm and data flow; with HD = 32 the wave's Q rows
// are TWO k-steps (qf[2]), a score tile costs 2 MFMAs, and PV has ONE 32-column output tile (o[1]): 8 MFMAs per tile pair and chunk
// instead of 16, 16 accumulator registers instead of 32.  A K / V row is 64 B — four 16-byte segments — so a 64-key chunk is 256 segments
// of K and of V: one staging pass of 4 waves (thread -> row tid >> 2, segment tid & 3).  HD = 32 runs on 4 waves for every l: an 8-wave
// workgroup would leave half its threads without a segment to stage, and the staging it amortises is half the 64-wide kernel's already.
#define ATT_KSTR32 40         // HD = 32, K rows in LDS: 32 elements + 8 of padding (80 B = 5 slots of 16 B, odd: ds_read_b128 of 16 consecutive rows hit 16 different slots)
#ifndef ATT_VSTR32
#define ATT_VSTR32 32         // HD = 32, V rows in LDS: NO padding (64 B).  A 32-lane group of ds_read_b64_tr_b16 reads ALL 32 d of four consecutive keys:
#endif                        // with 64-byte rows that is 256 contiguous bytes = the 64 banks once each; ds_write_b128 of 8 lanes covers two whole rows (128 B, 32 banks).
                              // Any multiple of 8 elements >= 32 is correct (8-byte reads, 16-byte writes).  Measured, us per call at 32 x 512 x 12 heads, full sequences,
                              // bf16 / f16, medians of 9 regions x 40 calls, two processes each on one box: 32: 32.9, 31.9 / 31.4, 31.4   40: 32.5, 32.6 / 31.5, 32.1
                              // 48: 33.3, 33.3 / 31.7, 31.6 — inside the regions' own spread (bf16 min .. max 31.1 .. 38.6): the smallest footprint stays.
template <int DT, int NW, int HD>
__global__ __launch_bounds__(NW * 64, NW == 8 ? 4 : ATT_MIN_WG) void attn_fwd_kernel(const unsigned short* __restrict__ qkv, const int* __restrict__ lens, int L, int hidden,
                                                           int n_heads, int n_qblocks, int total, float sc /* log2(e) / sqrt(HD) */,
                                                           unsigned short* __restrict__ out) {
    static_assert(HD == 64 || HD == 32, "head width 64 or 32");
    static_assert(HD == 64 || (ATT_VTR && !ATT_SWZL && !ATT_DMA), "the development layouts (ATT_VTR = 0, ATT_SWZL, ATT_DMA) are written for 64-wide heads");
    static_assert(HD == 64 || NW == 4, "32-wide heads: a chunk is one staging pass of 4 waves");
    static_assert(ATT_VSTR32 >= 32 && ATT_VSTR32 % 8 == 0, "V rows of 32 elements, 16-byte aligned");
    constexpr int KSTR = HD == 64 ? ATT_KSTR : ATT_KSTR32, VSTR = HD == 64 ? ATT_VSTR : ATT_VSTR32;      // LDS row strides, elements
    constexpr int KS = HD / 16, DTN = HD / 32, SEGS = HD / 8;      // k-steps of QK^T; 32-column output tiles of PV; 16-byte segments of a K / V row
#if ATT_SWZL
    // [key][64 d] unpadded (two rows per 256-byte bank row), 16-byte segment sg of row r at slot sg ^ f(r), f = ATT_SWZ: a DMA instruction lands
    // 8 rows x 128 B lane-linear (the lane picks the SOURCE segment that belongs in its slot).  f permutes the bits of u = (r >> 1) & 7 —
    // (u & 1) << 2 | u >> 1 — so that (MI355X_MICROARCH.md, LDS: 64 banks, lane groups per instruction)
    //   * ds_read_b128 of QK^T: a 16-lane group {0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} reads one segment of 16 rows; its eight even rows
    //     have eight different u, its eight odd rows (the other half of the bank row) too: 16 different slots;
    //   * ds_read_b64_tr_b16 of PV: a 32-lane group reads four segments of four consecutive rows; rows r and r + 2 share a half of the bank
    //     row and differ in bit 2 of f: their segment sets {4 dt .. 4 dt + 3} ^ f are disjoint.
    // (first version: f = r & 7 — SQ_LDS_BANK_CONFLICT twice the padded layout's, rows r and r + 2 of a transposing read on the same slots)
#define ATT_SWZ(r) (((((r) >> 1) & 1) << 2) | ((((r) >> 1) & 7) >> 1))
    __shared__ __attribute__((aligned(1024))) unsigned short k_lds[2][ATT_CHUNK * 64];
    __shared__ __attribute__((aligned(1024))) unsigned short v_lds[2][ATT_CHUNK * 64];
#else
    __shared__ __attribute__((aligned(16))) unsigned short k_lds[2][ATT_CHUNK * KSTR];
    __shared__ __attribute__((aligned(16))) unsigned short v_lds[2][64 * VSTR];      // ATT_VTR: [key][d], else [d][key]
#endif
    // workgroup id -> work item.  Hardware deals workgroup ids round-robin over the 8 XCDs: the query blocks of one (sequence, head)
    // pair stay on ONE XCD, so the pair's K / V come out of that XCD's L2 after the first block; the PAIRS go round the XCDs, so every
    // XCD holds a share of every sequence.  (Round 4 kept a whole sequence — all its heads — on one XCD: in a mini-batch of mixed
    // lengths the XCD that drew the long sequences set the kernel's time — 32 sequences of 17 .. 512 tokens took as long as 32 of 512.)
    const int xcd = (int)(blockIdx.x & 7), j = (int)(blockIdx.x >> 3);
    const int pair = (j / n_qblocks) * 8 + xcd;
    if (pair >= total / n_qblocks) return;
    // (the host sorts a mini-batch's rows by ascending length: taking the sequences from the back starts the long ones first and
    //  leaves the short ones to fill the tail)
    const int qb = j % n_qblocks, head = pair % n_heads, seq = total / (n_qblocks * n_heads) - 1 - pair / n_heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5, c = lane & 31;
    constexpr int QBLOCK = NW * 32, PROWS = NW * 64 / SEGS, PASSES = ATT_CHUNK / PROWS;      // rows per workgroup; staging passes of PROWS K / V rows each
    const int q0 = qb * QBLOCK;
    int len = lens[seq];
    len = len < L ? len : L;
    const size_t rs = (size_t)3 * hidden;
    const unsigned short* qbase = qkv + (size_t)seq * L * rs + (size_t)head * HD;
    const unsigned short* kbase = qbase + hidden;
    const unsigned short* vbase = qbase + 2 * (size_t)hidden;
    unsigned short* obase = out + (size_t)seq * L * hidden + (size_t)head * HD;

    if (q0 >= len) {                                   // a block of padding rows only: zeros, nothing reads them but LayerNorm
        const int row = q0 + (tid >> 1);               // (two threads per row, half a head row each)
        if (row < L) {
            uint4* dst = reinterpret_cast<uint4*>(obase + (size_t)row * hidden + (tid & 1) * (HD / 2));
            const uint4 z = make_uint4(0, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < HD / 16; ++i) dst[i] = z;
        }
        return;
    }

    // the wave's 32 query rows as B operands of the KS k-steps over d (lane: row c, d = 16*ks + 8*g + [0,8))
    const int qrow = q0 + wave * 32 + c;
    v4u qf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        qf[ks] = v4u{0, 0, 0, 0};
        if (qrow < L) qf[ks] = *reinterpret_cast<const v4u*>(qbase + (size_t)qrow * rs + ks * 16 + g * 8);
    }

#if ATT_DMA
    // chunk staging by LDS-DMA: wave w brings rows 8w + PROWS*h .. + 7 of K and of V (one instruction each: 64 lanes x 16 B = 8 rows), lane l the
    // segment (l & 7) ^ f(row) of row l >> 3 into slot l & 7.  Rows beyond the sequence re-read its last row: finite values under p = 0
    // (a lane switched off would leave whatever the buffer held, and 0 x Inf is NaN).  Inline asm (M0 = LDS destination): hipcc neither
    // counts these loads nor knows that the LDS reads depend on them — the wait in front of the chunk's barrier is written out below.
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);      // (M0 takes an SGPR)
    const int dr = lane >> 3, dsg = (lane & 7) ^ ATT_SWZ(dr + 8 * (wave_u & 1));      // (a wave's rows start at a multiple of 8: bit 3 of the row = wave & 1)
    const unsigned k_dst = (unsigned)(size_t)((__attribute__((address_space(3))) unsigned short*)&k_lds[0][0]) + (unsigned)wave_u * 1024u;
    const unsigned v_dst = (unsigned)(size_t)((__attribute__((address_space(3))) unsigned short*)&v_lds[0][0]) + (unsigned)wave_u * 1024u;
    auto dma_chunk = [&](int ch, int buf) {
        const int k0 = ch * ATT_CHUNK;
#pragma unroll
        for (int h = 0; h < PASSES; ++h) {
            int key = k0 + wave * 8 + PROWS * h + dr;
            key = key < len ? key : len - 1;
            const unsigned voff = ((unsigned)key * (unsigned)rs + (unsigned)dsg * 8u) * 2u;
            const unsigned dk = k_dst + (unsigned)buf * (ATT_CHUNK * 128u) + (unsigned)h * (PROWS * 128u);
            const unsigned dv = v_dst + (unsigned)buf * (ATT_CHUNK * 128u) + (unsigned)h * (PROWS * 128u);
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff), "s"(kbase), "s"(dk) : "memory", "m0");
            asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" :: "v"(voff), "s"(vbase), "s"(dv) : "memory", "m0");
        }
    };
#endif
    // chunk staging.  K: thread -> rows r and r + 32, 16-byte segment seg (HD = 32: the one row tid >> 2, segment tid & 3).  V: thread -> the key pair pi, d segment dseg.
    const int kr = tid >> (HD == 64 ? 3 : 2), kseg = tid & (SEGS - 1);
    const int pi = wave * 8 + (lane & 7), dseg = lane >> 3;
    v4u kreg[PASSES], vreg[PASSES];
    auto load_chunk = [&](int ch) {
        const int k0 = ch * ATT_CHUNK;
#pragma unroll
        for (int h = 0; h < PASSES; ++h) {
            const int key = k0 + kr + PROWS * h;
            kreg[h] = v4u{0, 0, 0, 0};
            if (key < len) kreg[h] = *reinterpret_cast<const v4u*>(kbase + (size_t)key * rs + kseg * 8);
            const int vkey = ATT_VTR ? key : k0 + 2 * pi + h;                  // ATT_VTR: the same (row, segment) as K
            vreg[h] = v4u{0, 0, 0, 0};
            if (vkey < len) vreg[h] = *reinterpret_cast<const v4u*>(vbase + (size_t)vkey * rs + (ATT_VTR ? kseg : dseg) * 8);
        }
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
#if ATT_SWZL
        for (int h = 0; h < PASSES; ++h) *reinterpret_cast<v4u*>(&k_lds[buf][(kr + PROWS * h) * 64 + ((kseg ^ ATT_SWZ(kr + PROWS * h)) * 8)]) = kreg[h];
#pragma unroll
        for (int h = 0; h < (ATT_ABL == 6 ? 0 : PASSES); ++h) *reinterpret_cast<v4u*>(&v_lds[buf][(kr + PROWS * h) * 64 + ((kseg ^ ATT_SWZ(kr + PROWS * h)) * 8)]) = vreg[h];
#elif ATT_VTR
        for (int h = 0; h < PASSES; ++h) *reinterpret_cast<v4u*>(&k_lds[buf][(kr + PROWS * h) * KSTR + kseg * 8]) = kreg[h];
#pragma unroll
        for (int h = 0; h < (ATT_ABL == 6 ? 0 : PASSES); ++h) *reinterpret_cast<v4u*>(&v_lds[buf][(kr + PROWS * h) * VSTR + kseg * 8]) = vreg[h];
#else
        for (int h = 0; h < PASSES; ++h) *reinterpret_cast<v4u*>(&k_lds[buf][(kr + PROWS * h) * ATT_KSTR + kseg * 8]) = kreg[h];
#pragma unroll
        for (int w = 0; w < (ATT_ABL == 6 ? 0 : 4); ++w) {                  // element 2w and 2w + 1 of both keys -> V^T[d][key0], V^T[d][key0 + 1]
            const unsigned a = vreg[0][w], b = vreg[1][w];
            *reinterpret_cast<unsigned*>(&v_lds[buf][(dseg * 8 + 2 * w) * ATT_VSTR + 2 * pi]) = (a & 0xFFFFu) | (b << 16);
            *reinterpret_cast<unsigned*>(&v_lds[buf][(dseg * 8 + 2 * w + 1) * ATT_VSTR + 2 * pi]) = (a >> 16) | (b & 0xFFFF0000u);
        }
#endif
    };

    f32x16 o[DTN];
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int dt = 0; dt < DTN; ++dt) o[dt][r] = 0.0f;
    float m = ATT_NEG, lsum = 0.0f;
    const int nch = (len + ATT_CHUNK - 1) / ATT_CHUNK;
#if ATT_DMA
    dma_chunk(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
    load_chunk(0);
    store_chunk(0);
#endif
    __syncthreads();
    for (int ch = 0; ch < nch; ++ch) {
        const int cur = ch & 1;
#if ATT_DMA
        if (ATT_ABL != 4 && ATT_ABL != 7 && ch + 1 < nch) dma_chunk(ch + 1, cur ^ 1);      // (everybody left that buffer at the previous chunk's barrier)
#else
        if (ATT_ABL != 4 && ATT_ABL != 7 && ch + 1 < nch) load_chunk(ch + 1);
#endif
        // S^T tiles: keys t*32 + [0,32) of the chunk x the wave's 32 queries
        f32x16 s[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[t][r] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
#if ATT_SWZL
                const v4u kf = *reinterpret_cast<const v4u*>(&k_lds[ATT_ABL == 4 ? 0 : cur][(t * 32 + c) * 64 + (((ks * 2 + g) ^ ATT_SWZ(c)) * 8)]);
#else
                const v4u kf = *reinterpret_cast<const v4u*>(&k_lds[ATT_ABL == 4 ? 0 : cur][(t * 32 + c) * KSTR + ks * 16 + g * 8]);
#endif
                if (ATT_ABL != 2) s[t] = CmrBlk<DT>::mma(kf, qf[ks], s[t]);
                else s[t][ks] += __uint_as_float(kf[0] & 0x3F800000u);
            }
        }
        const int k0 = ch * ATT_CHUNK;
        if (k0 + ATT_CHUNK > len) {                    // the chunk holding the end of the sequence (wave-uniform)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (k0 + t * 32 + cmr_acc_row(r, lane) >= len) s[t][r] = ATT_NEG;
        }
        float cm = ATT_NEG;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) cm = fmaxf(cm, s[t][r]);
        cm = fmaxf(cm, __shfl_xor(cm, 32));
        const float mn = fmaxf(m, cm);
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * sc);
        const float msc = mn * sc;
        // two scores per instruction where the ISA has a packed form (v_pk_fma_f32, v_pk_add_f32: the kernel is bound by its VALU work —
        // 155 instructions per 16 MFMAs and chunk, 64 of them these multiply-adds and sums)
#if ATT_PK
        typedef float att_f2 __attribute__((ext_vector_type(2)));
        att_f2 ps2 = {0.0f, 0.0f};
        const att_f2 sc2 = {sc, sc}, nm2 = {-msc, -msc};
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                att_f2 x = {s[t][r], s[t][r + 1]};
                x = __builtin_elementwise_fma(x, sc2, nm2);
                if (ATT_ABL != 1) { x[0] = __builtin_amdgcn_exp2f(x[0]); x[1] = __builtin_amdgcn_exp2f(x[1]); }
                s[t][r] = x[0];
                s[t][r + 1] = x[1];
                ps2 += x;
            }
        const float ps = ps2[0] + ps2[1];
#else
        float ps = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float p = ATT_ABL == 1 ? fmaf(s[t][r], sc, -msc) : __builtin_amdgcn_exp2f(fmaf(s[t][r], sc, -msc));
                s[t][r] = p;
                ps += p;
            }
#endif
        // (after the first chunks the running maxima rarely move: alpha is exactly 1.0 in every lane then, and x * 1.0 == x)
        if (!ATT_SKIP_RESCALE || __any(mn != m)) {
            lsum = fmaf(lsum, alpha, ps);
            m = mn;
#pragma unroll
            for (int r = 0; r < 16; ++r)
#pragma unroll
                for (int dt = 0; dt < DTN; ++dt) o[dt][r] *= alpha;
        } else {
            lsum += ps;
        }
        // O^T += V^T P^T: four k-steps of 16 keys, DTN output tiles each; the P registers 8*sp .. 8*sp + 7 of tile t are the B operand as they are
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int sp = 0; sp < 2; ++sp) {
                v4u pb;
                pb[0] = enc_pack2<DT>(s[t][8 * sp + 0], s[t][8 * sp + 1]);
                pb[1] = enc_pack2<DT>(s[t][8 * sp + 2], s[t][8 * sp + 3]);
                pb[2] = enc_pack2<DT>(s[t][8 * sp + 4], s[t][8 * sp + 5]);
                pb[3] = enc_pack2<DT>(s[t][8 * sp + 6], s[t][8 * sp + 7]);
                const int kb = t * 32 + sp * 16 + 4 * g;
#pragma unroll
                for (int dt = 0; dt < DTN; ++dt) {
#if ATT_VTR
                    // the A operand of lane l: V[kb + {0..3, 8..11}][dt*32 + c].  A transposing read hands lane i of a 16-lane group column i of the
                    // 4 x 16 block whose row (i >> 2), columns 4 * (i & 3) .. + 3 that lane addresses (tools/probe/tr_probe.hip): rows = keys
                    // kb .. kb + 3, columns = d of this group's sixteen lanes
#if ATT_SWZL
                    // (row + 8 flips bit 2 of u = bit 1 of f: the second read's slot is the first one's ^ 2)
                    const int vrow_ = kb + ((lane & 15) >> 2);
                    const int vslot_ = (dt * 4 + 2 * ((lane >> 4) & 1) + ((lane & 3) >> 1)) ^ ATT_SWZ(vrow_);
                    const unsigned short* vblk = &v_lds[cur][vrow_ * 64 + vslot_ * 8 + 4 * (lane & 1)];
                    const unsigned short* vblk8 = &v_lds[cur][(vrow_ + 8) * 64 + (vslot_ ^ 2) * 8 + 4 * (lane & 1)];
#else
                    const unsigned short* vblk = &v_lds[cur][(kb + ((lane & 15) >> 2)) * VSTR + dt * 32 + 16 * ((lane >> 4) & 1) + 4 * (lane & 3)];
                    const unsigned short* vblk8 = vblk + 8 * VSTR;
#endif
                    typedef __attribute__((address_space(3))) att_v4s* lds_v4s;
                    const att_v4s lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)vblk);
                    const att_v4s hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)vblk8);
                    const uint2 lo = __builtin_bit_cast(uint2, lo4), hi = __builtin_bit_cast(uint2, hi4);
#else
                    const unsigned short* vrow = &v_lds[cur][(dt * 32 + c) * ATT_VSTR + kb];
                    const uint2 lo = *reinterpret_cast<const uint2*>(vrow);
                    const uint2 hi = *reinterpret_cast<const uint2*>(vrow + 8);
#endif
                    if (ATT_ABL != 3) o[dt] = CmrBlk<DT>::mma(v4u{lo.x, lo.y, hi.x, hi.y}, pb, o[dt]);
                    else o[dt][0] += __uint_as_float((lo.x ^ pb[0]) & 0x3F800000u);
                }
            }
        if (ATT_ABL != 4) {
#if ATT_DMA
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // my pieces of the next chunk have landed; the barrier says everybody's have
#else
            if (ch + 1 < nch) store_chunk(cur ^ 1);
#endif
            if (ATT_ABL != 5) __syncthreads();
        }
    }
    const float inv = 1.0f / (lsum + __shfl_xor(lsum, 32));
    if (qrow < L) {
#pragma unroll
        for (int dt = 0; dt < DTN; ++dt)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) {           // registers 4*rr .. 4*rr + 3 = d columns dt*32 + 8*rr + 4*g + [0,4)
                uint2 w;
                w.x = enc_pack2<DT>(o[dt][4 * rr + 0] * inv, o[dt][4 * rr + 1] * inv);
                w.y = enc_pack2<DT>(o[dt][4 * rr + 2] * inv, o[dt][4 * rr + 3] * inv);
                *reinterpret_cast<uint2*>(obase + (size_t)qrow * hidden + dt * 32 + 8 * rr + 4 * g) = w;
            }
    }
}

// The same attention for fp32 tensors, fp32 end to end: both products run on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32: every
// result a k-ordered fmaf chain), nothing is rounded to 16 bits.  Same orientation, S^T = K Q^T, so the statistics code is the 16-bit
// kernel's (the C/D lane map does not depend on the input type).  The operands of this MFMA are ONE float per lane, k = lane >> 5:
//   * QK^T: the order of d inside the sum is free as long as K and Q agree.  k-step (j, e), j = 0..7, e = 0..3, takes d = 8j + 4g + e
//     of lane half g, so a lane reads K from LDS — and its Q row from global memory, once — as 16-byte vectors [8j + 4g, + 4).
//     K rows are 68 floats apart in LDS (272 B: sixteen consecutive rows of a ds_read_b128 start in sixteen different 16-byte slots).
//   * PV, O^T = V^T P^T: register r of a score tile holds key (r & 3) + 8 (r >> 2) in lane half 0 and that key + 4 in lane half 1
//     (cmr_acc_row), which IS the B operand of a k-step over that key pair — no conversion, no lane movement.  The A operand of lane
//     (c, g) is V[key + 4g][32 dt + c]: 32 consecutive floats per lane half; V rows are 72 floats apart (4 rows = 288 floats = 32
//     banks mod 64: the two halves of a ds_read_b32 use disjoint banks).
// 128 MFMAs of 64 cycles per 64-key chunk and wave against ~140 VALU instructions: the matrix pipe is the long leg here (the 16-bit
// kernel's is the softmax), so K / V chunks are SINGLE-buffered in LDS (35 KiB per workgroup, the next chunk's global loads in flight in
// registers while this one is multiplied, two barriers per chunk) and one workgroup shape (4 waves, 128 query rows) serves every l.
// The exponent is (s - max) * sc, not fma(s, sc, -max * sc): the difference is rounded where it is small, so the weights of the keys
// that matter carry no rounding error of the (large) maximum — 32 more VALU instructions per chunk next to 8192 MFMA cycles.
// HD = 32 (the 384-hidden tier): j runs 0..3 over the same d = 8j + 4g + e, PV has one output tile (o[1]) — 64 + 32 MFMAs per chunk and wave
// instead of 128 + 128; a row is eight 16-byte segments, so a chunk is two staging passes of 32 rows.  K rows 36 floats apart (144 B = 9 slots
// of 16 B, odd: sixteen different slots again), V rows 40 floats apart (4 rows = 160 floats = 32 banks mod 64, as 72).  19 KiB of LDS.
#define ATT32_KSTR 68
#define ATT32_VSTR 72
#define ATT32_KSTR_HD32 36
#define ATT32_VSTR_HD32 40
template <int HD>
__global__ __launch_bounds__(256, 2) void attn_fwd_f32_kernel(const float* __restrict__ qkv, const int* __restrict__ lens, int L, int hidden, int n_heads,
                                                              int n_qblocks, int total, float sc /* log2(e) / sqrt(HD) */, float* __restrict__ out) {
    static_assert(HD == 64 || HD == 32, "head width 64 or 32");
    constexpr int KSTR = HD == 64 ? ATT32_KSTR : ATT32_KSTR_HD32, VSTR = HD == 64 ? ATT32_VSTR : ATT32_VSTR_HD32;      // LDS row strides, floats
    constexpr int NJ = HD / 8, DTN = HD / 32, SEGS = HD / 4;       // QK^T steps of 4 + 4 d; 32-column output tiles of PV; 16-byte segments of a K / V row
    constexpr int SROWS = 256 / SEGS, PASSES = ATT_CHUNK / SROWS;  // staging passes of SROWS K / V rows each
    __shared__ __attribute__((aligned(16))) float k_lds[ATT_CHUNK * KSTR];
    __shared__ __attribute__((aligned(16))) float v_lds[ATT_CHUNK * VSTR];
    // workgroup id -> (sequence, head, query block): as attn_fwd_kernel
    const int xcd = (int)(blockIdx.x & 7), j0 = (int)(blockIdx.x >> 3);
    const int pair = (j0 / n_qblocks) * 8 + xcd;
    if (pair >= total / n_qblocks) return;
    const int qb = j0 % n_qblocks, head = pair % n_heads, seq = total / (n_qblocks * n_heads) - 1 - pair / n_heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 5, c = lane & 31;
    const int q0 = qb * ATT_QBLOCK;
    int len = lens[seq];
    len = len < L ? len : L;
    const size_t rs = (size_t)3 * hidden;
    const float* qbase = qkv + (size_t)seq * L * rs + (size_t)head * HD;
    const float* kbase = qbase + hidden;
    const float* vbase = qbase + 2 * (size_t)hidden;
    float* obase = out + (size_t)seq * L * hidden + (size_t)head * HD;

    if (q0 >= len) {                                   // a block of padding rows only: zeros
        const int row = q0 + (tid >> 1);
        if (row < L) {
            float4* dst = reinterpret_cast<float4*>(obase + (size_t)row * hidden + (tid & 1) * (HD / 2));
            const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
            for (int i = 0; i < HD / 8; ++i) dst[i] = z;
        }
        return;
    }

    // the wave's 32 query rows as B operands: lane (c, g) holds d = 8j + 4g + [0,4) of row q0 + 32 wave + c in qf[j]
    const int qrow = q0 + wave * 32 + c;
    float4 qf[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        qf[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (qrow < L) qf[j] = *reinterpret_cast<const float4*>(qbase + (size_t)qrow * rs + 8 * j + 4 * g);
    }

    // chunk staging: thread -> 16-byte segment sseg of rows srow + SROWS h (16 h, h = 0..3; HD = 32: 32 h, h = 0..1) of K and of V; rows behind
    // the sequence's end are zeros
    const int srow = tid >> (HD == 64 ? 4 : 3), sseg = tid & (SEGS - 1);
    float4 kreg[PASSES], vreg[PASSES];
    auto load_chunk = [&](int ch) {
        const int k0 = ch * ATT_CHUNK;
#pragma unroll
        for (int h = 0; h < PASSES; ++h) {
            const int key = k0 + srow + SROWS * h;
            kreg[h] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            vreg[h] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (key < len) {
                kreg[h] = *reinterpret_cast<const float4*>(kbase + (size_t)key * rs + sseg * 4);
                vreg[h] = *reinterpret_cast<const float4*>(vbase + (size_t)key * rs + sseg * 4);
            }
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int h = 0; h < PASSES; ++h) {
            *reinterpret_cast<float4*>(&k_lds[(srow + SROWS * h) * KSTR + sseg * 4]) = kreg[h];
            *reinterpret_cast<float4*>(&v_lds[(srow + SROWS * h) * VSTR + sseg * 4]) = vreg[h];
        }
    };

    f32x16 o[DTN];
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int dt = 0; dt < DTN; ++dt) o[dt][r] = 0.0f;
    float m = ATT_NEG, lsum = 0.0f;
    const int nch = (len + ATT_CHUNK - 1) / ATT_CHUNK;
    load_chunk(0);
    for (int ch = 0; ch < nch; ++ch) {
        store_chunk();
        __syncthreads();
        if (ch + 1 < nch) load_chunk(ch + 1);
        // S^T tiles: keys t*32 + [0,32) of the chunk x the wave's 32 queries
        f32x16 s[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) s[t][r] = 0.0f;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float4 kf = *reinterpret_cast<const float4*>(&k_lds[(t * 32 + c) * KSTR + 8 * j + 4 * g]);
                s[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, qf[j].x, s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, qf[j].y, s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, qf[j].z, s[t], 0, 0, 0);
                s[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, qf[j].w, s[t], 0, 0, 0);
            }
        }
        const int k0 = ch * ATT_CHUNK;
        if (k0 + ATT_CHUNK > len) {                    // the chunk holding the end of the sequence (wave-uniform)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (k0 + t * 32 + cmr_acc_row(r, lane) >= len) s[t][r] = ATT_NEG;
        }
        float cm = ATT_NEG;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) cm = fmaxf(cm, s[t][r]);
        cm = fmaxf(cm, __shfl_xor(cm, 32));
        const float mn = fmaxf(m, cm);
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * sc);
        typedef float att_f2 __attribute__((ext_vector_type(2)));
        att_f2 ps2 = {0.0f, 0.0f};
        const att_f2 sc2 = {sc, sc}, mn2 = {mn, mn};
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; r += 2) {
                att_f2 x = {s[t][r], s[t][r + 1]};
                x = (x - mn2) * sc2;
                x[0] = __builtin_amdgcn_exp2f(x[0]);
                x[1] = __builtin_amdgcn_exp2f(x[1]);
                s[t][r] = x[0];
                s[t][r + 1] = x[1];
                ps2 += x;
            }
        lsum = fmaf(lsum, alpha, ps2[0] + ps2[1]);
        m = mn;
#pragma unroll
        for (int r = 0; r < 16; ++r)
#pragma unroll
            for (int dt = 0; dt < DTN; ++dt) o[dt][r] *= alpha;
        // O^T += V^T P^T: register r of tile t is the B operand of the k-step over keys {row(r), row(r) + 4} of the tile
        const float* vp = &v_lds[4 * g * VSTR + c];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int kr = t * 32 + (r & 3) + 8 * (r >> 2);
#pragma unroll
                for (int dt = 0; dt < DTN; ++dt) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[kr * VSTR + 32 * dt], s[t][r], o[dt], 0, 0, 0);
            }
        __syncthreads();                               // everybody has read this chunk: the next one may overwrite it
    }
    const float inv = 1.0f / (lsum + __shfl_xor(lsum, 32));
    if (qrow < L) {
#pragma unroll
        for (int dt = 0; dt < DTN; ++dt)
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)             // registers 4*rr .. 4*rr + 3 = d columns dt*32 + 8*rr + 4*g + [0,4)
                *reinterpret_cast<float4*>(obase + (size_t)qrow * hidden + dt * 32 + 8 * rr + 4 * g) =
                    make_float4(o[dt][4 * rr + 0] * inv, o[dt][4 * rr + 1] * inv, o[dt][4 * rr + 2] * inv, o[dt][4 * rr + 3] * inv);
    }
}

// sc = log2(e) / sqrt(HD): the scores' scale folded into the base-2 exponent
template <int HD> static constexpr float att_scale() { return HD == 64 ? 1.4426950408889634f * 0.125f : 1.4426950408889634f * 0.17677669529663687f; }

template <int HD>
static hipError_t launch_attention_f32(const void* qkv, const int* lens, int b, int L, int n_heads, void* out, hipStream_t s) {
    const int hidden = n_heads * HD;
    const int n_qblocks = (L + ATT_QBLOCK - 1) / ATT_QBLOCK;
    const long long total = (long long)n_qblocks * n_heads * b;
    if (total > (1LL << 28)) return hipErrorInvalidValue;
    const long long pairs = (long long)n_heads * b;
    const int per = (int)((pairs + 7) / 8) * n_qblocks;
    const float sc = att_scale<HD>();
    hipLaunchKernelGGL(attn_fwd_f32_kernel<HD>, dim3((unsigned)(per * 8)), dim3(256), 0, s, reinterpret_cast<const float*>(qkv), lens, L, hidden, n_heads, n_qblocks,
                       (int)total, sc, reinterpret_cast<float*>(out));
    return hipGetLastError();
}

#ifndef ATT_WAVES_MODE
#define ATT_WAVES_MODE 0      // 0: eight waves per workgroup for mini-batches of >= 256 (padded) tokens, four below; 4 / 8: always
#endif
template <int DT, int NW, int HD>
static hipError_t launch_attention(const void* qkv, const int* lens, int b, int L, int n_heads, void* out, hipStream_t s) {
    static_assert(ATT_VTR || NW == 4, "the transposed-store layout of V is a 4-wave mapping");
    const int hidden = n_heads * HD;
    const int n_qblocks = (L + NW * 32 - 1) / (NW * 32);
    const long long total = (long long)n_qblocks * n_heads * b;
    if (total > (1LL << 28)) return hipErrorInvalidValue;
    const long long pairs = (long long)n_heads * b;
    const int per = (int)((pairs + 7) / 8) * n_qblocks;        // workgroups per XCD: its share of the (sequence, head) pairs x their query blocks
    const float sc = att_scale<HD>();
    hipLaunchKernelGGL((attn_fwd_kernel<DT, NW, HD>), dim3((unsigned)(per * 8)), dim3(NW * 64), 0, s, reinterpret_cast<const unsigned short*>(qkv), lens, L, hidden,
                       n_heads, n_qblocks, (int)total, sc, reinterpret_cast<unsigned short*>(out));
    return hipGetLastError();
}

// head_dim 64 or 32 (the caller checks).  32-wide heads run on 4 waves for every l (comment at attn_fwd_kernel).
hipError_t cmr_launch_attention(const void* qkv, int dtype, const int* lens, int b, int L, int n_heads, int head_dim, void* out, hipStream_t s) {
    if (head_dim == 32) {
        if (dtype == CMR_DT_F32) return launch_attention_f32<32>(qkv, lens, b, L, n_heads, out, s);
#if ATT_VTR && !ATT_SWZL && !ATT_DMA
        if (dtype == CMR_DT_BF16) return launch_attention<CMR_DT_BF16, 4, 32>(qkv, lens, b, L, n_heads, out, s);
        return launch_attention<CMR_DT_F16, 4, 32>(qkv, lens, b, L, n_heads, out, s);
#else
        return hipErrorInvalidValue;                   // a development build of the 64-wide layouts: no 16-bit HD = 32 kernel in it
#endif
    }
    if (head_dim != 64) return hipErrorInvalidValue;
    if (dtype == CMR_DT_F32) return launch_attention_f32<64>(qkv, lens, b, L, n_heads, out, s);
    const bool eight = ATT_VTR && (ATT_WAVES_MODE == 8 || (ATT_WAVES_MODE == 0 && L >= 256));
    if (dtype == CMR_DT_BF16) return eight ? launch_attention<CMR_DT_BF16, (ATT_VTR ? 8 : 4), 64>(qkv, lens, b, L, n_heads, out, s) : launch_attention<CMR_DT_BF16, 4, 64>(qkv, lens, b, L, n_heads, out, s);
    return eight ? launch_attention<CMR_DT_F16, (ATT_VTR ? 8 : 4), 64>(qkv, lens, b, L, n_heads, out, s) : launch_attention<CMR_DT_F16, 4, 64>(qkv, lens, b, L, n_heads, out, s);
}

// ------------------------------------------------------------------------------------------------ bias + residual + LayerNorm
// One wave per token row, d = 4 * d4 elements, lane holds vectors lane, lane + 64, ... (8-byte loads: a wave instruction reads
// 512 contiguous bytes).  Sum, mean and variance in fp32 over the UNROUNDED sum y + bias + residual (PyTorch rounds to 16 bits
// after the bias and again after the residual add).
// v[VPL][4] = the lane's elements of one row (vector i = j*64 + lane, valid while i < d4): mean / variance over the wave, then
// (v - mean) * rstd * gamma + beta, rounded once, written as 8-byte vectors
template <int DT, int VPL>
__device__ __forceinline__ void enc_ln_store(float (&v)[VPL][4], float sum, int lane, int d4, const typename EncVec<DT>::V4* __restrict__ gamma,
                                             const typename EncVec<DT>::V4* __restrict__ beta, float eps, typename EncVec<DT>::V4* __restrict__ out_row) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    const float inv_d = 1.0f / (float)(4 * d4);
    const float mean = sum * inv_d;
    float sq = 0.0f;
#pragma unroll
    for (int j = 0; j < VPL; ++j)
        if (j * 64 + lane < d4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float t = v[j][e] - mean; sq = fmaf(t, t, sq); }
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
    const float rstd = rsqrtf(sq * inv_d + eps);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = j * 64 + lane;
        if (i < d4) {
            float gm[4], bt[4];
            enc_get4<DT>(gm, gamma[i]);
            enc_get4<DT>(bt, beta[i]);
            out_row[i] = enc_put4<DT>(fmaf((v[j][0] - mean) * rstd, gm[0], bt[0]), fmaf((v[j][1] - mean) * rstd, gm[1], bt[1]),
                                      fmaf((v[j][2] - mean) * rstd, gm[2], bt[2]), fmaf((v[j][3] - mean) * rstd, gm[3], bt[3]));
        }
    }
}
template <int DT> __device__ __forceinline__ void enc_acc4(float (&f)[4], typename EncVec<DT>::V4 a) {
    float t[4];
    enc_get4<DT>(t, a);
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] += t[e];
}

template <int DT, int VPL>
__global__ __launch_bounds__(256) void add_ln_kernel(const typename EncVec<DT>::V4* __restrict__ y, const typename EncVec<DT>::V4* __restrict__ bias, const typename EncVec<DT>::V4* __restrict__ res,
                                                     const typename EncVec<DT>::V4* __restrict__ gamma, const typename EncVec<DT>::V4* __restrict__ beta, float eps, long long rows,
                                                     int d4, typename EncVec<DT>::V4* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    float v[VPL][4];
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = j * 64 + lane;
        v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0.0f;
        if (i < d4) {
            enc_acc4<DT>(v[j], y[row * d4 + i]);
            if (bias) enc_acc4<DT>(v[j], bias[i]);
            if (res) enc_acc4<DT>(v[j], res[row * d4 + i]);
            sum += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        }
    }
    enc_ln_store<DT, VPL>(v, sum, lane, d4, gamma, beta, eps, out + row * d4);
}

// The same for d % 8 == 0 with 16-byte vectors: sixteen lanes per token row, four rows per wave (a wave instruction still reads
// contiguous 256-byte pieces, and each lane has 2 * VPL 16-byte loads in flight instead of 8-byte ones: the one-row-per-wave
// form above ran at 4.5 TB/s of algorithmic traffic at 768 columns).
template <int DT> __device__ __forceinline__ void enc_acc8(float (&f)[8], typename EncVec<DT>::V8 a) {
    float t[8];
    enc_get8<DT>(t, a);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] += t[e];
}
template <int DT, int VPL>
__global__ __launch_bounds__(256) void add_ln16_kernel(const typename EncVec<DT>::V8* __restrict__ y, const typename EncVec<DT>::V8* __restrict__ bias, const typename EncVec<DT>::V8* __restrict__ res,
                                                       const typename EncVec<DT>::V8* __restrict__ gamma, const typename EncVec<DT>::V8* __restrict__ beta, float eps, long long rows,
                                                       int d8, typename EncVec<DT>::V8* __restrict__ out) {
    const int sub = threadIdx.x & 15;
    const long long row = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (row >= rows) return;                           // whole 16-lane groups leave together: the shuffles below stay inside a group
    float v[VPL][8];
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = j * 16 + sub;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[j][e] = 0.0f;
        if (i < d8) {
            enc_acc8<DT>(v[j], y[row * d8 + i]);
            if (bias) enc_acc8<DT>(v[j], bias[i]);
            if (res) enc_acc8<DT>(v[j], res[row * d8 + i]);
            sum += ((v[j][0] + v[j][1]) + (v[j][2] + v[j][3])) + ((v[j][4] + v[j][5]) + (v[j][6] + v[j][7]));
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    const float inv_d = 1.0f / (float)(8 * d8);
    const float mean = sum * inv_d;
    float sq = 0.0f;
#pragma unroll
    for (int j = 0; j < VPL; ++j)
        if (j * 16 + sub < d8) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float t = v[j][e] - mean; sq = fmaf(t, t, sq); }
        }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
    const float rstd = rsqrtf(sq * inv_d + eps);
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = j * 16 + sub;
        if (i < d8) {
            float gm[8], bt[8];
            enc_get8<DT>(gm, gamma[i]);
            enc_get8<DT>(bt, beta[i]);
            float w[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) w[e] = fmaf((v[j][e] - mean) * rstd, gm[e], bt[e]);
            out[row * d8 + i] = enc_put8<DT>(w);
        }
    }
}

// The LAST layer's bias + residual + LayerNorm with the encoder tail folded in (embedding_model/BGEEmbedding.py:15-28 mean_pooling,
// :126-127 F.normalize): the layer's output [b, l, d] is never written.  A block takes 16 consecutive tokens of ONE sequence (l is a
// multiple of 16), normalises them as add_ln16_kernel does, rounds to 16 bits (what the hidden state would have held), zeroes the
// tokens at or behind the sequence's length and adds the 16 tokens up in a fixed order (xor tree inside a wave, waves 0..3 in
// LDS): one fp32 partial row [d] per block, 1/16 of the bytes of the hidden state at 4 bytes instead of 2 -> an eighth of the
// write, and nothing is read back but these partials.  Blocks that hold only padding leave at once (no loads, no partial).
// pool_finish_kernel then adds a sequence's partials in block order, divides by the token count and L2-normalises (eps 1e-12).
// SLABS = true (the short-row route's last layer): y is not a 16-bit tensor but the n_split fp32 slabs [n_split, b*l, d] of small_linear_kernel's
// partials form, added in slab order as add_ln_partials_kernel adds them (slabs: float4 pairs, slab_stride = b*l*d / 4 of them apart).
template <int DT, int VPL, bool SLABS = false>
__global__ __launch_bounds__(256) void add_ln16_pool_kernel(const typename EncVec<DT>::V8* __restrict__ y, const typename EncVec<DT>::V8* __restrict__ bias, const typename EncVec<DT>::V8* __restrict__ res,
                                                            const typename EncVec<DT>::V8* __restrict__ gamma, const typename EncVec<DT>::V8* __restrict__ beta, float eps, int l, int d8,
                                                            const int* __restrict__ lens, float* __restrict__ partial, const float4* __restrict__ slabs = nullptr, int n_split = 0,
                                                            long long slab_stride = 0) {
    __shared__ float red[4][16 * VPL * 8];
    const int sub = threadIdx.x & 15, grp = threadIdx.x >> 4, wave = threadIdx.x >> 6;
    const int seq = blockIdx.y, t0 = blockIdx.x * 16;
    const int len = lens[seq];
    if (t0 >= len) return;                                          // a block of padding only
    const long long row = (long long)seq * l + t0 + grp;
    float v[VPL][8];
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = j * 16 + sub;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[j][e] = 0.0f;
        if (i < d8) {
            if constexpr (SLABS) {
                const float4* p = slabs + (row * d8 + i) * 2;
                for (int sp = 0; sp < n_split; ++sp) {
                    const float4 lo = p[sp * slab_stride], hi = p[sp * slab_stride + 1];
                    v[j][0] += lo.x; v[j][1] += lo.y; v[j][2] += lo.z; v[j][3] += lo.w;
                    v[j][4] += hi.x; v[j][5] += hi.y; v[j][6] += hi.z; v[j][7] += hi.w;
                }
            } else {
                enc_acc8<DT>(v[j], y[row * d8 + i]);
            }
            if (bias) enc_acc8<DT>(v[j], bias[i]);
            if (res) enc_acc8<DT>(v[j], res[row * d8 + i]);
            sum += ((v[j][0] + v[j][1]) + (v[j][2] + v[j][3])) + ((v[j][4] + v[j][5]) + (v[j][6] + v[j][7]));
        }
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
    const float inv_d = 1.0f / (float)(8 * d8);
    const float mean = sum * inv_d;
    float sq = 0.0f;
#pragma unroll
    for (int j = 0; j < VPL; ++j)
        if (j * 16 + sub < d8) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float t = v[j][e] - mean; sq = fmaf(t, t, sq); }
        }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) sq += __shfl_xor(sq, off);
    const float rstd = rsqrtf(sq * inv_d + eps);
    const bool live = t0 + grp < len;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = j * 16 + sub;
        if (i < d8) {
            float gm[8], bt[8];
            enc_get8<DT>(gm, gamma[i]);
            enc_get8<DT>(bt, beta[i]);
#pragma unroll
            for (int e = 0; e < 8; e += 2) {
                const float w0 = fmaf((v[j][e] - mean) * rstd, gm[e], bt[e]), w1 = fmaf((v[j][e + 1] - mean) * rstd, gm[e + 1], bt[e + 1]);
                if constexpr (DT == CMR_DT_F32) {      // the stored hidden state would have held these floats: nothing to round
                    v[j][e] = w0;
                    v[j][e + 1] = w1;
                } else {                               // round to 16 bits as the stored hidden state would be, then back
                    enc_unpack2<DT>(enc_pack2<DT>(w0, w1), v[j][e], v[j][e + 1]);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float x = live ? v[j][e] : 0.0f;
            x += __shfl_xor(x, 16);               // the wave's four tokens: a fixed tree
            x += __shfl_xor(x, 32);
            v[j][e] = x;
        }
    }
    if ((threadIdx.x & 63) < 16) {
#pragma unroll
        for (int j = 0; j < VPL; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) red[wave][(j * 16 + sub) * 8 + e] = v[j][e];
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        float* dst = partial + ((size_t)seq * gridDim.x + blockIdx.x) * (size_t)(8 * d8);
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int i = j * 16 + sub;
            if (i < d8) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = ((red[0][i * 8 + e] + red[1][i * 8 + e]) + red[2][i * 8 + e]) + red[3][i * 8 + e];
                reinterpret_cast<float4*>(dst + i * 8)[0] = make_float4(o[0], o[1], o[2], o[3]);
                reinterpret_cast<float4*>(dst + i * 8)[1] = make_float4(o[4], o[5], o[6], o[7]);
            }
        }
    }
}

// out[seq] = normalise(sum over the sequence's live blocks of partial / len): one block per sequence
__global__ __launch_bounds__(256) void pool_finish_kernel(const float* __restrict__ partial, const int* __restrict__ lens, int nblk, int d, int normalize,
                                                          float* __restrict__ out) {
    __shared__ float wsum[4];
    const int seq = blockIdx.x, len = lens[seq];
    const int live = len > 0 ? (len + 15) / 16 : 0;
    const float inv = len > 0 ? 1.0f / (float)len : 0.0f;
    float ss = 0.0f;
    float keep[8];                                                  // d <= 2048 = 256 threads x 8
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int f = r * 256 + threadIdx.x;
        float s = 0.0f;
        if (f < d)
            for (int b = 0; b < live && b < nblk; ++b) s += partial[((size_t)seq * nblk + b) * d + f];
        keep[r] = s * inv;
        ss = fmaf(keep[r], keep[r], ss);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float norm = sqrtf((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
    const float scale = normalize ? 1.0f / fmaxf(norm, 1e-12f) : 1.0f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int f = r * 256 + threadIdx.x;
        if (f < d) out[(size_t)seq * d + f] = keep[r] * scale;
    }
}

// BertEmbeddings: LayerNorm(word[ids[t]] + position[t mod L] + token_type[tt[t]]), one wave per token (tt == NULL: type 0).
// Ids outside the tables are clamped into them (PyTorch's gather would fault the device instead).
template <int DT, int VPL>
__global__ __launch_bounds__(256) void embed_ln_kernel(const long long* __restrict__ ids, const long long* __restrict__ tt,
                                                       const typename EncVec<DT>::V4* __restrict__ word, const typename EncVec<DT>::V4* __restrict__ pos, const typename EncVec<DT>::V4* __restrict__ type,
                                                       const typename EncVec<DT>::V4* __restrict__ gamma, const typename EncVec<DT>::V4* __restrict__ beta, float eps, long long rows,
                                                       int L, int d4, int vocab, int n_pos, int n_types, int pos_off, typename EncVec<DT>::V4* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    long long id = ids[row], ty = tt ? tt[row] : 0;
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    ty = ty < 0 ? 0 : (ty >= n_types ? n_types - 1 : ty);
    int p = (int)(row % L) + pos_off;      // RoBERTa-style tables start at padding_idx + 1 (right-padded rows: token t is position t + offset)
    p = p >= n_pos ? n_pos - 1 : p;
    float v[VPL][4];
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = j * 64 + lane;
        v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0.0f;
        if (i < d4) {
            enc_acc4<DT>(v[j], word[id * d4 + i]);
            enc_acc4<DT>(v[j], pos[(long long)p * d4 + i]);
            enc_acc4<DT>(v[j], type[ty * d4 + i]);
            sum += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        }
    }
    enc_ln_store<DT, VPL>(v, sum, lane, d4, gamma, beta, eps, out + row * d4);
}

// The same from RAGGED token ids: ids32 holds the sequences' tokens back to back (int32), sequence s = ids32[off[s] .. off[s + 1]);
// row (s, t) of the [b, L] mini-batch embeds token t of sequence s, or token 0 behind the sequence's end (those rows are padding:
// attention masks them as keys, the pooling leaves them out).  No padded id / mask / token-type tensors exist on either side of
// the link: the host concatenates the tokenizer's output and ships lens | offsets | ids in ONE copy.  Token type 0 (one segment).
template <int DT, int VPL>
__global__ __launch_bounds__(256) void embed_ln_ragged_kernel(const int* __restrict__ ids32, const int* __restrict__ off, const typename EncVec<DT>::V4* __restrict__ word,
                                                              const typename EncVec<DT>::V4* __restrict__ pos, const typename EncVec<DT>::V4* __restrict__ type, const typename EncVec<DT>::V4* __restrict__ gamma,
                                                              const typename EncVec<DT>::V4* __restrict__ beta, float eps, long long rows, int L, int d4, int vocab, int n_pos,
                                                              int pos_off, typename EncVec<DT>::V4* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const int seq = (int)(row / L), t = (int)(row % L);
    const int o0 = off[seq], len = off[seq + 1] - o0;
    long long id = t < len ? ids32[o0 + t] : 0;
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    int p = t + pos_off;
    p = p >= n_pos ? n_pos - 1 : p;
    float v[VPL][4];
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = j * 64 + lane;
        v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0.0f;
        if (i < d4) {
            enc_acc4<DT>(v[j], word[id * d4 + i]);
            enc_acc4<DT>(v[j], pos[(long long)p * d4 + i]);
            enc_acc4<DT>(v[j], type[i]);
            sum += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        }
    }
    enc_ln_store<DT, VPL>(v, sum, lane, d4, gamma, beta, eps, out + row * d4);
}

template <int DT>
static hipError_t launch_embed_ln_ragged(const int* ids32, const int* off, const void* word, const void* pos, const void* type, const void* gamma,
                                         const void* beta, float eps, long long rows, int L, int d, int vocab, int n_pos, int pos_off, void* out, hipStream_t s) {
    const int d4 = d / 4, vpl = (d4 + 63) / 64;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define ENC_EMBR(V)                                                                                                                       \
    hipLaunchKernelGGL((embed_ln_ragged_kernel<DT, V>), grid, block, 0, s, ids32, off, reinterpret_cast<const typename EncVec<DT>::V4*>(word), reinterpret_cast<const typename EncVec<DT>::V4*>(pos), \
                       reinterpret_cast<const typename EncVec<DT>::V4*>(type), reinterpret_cast<const typename EncVec<DT>::V4*>(gamma), reinterpret_cast<const typename EncVec<DT>::V4*>(beta), eps, rows, \
                       L, d4, vocab, n_pos, pos_off, reinterpret_cast<typename EncVec<DT>::V4*>(out))
    switch (vpl) {
        case 1: ENC_EMBR(1); break;
        case 2: ENC_EMBR(2); break;
        case 3: ENC_EMBR(3); break;
        case 4: ENC_EMBR(4); break;
        case 5: case 6: ENC_EMBR(6); break;
        case 7: case 8: ENC_EMBR(8); break;
        default: return hipErrorInvalidValue;
    }
#undef ENC_EMBR
    return hipGetLastError();
}

hipError_t cmr_launch_embed_layernorm_ragged(const int* ids32, const int* off, const void* word, const void* pos, const void* type, const void* gamma,
                                             const void* beta, float eps, long long rows, int L, int d, int vocab, int n_pos, int pos_off, int dtype,
                                             void* out, hipStream_t s) {
    if (dtype == CMR_DT_BF16) return launch_embed_ln_ragged<CMR_DT_BF16>(ids32, off, word, pos, type, gamma, beta, eps, rows, L, d, vocab, n_pos, pos_off, out, s);
    if (dtype == CMR_DT_F32) return launch_embed_ln_ragged<CMR_DT_F32>(ids32, off, word, pos, type, gamma, beta, eps, rows, L, d, vocab, n_pos, pos_off, out, s);
    return launch_embed_ln_ragged<CMR_DT_F16>(ids32, off, word, pos, type, gamma, beta, eps, rows, L, d, vocab, n_pos, pos_off, out, s);
}

#ifndef ENC_LN_FEW_ROWS
#define ENC_LN_FEW_ROWS 256
#endif
template <int DT>
static hipError_t launch_add_ln(const void* y, const void* bias, const void* res, const void* gamma, const void* beta, float eps, long long rows,
                                int d, void* out, hipStream_t s) {
    const bool al16 = (((uintptr_t)y | (uintptr_t)bias | (uintptr_t)res | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)out) & 15) == 0;
    // A handful of rows (one short query: 16 .. 128 token rows, 24 / 48 of these launches per encode) is all latency: a WAVE per row (8-byte
    // vectors, three or four per lane and array at 768 / 1024-d) instead of sixteen lanes per row (six / eight 16-byte vectors per lane) —
    // a quarter of the dependent loads per lane, four times the waves.  Above, the 16-byte kernel's bandwidth wins (14.6 us at 16 K rows).
    const bool few = rows <= ENC_LN_FEW_ROWS && d % 4 == 0 && (d / 4 + 63) / 64 <= 8;
    if (d % 8 == 0 && al16 && !few) {
        const int d8 = d / 8, vpl16 = (d8 + 15) / 16;
        const dim3 grid16((unsigned)((rows + 15) / 16)), block16(256);
#define ENC_LN16(V)                                                                                                                       \
    hipLaunchKernelGGL((add_ln16_kernel<DT, V>), grid16, block16, 0, s, reinterpret_cast<const typename EncVec<DT>::V8*>(y), reinterpret_cast<const typename EncVec<DT>::V8*>(bias), \
                       reinterpret_cast<const typename EncVec<DT>::V8*>(res), reinterpret_cast<const typename EncVec<DT>::V8*>(gamma), reinterpret_cast<const typename EncVec<DT>::V8*>(beta), eps, \
                       rows, d8, reinterpret_cast<typename EncVec<DT>::V8*>(out))
        switch (vpl16) {
            case 1: ENC_LN16(1); break;
            case 2: ENC_LN16(2); break;
            case 3: case 4: ENC_LN16(4); break;
            case 5: case 6: ENC_LN16(6); break;
            case 7: case 8: ENC_LN16(8); break;
            case 9: case 10: case 11: case 12: ENC_LN16(12); break;
            case 13: case 14: case 15: case 16: ENC_LN16(16); break;
            default: return hipErrorInvalidValue;
        }
#undef ENC_LN16
        return hipGetLastError();
    }
    const int d4 = d / 4, vpl = (d4 + 63) / 64;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define ENC_LN(V)                                                                                                                     \
    hipLaunchKernelGGL((add_ln_kernel<DT, V>), grid, block, 0, s, reinterpret_cast<const typename EncVec<DT>::V4*>(y), reinterpret_cast<const typename EncVec<DT>::V4*>(bias), \
                       reinterpret_cast<const typename EncVec<DT>::V4*>(res), reinterpret_cast<const typename EncVec<DT>::V4*>(gamma), reinterpret_cast<const typename EncVec<DT>::V4*>(beta), eps, \
                       rows, d4, reinterpret_cast<typename EncVec<DT>::V4*>(out))
    switch (vpl) {
        case 1: ENC_LN(1); break;
        case 2: ENC_LN(2); break;
        case 3: ENC_LN(3); break;
        case 4: ENC_LN(4); break;
        case 5: case 6: ENC_LN(6); break;
        case 7: case 8: ENC_LN(8); break;
        default: return hipErrorInvalidValue;
    }
#undef ENC_LN
    return hipGetLastError();
}

template <int DT>
static hipError_t launch_embed_ln(const long long* ids, const long long* tt, const void* word, const void* pos, const void* type, const void* gamma,
                                  const void* beta, float eps, long long rows, int L, int d, int vocab, int n_pos, int n_types, int pos_off, void* out,
                                  hipStream_t s) {
    const int d4 = d / 4, vpl = (d4 + 63) / 64;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define ENC_EMB(V)                                                                                                                       \
    hipLaunchKernelGGL((embed_ln_kernel<DT, V>), grid, block, 0, s, ids, tt, reinterpret_cast<const typename EncVec<DT>::V4*>(word), reinterpret_cast<const typename EncVec<DT>::V4*>(pos), \
                       reinterpret_cast<const typename EncVec<DT>::V4*>(type), reinterpret_cast<const typename EncVec<DT>::V4*>(gamma), reinterpret_cast<const typename EncVec<DT>::V4*>(beta), eps, rows, \
                       L, d4, vocab, n_pos, n_types, pos_off, reinterpret_cast<typename EncVec<DT>::V4*>(out))
    switch (vpl) {
        case 1: ENC_EMB(1); break;
        case 2: ENC_EMB(2); break;
        case 3: ENC_EMB(3); break;
        case 4: ENC_EMB(4); break;
        case 5: case 6: ENC_EMB(6); break;
        case 7: case 8: ENC_EMB(8); break;
        default: return hipErrorInvalidValue;
    }
#undef ENC_EMB
    return hipGetLastError();
}

template <int DT, bool SLABS = false>
static hipError_t launch_add_ln_pool(const void* y, const void* bias, const void* res, const void* gamma, const void* beta, float eps, int b, int l,
                                     int d, const int* lens, int normalize, float* partial, float* out, hipStream_t s, int n_split = 0) {
    const int d8 = d / 8, vpl16 = (d8 + 15) / 16;
    const dim3 grid((unsigned)(l / 16), (unsigned)b), block(256);
    // (SLABS: y is the fp32 slab array, not a 16-bit tensor)
#define ENC_LNP(V)                                                                                                                        \
    hipLaunchKernelGGL((add_ln16_pool_kernel<DT, V, SLABS>), grid, block, 0, s, reinterpret_cast<const typename EncVec<DT>::V8*>(SLABS ? nullptr : y), reinterpret_cast<const typename EncVec<DT>::V8*>(bias), \
                       reinterpret_cast<const typename EncVec<DT>::V8*>(res), reinterpret_cast<const typename EncVec<DT>::V8*>(gamma), reinterpret_cast<const typename EncVec<DT>::V8*>(beta), eps, l, \
                       d8, lens, partial, reinterpret_cast<const float4*>(SLABS ? y : nullptr), n_split, (long long)b * l * d8 * 2)
    switch (vpl16) {
        case 1: ENC_LNP(1); break;
        case 2: ENC_LNP(2); break;
        case 3: case 4: ENC_LNP(4); break;
        case 5: case 6: ENC_LNP(6); break;
        case 7: case 8: ENC_LNP(8); break;
        case 9: case 10: case 11: case 12: ENC_LNP(12); break;
        case 13: case 14: case 15: case 16: ENC_LNP(16); break;
        default: return hipErrorInvalidValue;
    }
#undef ENC_LNP
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pool_finish_kernel, dim3((unsigned)b), dim3(256), 0, s, partial, lens, l / 16, d, normalize, out);
    return hipGetLastError();
}

// LayerNorm(y + bias + residual) of a [b, l, d] mini-batch folded into the masked mean-pool + L2-normalise of its rows:
// l % 16 == 0, d % 8 == 0, d <= 2048, 16-byte aligned buffers; partial: b * (l / 16) * d floats of scratch
hipError_t cmr_launch_add_layernorm_pool(const void* y, const void* bias, const void* res, const void* gamma, const void* beta, float eps, int b, int l,
                                         int d, int dtype, const int* lens, int normalize, float* partial, float* out, hipStream_t s) {
    if (dtype == CMR_DT_BF16) return launch_add_ln_pool<CMR_DT_BF16>(y, bias, res, gamma, beta, eps, b, l, d, lens, normalize, partial, out, s);
    if (dtype == CMR_DT_F32) return launch_add_ln_pool<CMR_DT_F32>(y, bias, res, gamma, beta, eps, b, l, d, lens, normalize, partial, out, s);
    return launch_add_ln_pool<CMR_DT_F16>(y, bias, res, gamma, beta, eps, b, l, d, lens, normalize, partial, out, s);
}

// the same with y given as the n_split fp32 slabs [n_split, b*l, d] of the small-M linear's partials form (16-bit dtypes)
hipError_t cmr_launch_add_layernorm_partials_pool(const float* slabs, int n_split, const void* bias, const void* res, const void* gamma, const void* beta, float eps, int b,
                                                  int l, int d, int dtype, const int* lens, int normalize, float* partial, float* out, hipStream_t s) {
    if (dtype == CMR_DT_BF16) return launch_add_ln_pool<CMR_DT_BF16, true>(slabs, bias, res, gamma, beta, eps, b, l, d, lens, normalize, partial, out, s, n_split);
    return launch_add_ln_pool<CMR_DT_F16, true>(slabs, bias, res, gamma, beta, eps, b, l, d, lens, normalize, partial, out, s, n_split);
}

hipError_t cmr_launch_embed_layernorm(const long long* ids, const long long* tt, const void* word, const void* pos, const void* type,
                                      const void* gamma, const void* beta, float eps, long long rows, int L, int d, int vocab, int n_pos,
                                      int n_types, int pos_off, int dtype, void* out, hipStream_t s) {
    if (dtype == CMR_DT_BF16) return launch_embed_ln<CMR_DT_BF16>(ids, tt, word, pos, type, gamma, beta, eps, rows, L, d, vocab, n_pos, n_types, pos_off, out, s);
    if (dtype == CMR_DT_F32) return launch_embed_ln<CMR_DT_F32>(ids, tt, word, pos, type, gamma, beta, eps, rows, L, d, vocab, n_pos, n_types, pos_off, out, s);
    return launch_embed_ln<CMR_DT_F16>(ids, tt, word, pos, type, gamma, beta, eps, rows, L, d, vocab, n_pos, n_types, pos_off, out, s);
}

hipError_t cmr_launch_add_layernorm(const void* y, const void* bias, const void* res, const void* gamma, const void* beta, float eps, long long rows,
                                    int d, int dtype, void* out, hipStream_t s) {
    if (dtype == CMR_DT_BF16) return launch_add_ln<CMR_DT_BF16>(y, bias, res, gamma, beta, eps, rows, d, out, s);
    if (dtype == CMR_DT_F32) return launch_add_ln<CMR_DT_F32>(y, bias, res, gamma, beta, eps, rows, d, out, s);
    return launch_add_ln<CMR_DT_F16>(y, bias, res, gamma, beta, eps, rows, d, out, s);
}

// ------------------------------------------------------------------------------------------------ small-M linear
// y[M, N] = act(x[M, K] w[N, K]^T + bias) for the 1 .. 128 token rows of one short query (`self.embedding_model(**inputs)`,
// embedding_model/BGEEmbedding.py:119, the four nn.Linear of a BertLayer): all latency, and the weight is the only large operand, so the
// kernel is a weight stream.  A workgroup owns ONE 16-row tile of w (the A operand of v_mfma_f32_16x16x32: lane l = weight row l & 15,
// k = 8 (l >> 4) + [0, 8) of a k-step — a 16-byte load straight from nn.Linear's row-major tensor) and one K slice; the token rows are
// the MFMA's N dimension, 16 per tile, up to eight accumulator tiles per wave.  The grid is N / 16 tiles x S slices: every weight byte
// is read by exactly one lane of the grid, once.  Inside a workgroup the slice's k-steps go round the four waves (step j of an
// eight-step chunk -> wave j & 3) and each wave issues ALL the weight loads of a 32-step batch — up to eight 16-byte non-temporal loads
// per lane — before its first MFMA.  The slice's token tile goes through LDS in chunks of SML_KC columns: every thread brings 16-byte
// pieces of whole rows (coalesced, once per workgroup), the next chunk's pieces are in flight in registers while this one is multiplied,
// and the waves read their B fragments from LDS (rows SML_XSTR apart: the sixteen rows of a ds_read_b128 start in sixteen different
// 16-byte slots).  The four waves' partial tiles are added in wave order through LDS (the token buffer, reused).
//   MODE 0 / 1 (direct, S = 1): + bias in fp32, rounded to the 16-bit type as the GEMM's output would have been; MODE 1 then applies the
//     exact erf GELU to the ROUNDED value and rounds again — F.gelu(F.linear(x, w, b)) in one launch.
//   MODE 2 (partials): the slice's fp32 sums go to slab blockIdx.y of out[S, M, N] with plain 16-byte vector stores, no bias, no
//     rounding; the consumer launch (add_ln_partials_kernel) adds the slabs in slab order.  No workgroup waits on another one.
// S, the tile and the order of every sum depend on (N, K) only: a token row's bits do not depend on M or on the other rows.
#define SML_ROWS 16           // weight rows per workgroup
#define SML_MAXM 128          // token rows
#define SML_KC 256            // columns of the token tile per LDS chunk: eight k-steps of 32, two per wave
#define SML_XSTR (SML_KC + 8) // LDS row stride, elements (528 B = 33 slots of 16 B)
#define SML_TARGET_WG 192     // workgroups the split aims at (256 CUs; the round-6 kernel's 24 .. 96 were too few requests in flight)
typedef __attribute__((ext_vector_type(4))) float enc_f32x4;

template <int DT> __device__ __forceinline__ enc_f32x4 sml_mma(v4u a, v4u b, enc_f32x4 c) {
    if constexpr (DT == CMR_DT_BF16) return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// K slices of the partials form: the smallest divisor s of the K / 32 k-steps that puts N / 16 * s >= SML_TARGET_WG workgroups on the
// chip while a slice keeps at least four k-steps (one per wave); the largest such divisor if none reaches the target.
static int sml_split(int n, int k) {
    const int tiles = n / SML_ROWS, steps = k / 32;
    int best = 1;
    for (int s = 1; s <= steps / 4; ++s) {
        if (steps % s) continue;
        best = s;
        if (tiles * s >= SML_TARGET_WG) break;
    }
    return best;
}

// MT = token tiles of 16 rows the instantiation carries (2, 4, 6, 8: M <= 32, 64, 96, 128): it sizes the accumulators, the staging registers and
// the LDS buffer, never the order of a sum.  No branch in the loads or the MFMA loops: token rows >= M re-read row M - 1 (their columns of
// the product are never stored), k-steps behind the slice's end load the slice's last step and multiply a ZERO weight fragment (+ 0.0f).
// TILED (the many-row form, cmr_encoder_linear_rows*): the workgroup's token rows are the 128 from blockIdx.z * 128 on (MT = 8); the row clamp
// and the slab index take the global row and the total M, everything else is the same code: the same sums in the same order for every row.
template <int DT, int MODE, int MT, bool TILED = false>
__global__ __launch_bounds__(256) void small_linear_kernel(const unsigned short* __restrict__ x, const unsigned short* __restrict__ w, const unsigned short* __restrict__ bias,
                                                           int M, int N, int K, int kslice, void* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned short xs[MT * 16 * SML_XSTR];      // 8.25 KiB per token tile; the wave-order reduction reuses it (4 KiB per tile)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * SML_ROWS, k0 = blockIdx.y * kslice;
    const int m0 = TILED ? (int)blockIdx.z * SML_MAXM : 0;     // first token row of this workgroup
    const int nsteps = kslice / 32, nchunks = (nsteps + 7) / 8;
    const unsigned short* wrow = w + (size_t)(n0 + r) * K + k0 + 8 * q;

    // token-tile staging: thread -> 16-byte piece xseg of rows xrow + 8 i
    const int xseg = tid & 31, xrow = tid >> 5;
    const unsigned short* xp[2 * MT];
#pragma unroll
    for (int i = 0; i < 2 * MT; ++i) {
        const int row = m0 + xrow + 8 * i;
        xp[i] = x + (size_t)(row < M ? row : M - 1) * K + k0;
    }
    v4u xr[2 * MT];
    auto load_x = [&](int c) {
        int kk = c * SML_KC + 8 * xseg;
        kk = kk < kslice ? kk : kslice - 8;
#pragma unroll
        for (int i = 0; i < 2 * MT; ++i) xr[i] = *reinterpret_cast<const v4u*>(xp[i] + kk);
    };
    auto store_x = [&]() {
#pragma unroll
        for (int i = 0; i < 2 * MT; ++i) *reinterpret_cast<v4u*>(&xs[(xrow + 8 * i) * SML_XSTR + 8 * xseg]) = xr[i];
    };

    enc_f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = enc_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    load_x(0);
    for (int sb = 0; sb < nchunks; sb += 4) {          // a batch: four chunks = 32 k-steps, eight per wave
        v4u wr[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {                  // the wave's k-steps of the batch, all in flight before the first MFMA
            const int step = (sb + (i >> 1)) * 8 + 4 * (i & 1) + wave;
            const v4u t = __builtin_nontemporal_load(reinterpret_cast<const v4u*>(wrow + (step < nsteps ? step : nsteps - 1) * 32));
            wr[i] = step < nsteps ? t : v4u{0, 0, 0, 0};
        }
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const int c = sb + cc;
            if (c < nchunks) {                         // (workgroup-uniform: every thread meets the same barriers)
                store_x();
                __syncthreads();
                if (c + 1 < nchunks) load_x(c + 1);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const unsigned short* xb = &xs[r * SML_XSTR + (4 * j + wave) * 32 + 8 * q];
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
                        acc[mt] = sml_mma<DT>(wr[2 * cc + j], *reinterpret_cast<const v4u*>(xb + mt * 16 * SML_XSTR), acc[mt]);
                }
                __syncthreads();                       // everybody has read this chunk: the next one (or the reduction) may overwrite it
            }
        }
    }

    // the four waves' tiles added in wave order; C/D layout of the 16x16 MFMA: lane -> token l & 15, weight rows 4 (l >> 4) + [0, 4)
    float* red = reinterpret_cast<float*>(xs);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<enc_f32x4*>(&red[((wave * MT + mt) * 64 + lane) * 4]) = acc[mt];
    __syncthreads();
#pragma unroll
    for (int it = 0; it < MT / 4 + (MT % 4 ? 1 : 0); ++it) {
        const int item = tid + 256 * it, mt = item >> 6, ln = item & 63;
        const int m = m0 + mt * 16 + (ln & 15), n = n0 + 4 * (ln >> 4);
        if (mt >= MT || m >= M) continue;
        enc_f32x4 s = *reinterpret_cast<const enc_f32x4*>(&red[(mt * 64 + ln) * 4]);
#pragma unroll
        for (int wv = 1; wv < 4; ++wv) s += *reinterpret_cast<const enc_f32x4*>(&red[((wv * MT + mt) * 64 + ln) * 4]);
        if constexpr (MODE == 2) {
            *reinterpret_cast<enc_f32x4*>(reinterpret_cast<float*>(out) + ((size_t)blockIdx.y * M + m) * N + n) = s;
        } else {
            float v[4] = {s[0], s[1], s[2], s[3]};
            if (bias) enc_acc4<DT>(v, *reinterpret_cast<const uint2*>(bias + n));
            uint2 o = enc_put4<DT>(v[0], v[1], v[2], v[3]);
            if constexpr (MODE == 1) {                 // the model's erf GELU on the rounded pre-activation, as F.gelu sees it
                enc_get4<DT>(v, o);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
                o = enc_put4<DT>(v[0], v[1], v[2], v[3]);
            }
            *reinterpret_cast<uint2*>(reinterpret_cast<unsigned short*>(out) + (size_t)m * N + n) = o;
        }
    }
}

template <int DT, int MODE>
static hipError_t launch_small_linear(const void* x, const void* w, const void* bias, int m, int n, int k, int split, void* out, hipStream_t s) {
    const dim3 grid((unsigned)(n / SML_ROWS), (unsigned)split), block(256);
#define ENC_SML(T)                                                                                                                     \
    hipLaunchKernelGGL((small_linear_kernel<DT, MODE, T>), grid, block, 0, s, reinterpret_cast<const unsigned short*>(x), reinterpret_cast<const unsigned short*>(w), \
                       reinterpret_cast<const unsigned short*>(bias), m, n, k, k / split, out)
    if (m <= 32) ENC_SML(2);
    else if (m <= 64) ENC_SML(4);
    else if (m <= 96) ENC_SML(6);
    else if (m <= SML_MAXM) ENC_SML(8);
    else {                                             // the many-row form: ceil(m / 128) row tiles over the grid's third dimension
        const dim3 tiled((unsigned)(n / SML_ROWS), (unsigned)split, (unsigned)((m + SML_MAXM - 1) / SML_MAXM));
        hipLaunchKernelGGL((small_linear_kernel<DT, MODE, 8, true>), tiled, block, 0, s, reinterpret_cast<const unsigned short*>(x), reinterpret_cast<const unsigned short*>(w),
                           reinterpret_cast<const unsigned short*>(bias), m, n, k, k / split, out);
    }
#undef ENC_SML
    return hipGetLastError();
}

int cmr_small_linear_split(int n, int k) { return sml_split(n, k); }

// mode 0: F.linear; 1: F.gelu(F.linear); 2: fp32 partial slabs [cmr_small_linear_split(n, k), m, n] (bias unused).  16-bit dtypes, 1 <= m <= 128
// for cmr_encoder_linear_small*, <= CMR_ENCODER_ROWS_MAX for cmr_encoder_linear_rows* (m > 128: row tiles of 128 over grid.z),
// n % 16 == 0, k % 32 == 0, 16-byte aligned buffers (the caller checks)
hipError_t cmr_launch_small_linear(const void* x, const void* w, const void* bias, int m, int n, int k, int dtype, int mode, void* out, hipStream_t s) {
    const int split = mode == 2 ? sml_split(n, k) : 1;
    if (dtype == CMR_DT_BF16) {
        if (mode == 0) return launch_small_linear<CMR_DT_BF16, 0>(x, w, bias, m, n, k, split, out, s);
        if (mode == 1) return launch_small_linear<CMR_DT_BF16, 1>(x, w, bias, m, n, k, split, out, s);
        return launch_small_linear<CMR_DT_BF16, 2>(x, w, bias, m, n, k, split, out, s);
    }
    if (mode == 0) return launch_small_linear<CMR_DT_F16, 0>(x, w, bias, m, n, k, split, out, s);
    if (mode == 1) return launch_small_linear<CMR_DT_F16, 1>(x, w, bias, m, n, k, split, out, s);
    return launch_small_linear<CMR_DT_F16, 2>(x, w, bias, m, n, k, split, out, s);
}

// LayerNorm(sum over the S slabs of partial[s] + bias + residual): the consumer of small_linear_kernel's partials form.  The slabs
// [S, rows, d] fp32 are added in slab order; from there on it is add_ln_kernel (a wave per row, the shared body enc_ln_store).
template <int DT, int VPL>
__global__ __launch_bounds__(256) void add_ln_partials_kernel(const float4* __restrict__ part, int n_split, const typename EncVec<DT>::V4* __restrict__ bias,
                                                              const typename EncVec<DT>::V4* __restrict__ res, const typename EncVec<DT>::V4* __restrict__ gamma,
                                                              const typename EncVec<DT>::V4* __restrict__ beta, float eps, long long rows, int d4, typename EncVec<DT>::V4* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const long long slab = rows * d4;
    float v[VPL][4];
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < VPL; ++j) v[j][0] = v[j][1] = v[j][2] = v[j][3] = 0.0f;
    // slab order.  Four slabs at a time: their 4 VPL loads per lane are in flight together (80 rows are 80 waves: all latency), then added in order
    int sp = 0;
    for (; sp + 4 <= n_split; sp += 4) {
        const float4* p = part + sp * slab + row * d4;
        float4 t[4][VPL];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int i = j * 64 + lane;
                t[u][j] = p[u * slab + (i < d4 ? i : 0)];
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < VPL; ++j) { v[j][0] += t[u][j].x; v[j][1] += t[u][j].y; v[j][2] += t[u][j].z; v[j][3] += t[u][j].w; }
    }
    for (; sp < n_split; ++sp) {
        const float4* p = part + sp * slab + row * d4;
#pragma unroll
        for (int j = 0; j < VPL; ++j) {
            const int i = j * 64 + lane;
            const float4 t = p[i < d4 ? i : 0];
            v[j][0] += t.x; v[j][1] += t.y; v[j][2] += t.z; v[j][3] += t.w;
        }
    }
#pragma unroll
    for (int j = 0; j < VPL; ++j) {
        const int i = j * 64 + lane;
        if (i < d4) {
            if (bias) enc_acc4<DT>(v[j], bias[i]);
            if (res) enc_acc4<DT>(v[j], res[row * d4 + i]);
            sum += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
        }
    }
    enc_ln_store<DT, VPL>(v, sum, lane, d4, gamma, beta, eps, out + row * d4);
}

template <int DT>
static hipError_t launch_add_ln_partials(const float* part, int n_split, const void* bias, const void* res, const void* gamma, const void* beta, float eps,
                                         long long rows, int d, void* out, hipStream_t s) {
    const int d4 = d / 4, vpl = (d4 + 63) / 64;
    const dim3 grid((unsigned)((rows + 3) / 4)), block(256);
#define ENC_LNS(V)                                                                                                                    \
    hipLaunchKernelGGL((add_ln_partials_kernel<DT, V>), grid, block, 0, s, reinterpret_cast<const float4*>(part), n_split, reinterpret_cast<const typename EncVec<DT>::V4*>(bias), \
                       reinterpret_cast<const typename EncVec<DT>::V4*>(res), reinterpret_cast<const typename EncVec<DT>::V4*>(gamma), reinterpret_cast<const typename EncVec<DT>::V4*>(beta), eps, \
                       rows, d4, reinterpret_cast<typename EncVec<DT>::V4*>(out))
    switch (vpl) {
        case 1: ENC_LNS(1); break;
        case 2: ENC_LNS(2); break;
        case 3: ENC_LNS(3); break;
        case 4: ENC_LNS(4); break;
        case 5: case 6: ENC_LNS(6); break;
        case 7: case 8: ENC_LNS(8); break;
        default: return hipErrorInvalidValue;
    }
#undef ENC_LNS
    return hipGetLastError();
}

hipError_t cmr_launch_add_layernorm_partials(const float* part, int n_split, const void* bias, const void* res, const void* gamma, const void* beta, float eps,
                                             long long rows, int d, int dtype, void* out, hipStream_t s) {
    if (dtype == CMR_DT_BF16) return launch_add_ln_partials<CMR_DT_BF16>(part, n_split, bias, res, gamma, beta, eps, rows, d, out, s);
    return launch_add_ln_partials<CMR_DT_F16>(part, n_split, bias, res, gamma, beta, eps, rows, d, out, s);
}

// ------------------------------------------------------------------------------------------------ cross-encoder tail
// A cross-encoder's head reads token 0 of every sequence only, so the LAST layer needs its attention for ONE query row per (sequence, head):
// a memory-bound read of the head's K and V rows with fp32 arithmetic on the VALU (a one-row query has no use for the matrix pipe).
// attn_cls_kernel: one workgroup of CLS_WAVES waves per (sequence, head).  Wave w takes the 64-key chunks w, w + CLS_WAVES, ...; in a chunk a
// lane owns a key for q.k (16-byte loads of its K row), then the lanes regroup — NSEG lanes per V row, one 16-byte segment each, 64 / NSEG rows per
// pass — and pick their key's weight up by a lane shuffle.  Every wave keeps a running (max, sum, o[HD]) of its chunks; the waves' partials
// meet in LDS and are combined in wave order.  Keys >= len are neither read nor weighted.
// Measured at b = 100, l = 512 (profiles/rerank.json): 31 us (12 heads, bf16), 45 us (12 heads, f16), 49 / 72 us (16 heads), against 140 - 195 us
// of the all-rows kernel; f16 pays its conversions (v_cvt per element, where bf16 is a shift).
#define CLS_WAVES 4
template <int DT> __device__ __forceinline__ void cls_load(const void* p, float (&t)[DT == CMR_DT_F32 ? 4 : 8]) {      // one 16-byte segment, widened
    if constexpr (DT == CMR_DT_F32) {
        const float4 a = *reinterpret_cast<const float4*>(p);
        t[0] = a.x; t[1] = a.y; t[2] = a.z; t[3] = a.w;
    } else {
        enc_get8<DT>(t, *reinterpret_cast<const uint4*>(p));
    }
}
template <int DT> __device__ __forceinline__ float cls_elem(const void* p, int i) {
    if constexpr (DT == CMR_DT_F32) {
        return reinterpret_cast<const float*>(p)[i];
    } else {
        float a, b;
        enc_unpack2<DT>((unsigned)reinterpret_cast<const unsigned short*>(p)[i], a, b);
        return a;
    }
}

template <int DT, int HD>
__global__ __launch_bounds__(CLS_WAVES * 64) void attn_cls_kernel(const void* __restrict__ qkv, const int* __restrict__ lens, int L, int hidden, int n_heads,
                                                                  float sc /* log2(e) / sqrt(HD) */, void* __restrict__ out) {
    constexpr int ES = DT == CMR_DT_F32 ? 4 : 2, SEG = 16 / ES, NSEG = HD / SEG, KPP = 64 / NSEG;       // element bytes; elements, segments of a row; V rows per pass
    __shared__ __attribute__((aligned(16))) float q_lds[HD];
    __shared__ float o_lds[CLS_WAVES][HD];
    __shared__ float m_lds[CLS_WAVES], l_lds[CLS_WAVES];
    const int seq = (int)blockIdx.x / n_heads, head = (int)blockIdx.x % n_heads;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int len = lens[seq];
    len = len < L ? len : L;
    len = len > 1 ? len : 1;                               // (the contract says lens >= 1: token 0 is always read)
    const size_t rs = (size_t)3 * hidden * ES;             // bytes between token rows
    const char* qrow = reinterpret_cast<const char*>(qkv) + (size_t)seq * L * rs + (size_t)head * HD * ES;
    const char* kbase = qrow + (size_t)hidden * ES;
    const char* vbase = qrow + 2 * (size_t)hidden * ES;
    if (tid < NSEG) {
        float t[SEG];
        cls_load<DT>(qrow + tid * 16, t);
#pragma unroll
        for (int i = 0; i < SEG; ++i) q_lds[tid * SEG + i] = t[i];
    }
    __syncthreads();

    const int sg = lane % NSEG, kg = lane / NSEG;
    float o[SEG];
#pragma unroll
    for (int i = 0; i < SEG; ++i) o[i] = 0.0f;
    float m = ATT_NEG, lsum = 0.0f;
    for (int k0 = wave * 64; k0 < len; k0 += CLS_WAVES * 64) {         // (wave-uniform bounds: every lane of the wave runs the shuffles)
        const int key = k0 + lane;
        float s = ATT_NEG;
        if (key < len) {
            const char* kr = kbase + (size_t)key * rs;
            float acc = 0.0f;
#pragma unroll
            for (int g = 0; g < NSEG; ++g) {
                float t[SEG];
                cls_load<DT>(kr + g * 16, t);
                float a = 0.0f;
#pragma unroll
                for (int i = 0; i < SEG; ++i) a = fmaf(t[i], q_lds[g * SEG + i], a);
                acc += a;
            }
            s = acc;
        }
        float cm = s;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cm = fmaxf(cm, __shfl_xor(cm, off));
        const float mn = fmaxf(m, cm);
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * sc);
        const float p = key < len ? __builtin_amdgcn_exp2f((s - mn) * sc) : 0.0f;
        lsum = fmaf(lsum, alpha, p);
        m = mn;
#pragma unroll
        for (int i = 0; i < SEG; ++i) o[i] *= alpha;
#pragma unroll
        for (int ps = 0; ps < NSEG; ++ps) {                // 64 keys = NSEG passes of KPP rows
            const int kk = ps * KPP + kg;
            const float pk = __shfl(p, kk);
            if (k0 + kk < len) {
                float t[SEG];
                cls_load<DT>(vbase + (size_t)(k0 + kk) * rs + sg * 16, t);
#pragma unroll
                for (int i = 0; i < SEG; ++i) o[i] = fmaf(pk, t[i], o[i]);
            }
        }
    }
    // the wave's partial: o summed over the lanes of a segment, the weights over all lanes
#pragma unroll
    for (int off = NSEG; off < 64; off <<= 1)
#pragma unroll
        for (int i = 0; i < SEG; ++i) o[i] += __shfl_xor(o[i], off);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) lsum += __shfl_xor(lsum, off);
    if (kg == 0) {
#pragma unroll
        for (int i = 0; i < SEG; ++i) o_lds[wave][sg * SEG + i] = o[i];
    }
    if (lane == 0) {
        m_lds[wave] = m;
        l_lds[wave] = lsum;
    }
    __syncthreads();
    if (tid < HD / 2) {                                    // two output elements per thread, the waves in wave order
        float mx = m_lds[0];
#pragma unroll
        for (int w = 1; w < CLS_WAVES; ++w) mx = fmaxf(mx, m_lds[w]);
        float a0 = 0.0f, a1 = 0.0f, lt = 0.0f;
#pragma unroll
        for (int w = 0; w < CLS_WAVES; ++w) {
            const float f = __builtin_amdgcn_exp2f((m_lds[w] - mx) * sc);     // a wave without keys: exp2(-huge) = 0 times its zeros
            lt = fmaf(l_lds[w], f, lt);
            a0 = fmaf(o_lds[w][2 * tid], f, a0);
            a1 = fmaf(o_lds[w][2 * tid + 1], f, a1);
        }
        const float inv = 1.0f / lt;
        char* orow = reinterpret_cast<char*>(out) + ((size_t)seq * hidden + (size_t)head * HD) * ES;
        if constexpr (DT == CMR_DT_F32) reinterpret_cast<float2*>(orow)[tid] = make_float2(a0 * inv, a1 * inv);
        else reinterpret_cast<unsigned*>(orow)[tid] = enc_pack2<DT>(a0 * inv, a1 * inv);
    }
}

template <int DT, int HD>
static hipError_t launch_attention_cls(const void* qkv, const int* lens, int b, int L, int n_heads, void* out, hipStream_t s) {
    if ((long long)b * n_heads > (1LL << 30)) return hipErrorInvalidValue;
    hipLaunchKernelGGL((attn_cls_kernel<DT, HD>), dim3((unsigned)(b * n_heads)), dim3(CLS_WAVES * 64), 0, s, qkv, lens, L, n_heads * HD, n_heads, att_scale<HD>(), out);
    return hipGetLastError();
}

hipError_t cmr_launch_attention_cls(const void* qkv, int dtype, const int* lens, int b, int L, int n_heads, int head_dim, void* out, hipStream_t s) {
    if (head_dim != 64 && head_dim != 32) return hipErrorInvalidValue;
#define ENC_CLS(T) (head_dim == 64 ? launch_attention_cls<T, 64>(qkv, lens, b, L, n_heads, out, s) : launch_attention_cls<T, 32>(qkv, lens, b, L, n_heads, out, s))
    if (dtype == CMR_DT_F32) return ENC_CLS(CMR_DT_F32);
    if (dtype == CMR_DT_BF16) return ENC_CLS(CMR_DT_BF16);
    return ENC_CLS(CMR_DT_F16);
#undef ENC_CLS
}

// cls_head_kernel: out[s] = b2 + sum_j w2[j] tanh(b1[j] + w1[j, :] . x[s]) — one workgroup per sequence; its x row sits in LDS as fp32.  A group
// of HEAD_LPR lanes owns a row of w1 (16-byte loads, 256 contiguous bytes per group and instruction; the b workgroups read w1 out of L2): the
// workgroup's 32 groups take rows 32 apart, HEAD_U of them at a time, reduce each dot product over the group's lanes and add w2[j] tanhf(.) to the
// group's running sum in j order.  The 32 sums are added in group order: a row's bits depend on (d, dtype) alone.
// Measured at b = 100 (tools/rerank_bench.py, profiles/rerank.json): 34 - 36 us at d = 768, 53 - 58 us at d = 1024.  The first form — a whole wave
// per row, four rows at a time, 32 dependent load-and-reduce rounds per wave at d = 1024 — took 65 - 67 and 85 - 88 us.  A weight-streaming form
// over all b rows (w1 read once, as the small-M linear kernels do) was not tried: four head launches are about 1 % of a 100-pair call at the base shape and less at the large one.
#define HEAD_WAVES 8
#define HEAD_LPR 16
#define HEAD_U 2
#define HEAD_MAXD 2048
template <int DT>
__global__ __launch_bounds__(HEAD_WAVES * 64) void cls_head_kernel(const void* __restrict__ x, long long x_stride, const void* __restrict__ w1, const void* __restrict__ b1,
                                                                   const void* __restrict__ w2, const void* __restrict__ b2, int d, float* __restrict__ out) {
    constexpr int ES = DT == CMR_DT_F32 ? 4 : 2, SEG = 16 / ES;
    constexpr int GROUPS = 64 / HEAD_LPR, SLOTS = HEAD_WAVES * GROUPS;        // lane groups of a wave; weight rows in flight per workgroup and unroll step
    __shared__ __attribute__((aligned(16))) float x_lds[HEAD_MAXD];
    __shared__ float part[SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nvec = d / SEG;
    const char* xrow = reinterpret_cast<const char*>(x) + (size_t)blockIdx.x * (size_t)x_stride * ES;
    for (int v = tid; v < nvec; v += HEAD_WAVES * 64) {
        float t[SEG];
        cls_load<DT>(xrow + (size_t)v * 16, t);
#pragma unroll
        for (int i = 0; i < SEG; ++i) x_lds[v * SEG + i] = t[i];
    }
    __syncthreads();
    const size_t wrow = (size_t)d * ES;
    const int grp = lane / HEAD_LPR, sub = lane % HEAD_LPR;
    float acc = 0.0f;
    for (int jb = wave * GROUPS; jb < d; jb += SLOTS * HEAD_U) {       // wave-uniform bounds: every lane runs the shuffles
        float dot[HEAD_U];
#pragma unroll
        for (int r = 0; r < HEAD_U; ++r) dot[r] = 0.0f;
#pragma unroll 4
        for (int v = sub; v < nvec; v += HEAD_LPR) {
            float xv[SEG];
#pragma unroll
            for (int i = 0; i < SEG; ++i) xv[i] = x_lds[v * SEG + i];
#pragma unroll
            for (int r = 0; r < HEAD_U; ++r) {
                const int j = jb + grp + SLOTS * r;
                if (j < d) {
                    float t[SEG];
                    cls_load<DT>(reinterpret_cast<const char*>(w1) + (size_t)j * wrow + (size_t)v * 16, t);
#pragma unroll
                    for (int i = 0; i < SEG; ++i) dot[r] = fmaf(t[i], xv[i], dot[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < HEAD_U; ++r) {
#pragma unroll
            for (int off = HEAD_LPR / 2; off > 0; off >>= 1) dot[r] += __shfl_xor(dot[r], off);
            const int j = jb + grp + SLOTS * r;
            if (j < d) acc = fmaf(cls_elem<DT>(w2, j), tanhf(dot[r] + (b1 ? cls_elem<DT>(b1, j) : 0.0f)), acc);
        }
    }
    if (sub == 0) part[wave * GROUPS + grp] = acc;
    __syncthreads();
    if (tid == 0) {
        float t = b2 ? cls_elem<DT>(b2, 0) : 0.0f;
#pragma unroll
        for (int w = 0; w < SLOTS; ++w) t += part[w];
        out[blockIdx.x] = t;
    }
}

hipError_t cmr_launch_cls_head(const void* x, long long x_stride, const void* w1, const void* b1, const void* w2, const void* b2, int b, int d, int dtype,
                               float* out, hipStream_t s) {
    if (d <= 0 || d % 8 || d > HEAD_MAXD) return hipErrorInvalidValue;
#define ENC_HEAD(T) hipLaunchKernelGGL(cls_head_kernel<T>, dim3((unsigned)b), dim3(HEAD_WAVES * 64), 0, s, x, x_stride, w1, b1, w2, b2, d, out)
    if (dtype == CMR_DT_F32) ENC_HEAD(CMR_DT_F32);
    else if (dtype == CMR_DT_BF16) ENC_HEAD(CMR_DT_BF16);
    else ENC_HEAD(CMR_DT_F16);
#undef ENC_HEAD
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------ C-ABI (include/comorag_hip.h)
// argument checks of the encoder entry points; each ends in one launcher call above
extern "C" {

int32_t cmr_encoder_attention(int32_t device_id, const void* qkv_dev, int32_t dtype, const int32_t* lens_dev, int32_t b, int32_t l,
                              int32_t n_heads, int32_t head_dim, void* out_dev, void* stream) {
    if (!qkv_dev || !lens_dev || !out_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (b <= 0 || l <= 0 || n_heads <= 0) return cmr_fail(CMR_ERR_INVALID, "b, l, n_heads must be > 0");
    if (head_dim != 64 && head_dim != 32) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_attention: head_dim must be 64 or 32 (BERT-base / -large heads; bge-small / MiniLM heads)");
    if (dtype != CMR_BF16 && dtype != CMR_F16 && dtype != CMR_F32) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_attention: dtype must be bf16 or f16 or f32");
    if (((uintptr_t)qkv_dev | (uintptr_t)out_dev) & 15) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_attention: buffers must be 16-byte aligned");
    int rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_attention(qkv_dev, dtype, lens_dev, b, l, n_heads, head_dim, out_dev, (hipStream_t)stream));
    return CMR_OK;
}

int32_t cmr_encoder_attention_cls(int32_t device_id, const void* qkv_dev, int32_t dtype, const int32_t* lens_dev, int32_t b, int32_t l,
                                  int32_t n_heads, int32_t head_dim, void* out_dev, void* stream) {
    if (!qkv_dev || !lens_dev || !out_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (b <= 0 || l <= 0 || n_heads <= 0) return cmr_fail(CMR_ERR_INVALID, "b, l, n_heads must be > 0");
    if (head_dim != 64 && head_dim != 32) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_attention_cls: head_dim must be 64 or 32");
    if (dtype != CMR_BF16 && dtype != CMR_F16 && dtype != CMR_F32) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_attention_cls: dtype must be bf16 or f16 or f32");
    if (((uintptr_t)qkv_dev | (uintptr_t)out_dev) & 15) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_attention_cls: buffers must be 16-byte aligned");
    int rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_attention_cls(qkv_dev, dtype, lens_dev, b, l, n_heads, head_dim, out_dev, (hipStream_t)stream));
    return CMR_OK;
}

int32_t cmr_encoder_cls_head(int32_t device_id, const void* x_dev, int64_t x_stride, const void* w1_dev, const void* b1_dev, const void* w2_dev,
                             const void* b2_dev, int32_t b, int32_t d, int32_t dtype, float* out_dev, void* stream) {
    if (!x_dev || !w1_dev || !w2_dev || !out_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (b <= 0 || d <= 0 || x_stride < d) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_cls_head: b, d must be > 0 and x_stride >= d");
    if (dtype != CMR_BF16 && dtype != CMR_F16 && dtype != CMR_F32) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_cls_head: dtype must be bf16 or f16 or f32");
    if (d % 8 || d > HEAD_MAXD) return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_cls_head: d must be a multiple of 8 and <= 2048");
    const int es = dtype == CMR_F32 ? 4 : 2;
    if ((((uintptr_t)x_dev | (uintptr_t)w1_dev) & 15) || (x_stride * es) % 16 || (((uintptr_t)b1_dev | (uintptr_t)w2_dev | (uintptr_t)b2_dev) & (es - 1)) ||
        ((uintptr_t)out_dev & 3))
        return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_cls_head: x and w1 rows must be 16-byte aligned, the vectors element-aligned");
    int rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_cls_head(x_dev, (long long)x_stride, w1_dev, b1_dev, w2_dev, b2_dev, b, d, dtype, out_dev, (hipStream_t)stream));
    return CMR_OK;
}

int32_t cmr_encoder_add_layernorm(int32_t device_id, const void* y_dev, const void* bias_dev, const void* residual_dev, const void* gamma_dev,
                                  const void* beta_dev, float eps, int64_t rows, int32_t d, int32_t dtype, void* out_dev, void* stream) {
    if (!y_dev || !gamma_dev || !beta_dev || !out_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (rows <= 0 || d <= 0 || d % 4 || d > 2048) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_add_layernorm: rows > 0, d a multiple of 4, d <= 2048");
    if (dtype != CMR_BF16 && dtype != CMR_F16 && dtype != CMR_F32) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_add_layernorm: dtype must be bf16 or f16 or f32");
    if (((uintptr_t)y_dev | (uintptr_t)bias_dev | (uintptr_t)residual_dev | (uintptr_t)gamma_dev | (uintptr_t)beta_dev | (uintptr_t)out_dev) & (dtype == CMR_F32 ? 15 : 7))
        return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_add_layernorm: buffers must be 8-byte aligned (16-byte for f32)");
    int rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_add_layernorm(y_dev, bias_dev, residual_dev, gamma_dev, beta_dev, eps, rows, d, dtype, out_dev, (hipStream_t)stream));
    return CMR_OK;
}

int32_t cmr_encoder_add_layernorm_pool(int32_t device_id, const void* y_dev, const void* bias_dev, const void* residual_dev, const void* gamma_dev,
                                       const void* beta_dev, float eps, int32_t b, int32_t l, int32_t d, int32_t dtype, const int32_t* lens_dev,
                                       int32_t normalize, float* partial_dev, float* out_dev, void* stream) {
    if (!y_dev || !gamma_dev || !beta_dev || !lens_dev || !partial_dev || !out_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (b <= 0 || l <= 0 || d <= 0) return cmr_fail(CMR_ERR_INVALID, "b, l, d must be > 0");
    if (l % 16 || d % 8 || d > 2048) return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_add_layernorm_pool: l must be a multiple of 16, d a multiple of 8 and <= 2048");
    if (dtype != CMR_BF16 && dtype != CMR_F16 && dtype != CMR_F32) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_add_layernorm_pool: dtype must be bf16 or f16 or f32");
    if (((uintptr_t)y_dev | (uintptr_t)bias_dev | (uintptr_t)residual_dev | (uintptr_t)gamma_dev | (uintptr_t)beta_dev | (uintptr_t)partial_dev | (uintptr_t)out_dev) & 15)
        return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_add_layernorm_pool: buffers must be 16-byte aligned");
    int rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_add_layernorm_pool(y_dev, bias_dev, residual_dev, gamma_dev, beta_dev, eps, b, l, d, dtype, (const int*)lens_dev, normalize, partial_dev,
                                          out_dev, (hipStream_t)stream));
    return CMR_OK;
}

// shape / type checks shared by the small-M entry points (no device call)
static int sml_check(const char* who, int32_t m, int32_t n, int32_t k, int32_t dtype, int32_t max_m = SML_MAXM) {
    if (m <= 0 || n <= 0 || k <= 0) return cmr_fail(CMR_ERR_INVALID, "%s: m, n, k must be > 0", who);
    if (dtype != CMR_BF16 && dtype != CMR_F16 && dtype != CMR_F32) return cmr_fail(CMR_ERR_INVALID, "%s: dtype must be bf16 or f16", who);
    if (dtype == CMR_F32) return cmr_fail(CMR_ERR_UNSUPPORTED, "%s: 16-bit tensors only (bf16 or f16)", who);
    if (m > max_m) return cmr_fail(CMR_ERR_UNSUPPORTED, "%s: at most %d token rows", who, max_m);
    if (n % SML_ROWS || k % 32) return cmr_fail(CMR_ERR_UNSUPPORTED, "%s: n must be a multiple of 16 and k a multiple of 32", who);
    return CMR_OK;
}

int32_t cmr_encoder_linear_small_split(int32_t m, int32_t n, int32_t k, int32_t dtype, int32_t* n_split, int64_t* slab_bytes) {
    if (!n_split || !slab_bytes) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    int rc = sml_check("cmr_encoder_linear_small_split", m, n, k, dtype);
    if (rc) return rc;
    *n_split = cmr_small_linear_split(n, k);
    *slab_bytes = (int64_t)*n_split * m * n * (int64_t)sizeof(float);
    return CMR_OK;
}

int32_t cmr_encoder_linear_small(int32_t device_id, const void* x_dev, const void* w_dev, const void* bias_dev, int32_t m, int32_t n, int32_t k, int32_t dtype,
                                 int32_t act, void* out_dev, void* stream) {
    if (!x_dev || !w_dev || !out_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (act != 0 && act != 1) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_linear_small: act must be 0 (none) or 1 (erf GELU)");
    int rc = sml_check("cmr_encoder_linear_small", m, n, k, dtype);
    if (rc) return rc;
    if (((uintptr_t)x_dev | (uintptr_t)w_dev | (uintptr_t)bias_dev | (uintptr_t)out_dev) & 15)
        return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_linear_small: buffers must be 16-byte aligned");
    rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_small_linear(x_dev, w_dev, bias_dev, m, n, k, dtype, act, out_dev, (hipStream_t)stream));
    return CMR_OK;
}

int32_t cmr_encoder_linear_small_partials(int32_t device_id, const void* x_dev, const void* w_dev, int32_t m, int32_t n, int32_t k, int32_t dtype,
                                          float* partials_dev, void* stream) {
    if (!x_dev || !w_dev || !partials_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    int rc = sml_check("cmr_encoder_linear_small_partials", m, n, k, dtype);
    if (rc) return rc;
    if (((uintptr_t)x_dev | (uintptr_t)w_dev | (uintptr_t)partials_dev) & 15)
        return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_linear_small_partials: buffers must be 16-byte aligned");
    rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_small_linear(x_dev, w_dev, nullptr, m, n, k, dtype, 2, partials_dev, (hipStream_t)stream));
    return CMR_OK;
}

// the many-row forms: the same launcher; m > 128 takes the row-tiled instantiation (a row's bits are those of cmr_encoder_linear_small*)
int32_t cmr_encoder_linear_rows(int32_t device_id, const void* x_dev, const void* w_dev, const void* bias_dev, int32_t m, int32_t n, int32_t k, int32_t dtype,
                                int32_t act, void* out_dev, void* stream) {
    if (!x_dev || !w_dev || !out_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (act != 0 && act != 1) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_linear_rows: act must be 0 (none) or 1 (erf GELU)");
    int rc = sml_check("cmr_encoder_linear_rows", m, n, k, dtype, CMR_ENCODER_ROWS_MAX);
    if (rc) return rc;
    if (((uintptr_t)x_dev | (uintptr_t)w_dev | (uintptr_t)bias_dev | (uintptr_t)out_dev) & 15)
        return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_linear_rows: buffers must be 16-byte aligned");
    rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_small_linear(x_dev, w_dev, bias_dev, m, n, k, dtype, act, out_dev, (hipStream_t)stream));
    return CMR_OK;
}

int32_t cmr_encoder_linear_rows_partials(int32_t device_id, const void* x_dev, const void* w_dev, int32_t m, int32_t n, int32_t k, int32_t dtype,
                                         float* partials_dev, void* stream) {
    if (!x_dev || !w_dev || !partials_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    int rc = sml_check("cmr_encoder_linear_rows_partials", m, n, k, dtype, CMR_ENCODER_ROWS_MAX);
    if (rc) return rc;
    if (((uintptr_t)x_dev | (uintptr_t)w_dev | (uintptr_t)partials_dev) & 15)
        return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_linear_rows_partials: buffers must be 16-byte aligned");
    rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_small_linear(x_dev, w_dev, nullptr, m, n, k, dtype, 2, partials_dev, (hipStream_t)stream));
    return CMR_OK;
}

int32_t cmr_encoder_add_layernorm_partials(int32_t device_id, const float* partials_dev, int32_t n_split, const void* bias_dev, const void* residual_dev,
                                           const void* gamma_dev, const void* beta_dev, float eps, int64_t rows, int32_t d, int32_t dtype, void* out_dev, void* stream) {
    if (!partials_dev || !gamma_dev || !beta_dev || !out_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (rows <= 0 || n_split <= 0 || d <= 0 || d % 4 || d > 2048)
        return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_add_layernorm_partials: rows, n_split > 0, d a multiple of 4, d <= 2048");
    if (dtype != CMR_BF16 && dtype != CMR_F16 && dtype != CMR_F32) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_add_layernorm_partials: dtype must be bf16 or f16");
    if (dtype == CMR_F32) return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_add_layernorm_partials: 16-bit tensors only (bf16 or f16)");
    if (((uintptr_t)partials_dev & 15) || (((uintptr_t)bias_dev | (uintptr_t)residual_dev | (uintptr_t)gamma_dev | (uintptr_t)beta_dev | (uintptr_t)out_dev) & 7))
        return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_add_layernorm_partials: the slabs must be 16-byte aligned, the 16-bit buffers 8-byte aligned");
    int rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_add_layernorm_partials(partials_dev, n_split, bias_dev, residual_dev, gamma_dev, beta_dev, eps, rows, d, dtype, out_dev, (hipStream_t)stream));
    return CMR_OK;
}

int32_t cmr_encoder_add_layernorm_partials_pool(int32_t device_id, const float* partials_dev, int32_t n_split, const void* bias_dev, const void* residual_dev,
                                                const void* gamma_dev, const void* beta_dev, float eps, int32_t b, int32_t l, int32_t d, int32_t dtype,
                                                const int32_t* lens_dev, int32_t normalize, float* pool_partial_dev, float* out_dev, void* stream) {
    if (!partials_dev || !gamma_dev || !beta_dev || !lens_dev || !pool_partial_dev || !out_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (b <= 0 || l <= 0 || d <= 0 || n_split <= 0) return cmr_fail(CMR_ERR_INVALID, "b, l, d, n_split must be > 0");
    if (dtype != CMR_BF16 && dtype != CMR_F16 && dtype != CMR_F32) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_add_layernorm_partials_pool: dtype must be bf16 or f16");
    if (dtype == CMR_F32) return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_add_layernorm_partials_pool: 16-bit tensors only (bf16 or f16)");
    if (l % 16 || d % 8 || d > 2048) return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_add_layernorm_partials_pool: l must be a multiple of 16, d a multiple of 8 and <= 2048");
    if (((uintptr_t)partials_dev | (uintptr_t)bias_dev | (uintptr_t)residual_dev | (uintptr_t)gamma_dev | (uintptr_t)beta_dev | (uintptr_t)pool_partial_dev | (uintptr_t)out_dev) & 15)
        return cmr_fail(CMR_ERR_UNSUPPORTED, "cmr_encoder_add_layernorm_partials_pool: buffers must be 16-byte aligned");
    int rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_add_layernorm_partials_pool(partials_dev, n_split, bias_dev, residual_dev, gamma_dev, beta_dev, eps, b, l, d, dtype, (const int*)lens_dev, normalize,
                                                   pool_partial_dev, out_dev, (hipStream_t)stream));
    return CMR_OK;
}

int32_t cmr_encoder_embed_layernorm(int32_t device_id, const int64_t* ids_dev, const int64_t* token_type_dev, const void* word_dev, const void* pos_dev,
                                    const void* type_dev, const void* gamma_dev, const void* beta_dev, float eps, int64_t rows, int32_t l, int32_t d,
                                    int32_t vocab, int32_t n_positions, int32_t n_types, int32_t position_offset, int32_t dtype, void* out_dev, void* stream) {
    if (!ids_dev || !word_dev || !pos_dev || !type_dev || !gamma_dev || !beta_dev || !out_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (rows <= 0 || l <= 0 || d <= 0 || d % 4 || d > 2048) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_embed_layernorm: rows, l > 0, d a multiple of 4, d <= 2048");
    if (vocab <= 0 || n_positions <= 0 || n_types <= 0 || position_offset < 0) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_embed_layernorm: empty embedding table / negative position offset");
    if (dtype != CMR_BF16 && dtype != CMR_F16 && dtype != CMR_F32) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_embed_layernorm: dtype must be bf16 or f16 or f32");
    if (((uintptr_t)word_dev | (uintptr_t)pos_dev | (uintptr_t)type_dev | (uintptr_t)gamma_dev | (uintptr_t)beta_dev | (uintptr_t)out_dev) & (dtype == CMR_F32 ? 15 : 7))
        return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_embed_layernorm: buffers must be 8-byte aligned (16-byte for f32)");
    int rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_embed_layernorm((const long long*)ids_dev, (const long long*)token_type_dev, word_dev, pos_dev, type_dev, gamma_dev, beta_dev, eps,
                                       rows, l, d, vocab, n_positions, n_types, position_offset, dtype, out_dev, (hipStream_t)stream));
    return CMR_OK;
}

int32_t cmr_encoder_embed_layernorm_ragged(int32_t device_id, const int32_t* ids32_dev, const int32_t* offsets_dev, const void* word_dev, const void* pos_dev,
                                           const void* type_dev, const void* gamma_dev, const void* beta_dev, float eps, int32_t b, int32_t l, int32_t d,
                                           int32_t vocab, int32_t n_positions, int32_t position_offset, int32_t dtype, void* out_dev, void* stream) {
    if (!ids32_dev || !offsets_dev || !word_dev || !pos_dev || !type_dev || !gamma_dev || !beta_dev || !out_dev) return cmr_fail(CMR_ERR_INVALID, "NULL argument");
    if (b <= 0 || l <= 0 || d <= 0 || d % 4 || d > 2048) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_embed_layernorm_ragged: b, l > 0, d a multiple of 4, d <= 2048");
    if (vocab <= 0 || n_positions <= 0 || position_offset < 0) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_embed_layernorm_ragged: empty embedding table / negative position offset");
    if (dtype != CMR_BF16 && dtype != CMR_F16 && dtype != CMR_F32) return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_embed_layernorm_ragged: dtype must be bf16 or f16 or f32");
    if (((uintptr_t)word_dev | (uintptr_t)pos_dev | (uintptr_t)type_dev | (uintptr_t)gamma_dev | (uintptr_t)beta_dev | (uintptr_t)out_dev) & (dtype == CMR_F32 ? 15 : 7))
        return cmr_fail(CMR_ERR_INVALID, "cmr_encoder_embed_layernorm_ragged: buffers must be 8-byte aligned (16-byte for f32)");
    int rc = cmr_check_device(device_id);
    if (rc) return rc;
    rc = cmr_set_device(device_id);
    if (rc) return rc;
    HIP_TRY(cmr_launch_embed_layernorm_ragged((const int*)ids32_dev, (const int*)offsets_dev, word_dev, pos_dev, type_dev, gamma_dev, beta_dev, eps, (long long)b * l, l,
                                              d, vocab, n_positions, position_offset, dtype, out_dev, (hipStream_t)stream));
    return CMR_OK;
}

}  // extern "C"
