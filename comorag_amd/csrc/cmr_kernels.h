// Host-callable launchers of the gfx950 kernels (defined in scan_kernels.hip / aux_kernels.hip / sort_kernels.hip).
// All launchers enqueue on `stream` and return the hipError_t of the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

typedef unsigned long long u64;

struct CmrScanGeom {
    int dtype;      // CMR_DT_*
    int dpad;       // padded dim (multiple of 128)
    int ks;         // 1-KiB blocks per panel  (dpad/16 for 16-bit, dpad/8 for fp32)
    int nqt;        // query tiles of 32 per pass (1 or 2)
    int cap;        // per-(wave,query) candidate list capacity (128 or 256)
    int ring;       // register ring depth (8 or 16), ks % ring == 0
    int grid;       // workgroups
    int asm_ring;   // 1: hand-counted inline-asm load ring, 0: compiler-counted loads
    size_t lds;     // dynamic LDS bytes
    int stream_default_policy;   // narrow top-k kernel: 1 = corpus loads with the default cache policy instead of non-temporal (query-split grid)
};

// max query tiles (1/2/0=unsupported) whose fragments fit LDS for this dtype/dpad
int cmr_scan_max_nqt(int dtype, int dpad);
// fills ks/lds for (dtype,dpad,nqt,cap); returns false if it does not fit
bool cmr_scan_geom(CmrScanGeom* g);

struct CmrScanArgs {
    const void* corpus;   // panel-major blocks
    const void* qfrag;    // [nqt][ks][64] uint4
    long long nrows;
    int npanels;
    int k;
    // top-k mode
    u64* lists;           // [W][nqt*32][cap]
    int* cnt;             // [W][nqt*32]
    float2* mm;           // [W][nqt*32]  (min,max)
    // scores mode
    float* scores;        // [nq][ld]
    long long ld;
    int nq;
    // sampling pass (top-k mode): sample_waves panels in chunks of 2^sample_chunk_log2 consecutive panels, chunk starts
    // sample_stride panels apart: sampled panel s is panel (s >> c) * sample_stride + (s & (2^c - 1)).  Narrow kernel:
    // wave w < sample_waves scans sampled panel w only; wide kernel: the grid's workgroups split the sampled panels.
    int sample_waves;
    int sample_stride;
    int sample_chunk_log2;
    const u64* tau_init;  // [nqt*32] initial threshold keys or nullptr
    // narrow kernel, <= 8 queries, k <= 64: the main pass derives its thresholds ITSELF from the lists of a preceding sampling
    // pass (sample_W lists of the same [W][32][cap] layout) instead of a merge launch between the two scans
    const u64* sample_lists;
    const int* sample_cnt;
    int sample_W;
    // narrow kernel, query-split grid: qgroups x (geom.grid) workgroups, group g scans the whole corpus for queries
    // g*nqt*32 ..; qfrag holds qgroups*nqt tiles, lists / cnt / mm are [qgroups][W][nqt*32](..), tau_init [qgroups][nqt*32]
    int qgroups;
    // narrow kernel with the finishing stage (cmr_launch_scan_fin): control words (CMR_FIN_CTL ints, zeroed once — the kernel re-arms
    // them), first-panel maxima [32][fin_ns], thresholds [32], dense candidate lists [32][fin_dcap], and the search's outputs
    int* fin;
    u64* fin_pmax;
    u64* fin_tau;
    u64* fin_dense;
    u64* fin_mm;          // [32][grid] scratch
    int fin_wgs;          // workgroups (the first to be through their first panels) whose waves' first panels supply the thresholds: 8 x fin_wgs <= CMR_FIN_SLOTS maxima
    int fin_first;        // workgroups of the first round (resident from the start: they cannot find thresholds when they begin); >= fin_wgs
    int fin_mul;          // workgroup b scans the panel ranges of virtual workgroup (b x fin_mul) mod grid (coprime with the grid; 1 = identity)
    int fin_dcap;
    int fin_spin;         // rounds (~1.5 us each) the other workgroups give the suppliers before they start without thresholds
    int64_t* out_ids;
    float* out_scores;
    float* out_min;
    float* out_max;
    long long id_base;
    // a word in pinned, device-mapped host memory (or nullptr) that the launch's LAST store sets once the results are written: 1 = final,
    // 2 = a list overflowed (the merge launch is still due).  The synchronous host API polls it instead of waiting for the end-of-kernel
    // signal (5.5 us per call on MI355X: tools/probe/poll_probe.hip) and launches the merge only in state 2.
    int* fin_done;
    // filtered scan (cmr_launch_scan_masked): one allow word per 32-row panel, [npanels] on the device — bit (r & 31) of word
    // (r >> 5) keeps local row r; bits beyond nrows are ignored.  Main pass and sampling passes take the same words.
    const unsigned* row_mask;
    // per-query filtered scan (cmr_launch_scan_masked_each): row_mask is [nq][row_mask_stride] — query i's words start at
    // row_mask + i * row_mask_stride (words; >= npanels), each block laid out as above.  Queries at or beyond nq have no words.
    long long row_mask_stride;
};
// control words (ints) — every counter on a 128-byte line of its own: device atomics on one line serialise
#define CMR_FIN_DONE 0        // workgroups whose waves have all published their first-panel maxima
#define CMR_FIN_READY 32      // bit q: the threshold of query q is published; bit 31: every first-panel maximum is
#define CMR_FIN_WGS 64        // workgroups finished
#define CMR_FIN_STATE 96      // result state: 1 = the scan wrote the final results itself, 2 = a list overflowed (the merge launch decides)
#define CMR_FIN_OVER 128      // some workgroup's staging area overflowed
#define CMR_FIN_PUB 160       // supplying workgroups whose maxima are written through
#define CMR_FIN_CLAIM 192     // queries whose threshold somebody has taken on
#define CMR_FIN_MAX_QUERIES 16
#define CMR_FIN_DCNT(q) (224 + 32 * (q))     // dense list lengths
#define CMR_FIN_CTL (224 + 32 * 32)
#define CMR_FIN_LDS 4096      // bytes of LDS the finishing stage adds to the geometry's (the waves' min / max and first-panel maxima)
#define CMR_FIN_SLOTS 1024    // first-panel maxima the thresholds are taken from (one selection chunk of a wave)

hipError_t cmr_launch_scan_topk(const CmrScanGeom& g, const CmrScanArgs& a, hipStream_t s);
hipError_t cmr_launch_scan_scores(const CmrScanGeom& g, const CmrScanArgs& a, hipStream_t s);
// cmr_launch_scan_topk among the rows a.row_mask keeps (geom.asm_ring is ignored: the compiler-counted ring)
hipError_t cmr_launch_scan_masked(const CmrScanGeom& g, const CmrScanArgs& a, hipStream_t s);
// the same with allow words of its own for every query of the pass (a.row_mask [a.nq][a.row_mask_stride])
hipError_t cmr_launch_scan_masked_each(const CmrScanGeom& g, const CmrScanArgs& a, hipStream_t s);
// top-k scan of <= 32 queries (k <= 64) that also derives its thresholds (no sampling launch) and selects the final k best per
// query (no merge launch); a.fin[CMR_FIN_STATE] tells the merge launch behind it whether anything is left to do
hipError_t cmr_launch_scan_fin(const CmrScanGeom& g, const CmrScanArgs& a, hipStream_t s);
// wide-batch (register-resident queries) top-k scan: 4 waves x 2 (768-d) or 1 (1024-d) tiles of 32 queries;
// in sampling mode (sample_waves > 0) the grid's workgroups split the sample_waves strided panels among them
hipError_t cmr_launch_scan_wide(const CmrScanGeom& g, const CmrScanArgs& a, hipStream_t s);
int cmr_wide_queries(int dtype, int dpad);      // queries per pass of the wide kernel (0 = unavailable)
size_t cmr_wide_lds_bytes(int ks, int cap);

// queries fp32 [nq, dim] (device) -> fragment-ordered blocks of the index dtype, zero padded
hipError_t cmr_launch_prep_queries(int dtype, const float* q, int nq, int dim, int dpad, int nqt,
                                   void* qfrag, int* nonfinite_flag, hipStream_t s);
// threshold search: n initial threshold keys that admit exactly the scores >= min_score
hipError_t cmr_launch_fill_threshold(float min_score, int n, u64* tau, hipStream_t s);
// rows fp32 [n, dim] (device) -> panel-major blocks at row offset row0 (+ optional fp32 shadow)
hipError_t cmr_launch_convert_rows(int dtype, const float* rows, long long n, int dim, int dpad,
                                   long long row0, void* corpus, float* shadow, int* nonfinite_flag,
                                   hipStream_t s);
// in-place row update (cmr_index_update_rows): entry i < m replaces local row dst_row[i] (strictly ascending, < the index's rows) by
// rows[src_idx[i]] (all three on the device, or in mapped host memory).  check = true: no store, raises *flag where a row is non-finite
// or rounds to Inf in the index dtype; check = false: returns at once when *flag is set, else packs and stores (+ the fp32 shadow)
hipError_t cmr_launch_update_rows(int dtype, bool check, const float* rows, const long long* dst_row, const long long* src_idx, long long m, int dim,
                                  int dpad, void* corpus, float* shadow, int* flag, hipStream_t s);
// per-wave candidate lists -> per-query top-k (ids/scores + min/max), or the sampling threshold
// grouped = true: the lists come from a query-split scan ([group][W][nq_stride]): query q reads group q / nq_stride
hipError_t cmr_launch_merge_query(const u64* lists, const int* cnt, int W, int nq_stride, int cap, int nq, int k,
                                  const float2* mm, long long id_base, int64_t* out_ids, float* out_scores,
                                  float* out_min, float* out_max, u64* out_tau, hipStream_t s, bool grouped = false,
                                  const int* skip_if_one = nullptr);      // device word: 1 = the results are final already (cmr_launch_scan_fin), return at once
// whole search of a small corpus in one launch (nq <= 16): kind 1 = <= 32 panels, kind 2 = hierarchical (up to max_panels panels,
// k <= 64; needs the arrival counter), 0 = not applicable.  `arrive`: a zeroed device int the launches of
// one stream share (nullptr: single-workgroup flat path only).
int cmr_tiny_kind(int nq, int npanels, int k, int multi, int max_panels);
size_t cmr_tiny_scratch_bytes(int nq, int npanels, int k, int multi, int max_panels);
hipError_t cmr_launch_tiny_search(int dtype, const void* corpus, const float* q, int nq, int dim, int dpad, long long nrows, int k, long long id_base,
                                  void* scratch, int64_t* out_ids, float* out_scores, float* out_min, float* out_max, int* flag, int* arrive,
                                  int max_panels, hipStream_t s, int* done = nullptr);      // done: as CmrScanArgs::fin_done (set to 1 behind the results)
hipError_t cmr_launch_tiny_scores(int dtype, const void* corpus, const float* q, int nq, int dim, int dpad, long long nrows, void* scratch,
                                  float* out, long long ld_out, int* flag, hipStream_t s, int* arrive = nullptr, int* done = nullptr);      // arrive (zeroed device int) + done: the last workgroup sets *done = 1 behind everybody's rows
// per-row top-k (k <= 4096) of a materialised score matrix [nq, ld]
hipError_t cmr_launch_topk_rows(const float* scores, long long ld, int n, int nq, int k, long long id_base,
                                int64_t* out_ids, float* out_scores, float* out_min, float* out_max, hipStream_t s);
// complete ranking by descending score (sort_kernels.hip: one stable LSD radix sort; ties by ascending row).  Workspace of nb segments of
// n rows, score_bytes 4 (fp32) or 8 (fp64).  fp32: one query, ids (+ id_base) and scores to the caller's buffers.  fp64: scores [nb][n], the
// first n_out ranks of every query stay in the workspace, at *ids_at [nb][n_out] and *scores_at [nb][n_out].
size_t cmr_sort_workspace_bytes(long long n, int nb, int score_bytes);
hipError_t cmr_launch_sort_scores(const float* scores, long long n, long long id_base, void* workspace, int64_t* out_ids,
                                  float* out_scores, hipStream_t s);
hipError_t cmr_launch_sort_scores_f64(const double* scores, long long n, int nb, long long n_out, void* workspace, int64_t** ids_at,
                                      double** scores_at, hipStream_t s);
// the same sort over ready-made 64-bit keys with a 32-bit payload (one segment of n pairs): stable, ascending by the 8-bit digit positions
// set in `digits`, lowest first; the passes alternate between (key_a, val_a) and (key_b, val_b) and the result ends in (*key_out, *val_out)
size_t cmr_sort_keys64_hist_bytes(long long n);
hipError_t cmr_launch_sort_keys64(u64* key_a, u64* key_b, unsigned* val_a, unsigned* val_b, unsigned* hist, long long n, unsigned digits, u64** key_out,
                                  unsigned** val_out, hipStream_t s);
// ---- range search (range_kernels.hip) over a materialised score block [nb][ld] (ld % 4 == 0, n < 2^32 rows)
// bound_code: the code `lo` a score's code is compared with (score >= min_score <=> code >= lo; +inf: above every score's)
// count: cnt (cmr_range_counter_bytes(n, nb)) = exclusive prefix of the hits per (query, tile of CMR_RANGE_TILE rows), query-major, the
//        total behind it; counts[nb] = hits per query.  Two launches.
// compact: the hits of queries [q_first, q_first + nq_group) — `hits` of them by cnt — as (query in group << 32 | ~code, row), per query by
//        ascending row, into key / val [hits].
// finish: sorted pairs -> row + id_base and the score's bits gathered from the block, out_ids / out_scores [hits]
// mask (filtered range search; nullptr: the unfiltered kernels): a hit also needs its allow bit — the masked variants of count
//        and compact.  words: device, one uint32 per 32-row panel and mask, ceil(n / 32) words each (none beyond is read); query q of the
//        block [nb] reads the mask at words + (q0 + q) * stride: stride 0 = one mask for every query, q0 = where in `words` the block's
//        first query has its mask (the block's place in the call's batch, or 0 where the words were built for the block alone).
struct CmrRangeMask { const unsigned* words; long long stride; long long q0; };
unsigned cmr_range_bound_code(float min_score);
size_t cmr_range_counter_bytes(long long n, int nb);
hipError_t cmr_launch_range_count(const float* scores, long long ld, long long n, int nb, unsigned lo, unsigned* cnt, long long* counts, hipStream_t s,
                                  const CmrRangeMask* mask = nullptr);
hipError_t cmr_launch_range_compact(const float* scores, long long ld, long long n, unsigned lo, const unsigned* offs, int q_first, int nq_group, long long hits,
                                    u64* key, unsigned* val, hipStream_t s, const CmrRangeMask* mask = nullptr);
hipError_t cmr_launch_range_finish(const u64* key, const unsigned* val, long long hits, const float* scores, long long ld, int q_first, long long id_base,
                                   int64_t* out_ids, float* out_scores, hipStream_t s);
// shard merge: ids/scores [S][nq][k] -> [nq][k]
hipError_t cmr_launch_merge_shards(const int64_t* ids, const float* scores, int S, int nq, int k,
                                   int64_t* out_ids, float* out_scores, hipStream_t s);
// exact fp32 dot of queries with candidate rows, then top-k
// (candidate and output ids are global: local row + id_base)
hipError_t cmr_launch_rescore(int dtype, const void* corpus, const float* shadow, int dim, int dpad,
                              long long nrows, long long id_base, const float* q, int nq, const int64_t* cand, int n_cand,
                              int k, int64_t* out_ids, float* out_scores, hipStream_t s);
// gather rows as fp32
hipError_t cmr_launch_gather_rows(int dtype, const void* corpus, int dim, int dpad, long long nrows, long long id_base,
                                  const int64_t* ids, long long n, float* out, hipStream_t s);
// ids[i] (shard-local row, < 0 = empty) -> global id through the block table [local0[nb] | global0[nb]] (device)
hipError_t cmr_launch_remap_ids(int64_t* ids, long long n, const long long* tab, int nb, hipStream_t s);
// allow words [nq_masks][n_words] of a filtered search from row-id lists.  fill: exclude = every row of [0, size) set, tail
// bits zero; allow = none.  apply: entry e of ids[0, n_ids) clears (exclude) / sets (allow) the bit of its LOCAL row in the words of the
// query that owns it (off: nq + 1 CSR offsets on the device, nullptr = one list, mask 0); ids are global (id_base, or nb > 1: the block
// table tab = [local0[nb] | global0[nb]]); negative ids and ids this index does not hold are skipped.  No access out of bounds whatever
// ids and offsets hold.
hipError_t cmr_launch_row_mask_fill(unsigned* words, long long nq_masks, long long n_words, long long size, int exclude, hipStream_t s);
hipError_t cmr_launch_row_mask_apply_ids(unsigned* words, long long n_words, long long size, int exclude, const long long* off, int nq,
                                         const long long* ids, long long n_ids, long long id_base, const long long* tab, int nb, hipStream_t s);
// row removal by in-place compaction (compact_kernels.hip).  keep_prefix: kept_before[n_words + 1] = exclusive prefix of the
// keep words' popcounts (one workgroup), info[0] = kept rows, info[1] = first removed row (size when none).  compact_chunk: the kept rows of
// the source panels [p_first, p_end) move to their destination rows through `stage` (room for stage_panels >= p_end - p_first + 1 panels);
// compact_shadow_chunk: the same for the row-major fp32 shadow (`stage`: room for stage_rows >= 32 * (p_end - p_first) rows of dim floats).
// Chunks must be enqueued in ascending order on ONE stream.
hipError_t cmr_launch_keep_prefix(const unsigned* words, long long n_words, long long size, unsigned* kept_before, long long* info, hipStream_t s);
hipError_t cmr_launch_compact_chunk(void* corpus, int ks, const unsigned* words, const unsigned* kept_before, long long p_first, long long p_end,
                                    void* stage, long long stage_panels, hipStream_t s);
hipError_t cmr_launch_compact_shadow_chunk(float* shadow, int dim, const unsigned* words, const unsigned* kept_before, long long p_first,
                                           long long p_end, void* stage, long long stage_rows, hipStream_t s);
// masked mean-pool + L2 norm
hipError_t cmr_launch_pool(const void* hidden, int hidden_dtype, const int64_t* mask, int b, int l, int d,
                           int normalize, float* partial, float* out, int splits, hipStream_t s);
int cmr_pool_splits(int b, int l, int d);
// encoder layer pieces (encoder_kernels.hip): masked attention over a packed [b*L, 3*hidden] projection (head width 64; bf16 / fp16,
// or fp32 end to end on the f32-input MFMA), LayerNorm(y + bias + residual) (bf16 / fp16 / fp32, d % 4 == 0, d <= 2048; bias / residual may be NULL)
hipError_t cmr_launch_attention(const void* qkv, int dtype, const int* lens, int b, int L, int n_heads, int head_dim /* 64 or 32 */, void* out, hipStream_t s);
hipError_t cmr_launch_embed_layernorm(const long long* ids, const long long* tt, const void* word, const void* pos, const void* type,
                                      const void* gamma, const void* beta, float eps, long long rows, int L, int d, int vocab, int n_pos,
                                      int n_types, int pos_off, int dtype, void* out, hipStream_t s);
hipError_t cmr_launch_add_layernorm(const void* y, const void* bias, const void* res, const void* gamma, const void* beta, float eps,
                                    long long rows, int d, int dtype, void* out, hipStream_t s);
// the LAST layer's LayerNorm(y + bias + residual) with the masked mean-pool + L2-normalise of the encoder tail folded in: the
// [b, l, d] hidden state is never written (l % 16 == 0, d % 8 == 0, d <= 2048; partial = b * (l / 16) * d floats of scratch)
hipError_t cmr_launch_add_layernorm_pool(const void* y, const void* bias, const void* res, const void* gamma, const void* beta, float eps, int b, int l,
                                         int d, int dtype, const int* lens, int normalize, float* partial, float* out, hipStream_t s);
// BertEmbeddings from RAGGED token ids (int32, sequences back to back; off[b + 1] their starts): row (s, t) of the [b, L] mini-batch
hipError_t cmr_launch_embed_layernorm_ragged(const int* ids32, const int* off, const void* word, const void* pos, const void* type, const void* gamma,
                                             const void* beta, float eps, long long rows, int L, int d, int vocab, int n_pos, int pos_off, int dtype,
                                             void* out, hipStream_t s);
// small-M linear (one short query's token rows): mode 0 y = x w^T + bias, 1 gelu of it, 2 fp32 partial slabs [split, m, n]; and the slabs' consumer.
// m > 128 (up to CMR_ENCODER_ROWS_MAX, the many-row entry points): row tiles of 128 over grid.z, every row with the bits of the m <= 128 launch
int cmr_small_linear_split(int n, int k);
hipError_t cmr_launch_small_linear(const void* x, const void* w, const void* bias, int m, int n, int k, int dtype, int mode, void* out, hipStream_t s);
hipError_t cmr_launch_add_layernorm_partials(const float* part, int n_split, const void* bias, const void* res, const void* gamma, const void* beta, float eps,
                                             long long rows, int d, int dtype, void* out, hipStream_t s);
hipError_t cmr_launch_add_layernorm_partials_pool(const float* slabs, int n_split, const void* bias, const void* res, const void* gamma, const void* beta, float eps, int b,
                                                  int l, int d, int dtype, const int* lens, int normalize, float* partial, float* out, hipStream_t s);
// cross-encoder tail: the attention of ONE query row (token 0) per sequence and head, out [b, hidden] (head_dim 64 or 32; bf16 / fp16 / fp32), and the
// one-logit classification head out[s] = b2 + w2 . tanh(b1 + w1 x[s]) over rows x_stride elements apart (d % 8 == 0, d <= 2048; b1 / b2 may be NULL)
hipError_t cmr_launch_attention_cls(const void* qkv, int dtype, const int* lens, int b, int L, int n_heads, int head_dim /* 64 or 32 */, void* out, hipStream_t s);
hipError_t cmr_launch_cls_head(const void* x, long long x_stride, const void* w1, const void* b1, const void* w2, const void* b2, int b, int d, int dtype,
                               float* out, hipStream_t s);
// exact top-k of a 16-bit index (cmr_index_search_exact): rows fp32 [n, dim] (device) -> atomicMax of (max ||round(x)||, max ||round(x) - x||)
// into stats[2] (fp32, device), skipped when *flag (the append's non-finite flag, may be NULL) is set; no-op for fp32 indexes.
// src_idx (device, or NULL: rows 0 .. n-1): the n rows are rows[src_idx[0 .. n-1]] (an update's winning rows)
hipError_t cmr_launch_round_stats(int dtype, const float* rows, long long n, int dim, const int* flag, float* stats, hipStream_t s,
                                  const long long* src_idx = nullptr);
// re-score the sorted stage-1 lists cand_ids / cand_sc [nq, kc] (global ids, -1 padded; 16-bit scan scores) from the fp32 shadow,
// select the fp32 top-k (k <= 64, kc <= 4096) and certify each query (out_exact[nq] = 0 / 1) against stats = (M_x, M_dx).
// part: cmr_exact_part_bytes(nq, kc) of scratch; arrive: nq zeroed ints (re-armed by the kernel); output ids carry id_base
// (shards with a block table: id_base 0, ids are local rows until remapped)
size_t cmr_exact_part_bytes(int nq, int kc);
hipError_t cmr_launch_exact_certify(int dtype, const float* shadow, int dim, long long nrows, long long id_base, const long long* tab, int nb,
                                    const float* q, int nq, const int64_t* cand_ids, const float* cand_sc, int kc, int k, const float* stats,
                                    void* part, int* arrive, int64_t* out_ids, float* out_scores, int* out_exact, hipStream_t s);

// ---- diversified top-k (mmr_kernels.hip).  rows: candidate ids [nq, F] (global: id_base, or nb > 1: the block table) -> local
// rows, -1 for a void position (negative, not held, or an earlier position of the query carries the same id).  gram: out [nq, F, F],
// out[q][s][c] = the scan's score of (query = stored row of position s, corpus row of position c), -inf where either is void; F <= 128;
// qfrag = nullptr: both operands gathered from the panels; else the query side comes from fragments [nq * ceil(F / 32)][ks][64] in
// prep_queries' layout and only the corpus side can be void.  select: the greedy selection of mmr_select.h, out [nq, k] in pick order.
hipError_t cmr_launch_mmr_rows(const int64_t* ids, int nq, int F, long long nrows, long long id_base, const long long* tab, int nb, long long* rows,
                               hipStream_t s);
hipError_t cmr_launch_mmr_gram(int dtype, const void* corpus, const void* qfrag, const long long* rows, int nq, int F, int dpad, float* out,
                               hipStream_t s);
hipError_t cmr_launch_mmr_select(const int64_t* ids, const float* rel, const long long* rows, const float* gram, int nq, int F, int k, float lam32,
                                 int64_t* out_ids, float* out_scores, hipStream_t s);

// ---- certified int8 pre-filter of the pipelined 16-bit scan (prefilter_kernels.hip)
// companion of panels [panel0, panel0 + npanels): int8 blocks, (scale, quantisation error norm) per row, and the atomicMax of
// (max ||x||, max error norm) into stats[2]; rows at or beyond nrows count as zero rows
hipError_t cmr_launch_q8_quantise(int dtype, const void* corpus, int dpad, long long panel0, long long npanels, long long nrows, void* q8,
                                  float2* scales, float* stats, hipStream_t s);
// queries fp32 [nq, dim] -> two int8 parts in block order ([2][tiles][dpad / 32] blocks of 1 KiB) and (a_q, B_q, c_q, 0) per query slot
hipError_t cmr_launch_q8_pack_queries(int dtype, const float* q, int nq, int dim, int dpad, int tiles, const float* stats, void* qpack,
                                      float4* qconst, hipStream_t s);
struct CmrQ8Args {
    int dtype, dpad, nqt, cap;
    int grid;                  // filter: workgroups of 8 waves
    int rescore_grid;          // re-score: workgroups of cmr_q8_rescore_waves() waves; lists / cnt hold one row per wave
    const void* corpus;        // the 16-bit panels
    const void* q8;            // the int8 companion
    const float2* scales;
    const void* qfrag;         // 16-bit query fragments (prep_queries)
    const void* qpack;         // int8 query parts
    const float4* qconst;
    const u64* tau_init;       // [nqt * 32] thresholds of the sampling passes, or nullptr
    long long nrows;
    int npanels, nq, k;
    int keep_all;              // the filter keeps every row (the re-score path alone)
    void* wrec;                // [grid * 8][wave_cap] 16-byte records (row, ub, lb, query slot) of the filter's hits, one area per wave of its grid
    unsigned* wcnt;            // [grid * 8] records offered per wave, written by every wave of the filter (past wave_cap: the area filled, the rest went to keep[])
    int wave_cap;              // records per wave; 0: every hit goes to keep[] directly (keep_all, or pcap == 0)
    void* pair;                // [nqt * 32][pcap] 16-byte records (row, ub, lb, 0): the wave areas' records sorted by query (bucket step)
    unsigned* pair_cnt;        // [nqt * 32] pairs offered per query, zeroed before the filter (past pcap: the list filled, the rest went to keep[])
    int pcap;                  // records per query; 0: no records at all and nothing to tighten
    unsigned* keep;            // [npanels] one 32-bit row mask per panel: written whole by the filter, OR-ed into by the bucket step and the tightening
    float* tau_tight;          // [nq] the thresholds after tightening (diagnostics)
    unsigned* cand_row;        // [nrows]: the rows of keep[]'s bits
    unsigned* n_cand;          // zeroed before the expansion
    u64* lists;
    int* cnt;
    // the int8 sample in front of the main pass (s_grid > 0): the filter body over s_nruns runs of s_run consecutive panels, run g at panel
    // g * s_stride (s_stride >= s_run), one run per wave of a grid of s_grid workgroups, against the level-0 threshold keys s_tau0
    int s_grid, s_run, s_stride, s_nruns;
    void* s_wrec;              // [s_grid * 8][s_wave_cap] the sample's records (a hit beyond the area is dropped)
    unsigned* s_wcnt;          // [s_grid * 8]
    int s_wave_cap;
    void* s_pair;              // [nqt * 32][s_pcap] the sample's records by query (a record beyond the list is dropped)
    unsigned* s_pair_cnt;      // [nqt * 32] zeroed before the sample
    int s_pcap;
    const u64* s_tau0;         // [nqt * 32] level-0 threshold keys
    u64* s_tau_out;            // [nq] threshold keys for the main pass: max(key of the k-th largest sampled lb, level-0 key)
};
// filter -> (bucket, tighten, when pcap > 0) -> expand -> rescore; all but the first in stream order behind the filter
// in front of them, with the int8 sample: filter (sample) -> bucket (sample) -> select, in stream order
hipError_t cmr_launch_q8_filter(const CmrQ8Args& a, hipStream_t s, bool sample = false);
hipError_t cmr_launch_q8_bucket(const CmrQ8Args& a, hipStream_t s, bool sample = false);
hipError_t cmr_launch_q8_select(const CmrQ8Args& a, hipStream_t s);
hipError_t cmr_launch_q8_tighten(const CmrQ8Args& a, hipStream_t s);
hipError_t cmr_launch_q8_expand(const CmrQ8Args& a, hipStream_t s);
hipError_t cmr_launch_q8_rescore(const CmrQ8Args& a, hipStream_t s);
int cmr_q8_rescore_waves(void);
