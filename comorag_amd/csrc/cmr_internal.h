// Library-internal entry points and helpers shared by the host sources (api.hip and the headers it alone includes, comm.hip, multi.hip,
// ppr.hip and the entry points at the end of aux_kernels.hip / encoder_kernels.hip).  NOT part of the C-ABI (include/comorag_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/comorag_hip.h"
#include "combine.h"

// sets the calling thread's error message (cmr_last_error) and returns `code`
int cmr_fail(int code, const char* fmt, ...);

// the one HIP error check of the library: returns from the calling function with the error text set
#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            const int code_ = (e_ == hipErrorOutOfMemory) ? CMR_ERR_OOM                           \
                              : (e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice) ? CMR_ERR_NO_DEVICE \
                                                                                        : CMR_ERR_HIP; \
            return cmr_fail(code_, "%s failed: %s", #expr, hipGetErrorString(e_));                \
        }                                                                                         \
    } while (0)

// device of the calling thread / is `device_id` a gfx950 this library can run on (api.hip; validated devices are remembered)
__attribute__((visibility("hidden"))) int cmr_set_device(int device);
__attribute__((visibility("hidden"))) int cmr_check_device(int device_id);

// a device buffer that only grows
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t need) {
        if (need <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; cap = 0; }
        size_t want = std::max(need, cap * 2);
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) return e;
        cap = want;
        return hipSuccess;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// cmr_index_search in two halves: `begin` enqueues the whole search on a workspace stream of the index and returns at once,
// `finish` waits for it, reports a non-finite query and copies ids / scores / min / max out (any of them may be NULL).  Every
// pending search must be finished or abandoned.  take_lock = true holds the index's shared lock from begin to finish — both
// calls must then come from ONE thread; take_lock = false is for an owner that excludes appends itself (the multi-device index
// holds its own layout lock around begin .. finish and is the only one to append to its shards).
struct CmrPending;
int cmr_index_search_begin(cmr_index_t* idx, const float* q, int nq, int k, const float* min_score, bool take_lock, CmrPending** out);
int cmr_index_search_finish(CmrPending* p, int64_t* out_ids, float* out_scores, float* out_min, float* out_max);
void cmr_index_search_abandon(CmrPending* p);
// The row filter of a filtered call as the caller gave it — host pointers, or device pointers for the
// _dev calls; none: every row.  The words forms: [n_masks][n_words] allow words, one word per 32-row panel.  The id forms: row ids in the
// domain the searches return, `mode` CMR_IDS_ALLOW or CMR_IDS_EXCLUDE, one list for every query (off NULL) or CSR per query.  each: one
// mask or list per query (a batch of one query included: the per-query scan variant and its route bits).  Everything that reads a filter
// (row_filter.h, range_host.h, multi.hip) reads this struct.
struct RowFilter {
    enum Kind { none, words_form, ids_form } kind = none;
    bool each = false;
    const uint32_t* words = nullptr; int64_t n_words = 0; int n_masks = 0;
    int mode = 0; const int64_t* off = nullptr; const int64_t* ids = nullptr; int64_t n_ids = 0;
    static RowFilter of_words(const uint32_t* words, int64_t n_words, int n_masks, bool each) { return {words_form, each, words, n_words, n_masks}; }
    static RowFilter of_ids(int mode, const int64_t* off, const int64_t* ids, int64_t n_ids) { return {ids_form, off != nullptr, nullptr, 0, 0, mode, off, ids, n_ids}; }
};
// every check of a filtered call that needs neither an index nor a device (row_filter.h, range_host.h, mmr_host.h), one of each: the bound, the
// words ladder, the id-list ladder (off_host: CSR offsets readable here, or NULL), the ladder of a host filter's form, the arguments of
// a range search or count (f none: the unfiltered call's), the arguments of the diversified top-k
int cmr_min_score_check(float min_score);
int cmr_words_args_check(const void* allow, int nq, int64_t n_words, int n_masks);
int cmr_ids_args_check(int mode, int nq, int k, const int64_t* off_host, const int64_t* ids, int64_t n_ids);
int cmr_filter_args_check(const RowFilter& f, int nq, int k);
int cmr_range_args_check(const void* idx, const void* q, const void* out, int nq, float min_score, const RowFilter& f);
int cmr_mmr_args_check(int nq, int F, int k, double lam);
// the filtered top-k the same way as cmr_index_search_begin: `begin` takes checked arguments, the pending search ends in
// cmr_index_search_finish / _abandon.  min_score (read during `begin` only): the filtered threshold search, entries below the
// bound come back as padding
int cmr_index_search_ids_begin(cmr_index_t* idx, const float* q, int nq, int k, const RowFilter& f, bool take_lock, CmrPending** out,
                               const float* min_score = nullptr);
// range search and count of one index behind their argument checks (range_host.h; *out is NULL), for the shards of multi.hip
int cmr_index_range_count_host(cmr_index_t* idx, const float* q, int nq, float min_score, int64_t* out_counts, const RowFilter& f);
int cmr_index_range_search_host(cmr_index_t* idx, const float* q, int nq, float min_score, int64_t max_total, cmr_range_result_t** out, const RowFilter& f);

// the result of a range search (cmr_range_result_t): CSR lists in host arrays the library owns.  range_host.h and multi.hip fill it.
struct cmr_range_result {
    int nq = 0;
    int64_t* lims = nullptr;      // [nq + 1]
    int64_t* ids = nullptr;       // [lims[nq]]
    float* scores = nullptr;      // [lims[nq]]
    ~cmr_range_result() { delete[] lims; delete[] ids; delete[] scores; }
};

// shrink an index to its first n_rows rows (roll-back of a multi-shard append that failed on a later shard)
int cmr_index_truncate(cmr_index_t* idx, long long n_rows);
// cmr_index_remove_ids for the owner of a shard's block table (multi.hip): ids in the domain the shard returns NOW (its current table), any
// number of blocks; the table is stale once rows went and the owner sets the new one (cmr_index_set_id_blocks) before the next search
int cmr_index_compact_ids(cmr_index_t* idx, const int64_t* ids, int64_t n_ids, int64_t* n_removed);
// one shard's share of a row update (multi.hip plans: cmr_mindex_plan_update): entry i replaces local row local_rows[i] (strictly
// ascending) by row src[i] of the host rows [n_rows, dim].  phases: CMR_UPD_CHECK — nothing is written, CMR_ERR_NONFINITE when a source row
// would be refused; CMR_UPD_WRITE — the stores and the maxima, for entries checked before; both — cmr_index_update_rows' own order
enum { CMR_UPD_CHECK = 1, CMR_UPD_WRITE = 2 };
int cmr_index_update_planned(cmr_index_t* idx, const int64_t* local_rows, const int64_t* src, int64_t m, const float* rows, int64_t n_rows, int phases);

// for ppr.hip: scores of nb host queries [nb, dim] into a device buffer [nb, n] of the index's workspace, row b holding the bits a
// one-query scan of q_host[b] gives (shared index lock held, workspace reserved for the calling thread) until
// cmr_index_scores_release, which also reports a non-finite query
int cmr_index_scores_to_device_batch(cmr_index_t* idx, const float* q_host, int nb, float** scores_dev, long long* n, void** stream);
int cmr_index_scores_release(cmr_index_t* idx);
long long cmr_index_row_count(cmr_index_t* idx);      // (no device call)

// for multi.hip (cmr_mindex_pair_scores): the pair scores of candidate rows this shard may not hold.  rows [nq * T * 32, dim]
// fp32 on the host, T = ceil(F / 32): query i's candidate rows at rows + i * T * 32 * dim, zero rows behind the F-th; they are packed as
// queries and scored against the candidates of ids [nq, F] (global) that this shard holds: out[i][s][c] is finite where the shard holds
// position c (and no earlier position repeats its id), -inf elsewhere, whatever position s is.
int cmr_index_gram_rows(cmr_index_t* idx, const float* rows, const int64_t* ids, int nq, int F, float* out);

// for ppr.hip: the combiner of an index (combine.h) — its width (0: off; *dim: floats of one query) and one submission
// with the index's gather window
int cmr_index_combine_width(cmr_index_t* idx, int* dim, int* dtype);
void cmr_index_combine_submit(cmr_index_t* idx, const cmr_combine::Key& key, cmr_combine::Request* req, int width, cmr_combine::RunFn run, void* ctx);
