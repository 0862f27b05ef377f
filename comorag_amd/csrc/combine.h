// Flat combining of concurrent synchronous calls.  Host only: no HIP call, compiles with a plain C++17 compiler
// (tools/combine_selftest.cpp drives it with a recording callback; tests/test_combine_host.py).
//
// Threads that issue the same kind of single call on one index at the same time (ComoRAG answers up to 16 questions from one
// thread pool, every thread with one-query dense_passage_retrieval / get_fact_scores / run_ppr calls) are served by ONE batched
// call:
//   - a call that arrives while no batch of its key is being gathered or run becomes the LEADER;
//   - the leader takes what is queued for the key, itself first, in arrival order, up to `width` queries in total;
//   - it runs ONE batch through the owner's callback, which answers every participant (code and message per request),
//     and wakes the participants;
//   - if requests queued up meanwhile it hands leadership to the first of them: a leader serves one batch, never a stream.
// A caller that finds nobody else forms a batch of one; the callback sees n == 1 and runs the unchanged single call with the
// caller's own arguments.  With the gather window at 0 the only cost of that is one uncontended mutex, and batches form only from
// calls that arrive while an earlier batch is on the device.  With a window (`wait_us` > 0) the leader waits until `width`
// queries have gathered or the window has passed, whichever comes first; a request as wide as the batch (nq >= width) cannot
// share and never waits.
//
// Locks: a queued caller holds NO lock of the owner.  The callback takes whatever it needs (the index's shared lock) once for
// the batch.  Waiters that held a shared lock while the leader asked for another would deadlock with an appender waiting for the
// exclusive lock between them (std::shared_mutex may prefer the writer).
//
// Errors are per request: the owner's last-error text is thread-local, so the callback records code and text in the request and
// each participant publishes them in its own thread after submit() returns.
//
// Filtered searches (cmr_index_search_masked, cmr_index_search_masked_each) are queued only where the index option "combine_filtered" is set:
// a batch of them runs as ONE per-query-mask search, every query with its caller's mask.
// Not combined (the owner never queues them): cmr_index_search_min_score, cmr_index_sorted_scores, cmr_index_search_exact,
// cmr_graph_ppr, every _dev / pipelined call, cmr_mindex_* (searches through a multi-device handle do not pass here).  The encoder
// does not pass here either: concurrent one-question encodes are combined one level up, by the Python restatement of this protocol
// (embedding_model/combine.py, config `embedding_combine`), over the many-row linear kernels (cmr_encoder_linear_rows*).
#pragma once
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace cmr_combine {

constexpr int kMaxWidth = 16;      // = CMR_PPR_MAX_BATCH and the widest single-launch search

// What must be equal for two calls to share a batch: up to 6 words, compared as bytes.
struct Key {
    uint64_t w[6] = {0, 0, 0, 0, 0, 0};
    bool operator<(const Key& o) const { return memcmp(w, o.w, sizeof(w)) < 0; }
    static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
};

// One caller's call.  The owner fills `args` (its own argument block) and `nq`; the batch callback fills `rc` and `err`.
struct Request {
    void* args = nullptr;
    int nq = 1;
    int rc = 0;
    std::string err;
    // -- combiner's own
    bool done = false, lead = false;
    std::condition_variable cv;
};

// Runs ONE batch: `n` requests of one key, `reqs[0]` the leader's own, nq summing to at most the width.  Must set rc (and err on
// failure) of every request.  Called on the leader's thread with no combiner lock held.
using RunFn = void (*)(void* ctx, Request** reqs, int n);

class Combiner {
public:
    // Serves `req` — as the leader of a batch or as a participant of somebody else's — and returns once req->rc / req->err are set.
    void submit(const Key& key, Request* req, int width, long long wait_us, RunFn run, void* ctx) {
        std::unique_lock<std::mutex> lk(mu_);
        Slot& slot = slots_[key];
        slot.queue.push_back(req);
        slot.queued_nq += req->nq;
        if (slot.busy) {
            if (slot.gathering && slot.queued_nq >= width) slot.leader->cv.notify_one();      // the window ends with the batch full
            req->cv.wait(lk, [&] { return req->done || req->lead; });
            if (req->done) return;
        } else {
            slot.busy = true;
        }
        // leader of one batch: this request is the queue's head
        slot.leader = req;
        if (wait_us > 0 && req->nq < width && slot.queued_nq < width) {
            slot.gathering = true;
            req->cv.wait_for(lk, std::chrono::microseconds(wait_us), [&] { return slot.queued_nq >= width; });
            slot.gathering = false;
        }
        Request* batch[kMaxWidth];
        int n = 0, total = 0;
        while (!slot.queue.empty() && n < kMaxWidth) {
            Request* r = slot.queue.front();
            if (n && total + r->nq > width) break;
            slot.queue.pop_front();
            batch[n++] = r;
            total += r->nq;
        }
        slot.queued_nq -= total;
        lk.unlock();
        run(ctx, batch, n);
        lk.lock();
        ++batches_;
        queries_ += total;
        if (total > max_width_) max_width_ = total;
        for (int i = 1; i < n; ++i) {      // (notified under the mutex: a woken participant's request may leave its stack only after we let go)
            batch[i]->done = true;
            batch[i]->cv.notify_one();
        }
        // `slot` is still ours: busy kept every other caller of the key out of leadership
        if (!slot.queue.empty()) {
            Request* next = slot.queue.front();
            slot.leader = next;
            next->lead = true;
            next->cv.notify_one();
        } else {
            slots_.erase(key);
        }
    }

    long long batches() const { std::lock_guard<std::mutex> g(mu_); return batches_; }
    long long queries() const { std::lock_guard<std::mutex> g(mu_); return queries_; }
    long long max_width() const { std::lock_guard<std::mutex> g(mu_); return max_width_; }
    // requests queued and not yet taken into a batch (the leader of a running batch is not among them)
    int waiting() const {
        std::lock_guard<std::mutex> g(mu_);
        int n = 0;
        for (const auto& kv : slots_) n += (int)kv.second.queue.size();
        return n;
    }

private:
    struct Slot {
        std::deque<Request*> queue;      // arrival order; the head is the leader while busy
        Request* leader = nullptr;
        int queued_nq = 0;
        bool busy = false;               // a leader of this key exists (gathering or running)
        bool gathering = false;
    };
    mutable std::mutex mu_;
    std::map<Key, Slot> slots_;
    long long batches_ = 0, queries_ = 0, max_width_ = 0;
};

// any NaN / Inf among n floats, as the packing kernels judge them for an index of `dtype` (0 fp32, 1 bf16, 2 f16: a finite fp32 value
// that rounds to an infinity there counts) — a query that would set the batch kernels' one flag per launch stays out of a batch
inline bool all_finite(const float* v, size_t n, int dtype = 0) {
    for (size_t i = 0; i < n; ++i) {
        uint32_t u;
        memcpy(&u, v + i, 4);
        if ((u & 0x7F800000u) == 0x7F800000u) return false;
        if (dtype == 1 && (((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16) & 0x7F80u) == 0x7F80u) return false;      // bf16, round to nearest even
        if (dtype == 2 && (u & 0x7FFFFFFFu) >= 0x477FF000u) return false;                                     // f16: |v| >= 65520 rounds to Inf
    }
    return true;
}

}  // namespace cmr_combine
