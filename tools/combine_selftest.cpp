// Host driver of comorag_amd/csrc/combine.h for tests/test_combine_host.py: the combiner with a "run batch" callback that runs nothing
// and records what it was given.  Plain C++, no GPU:
//     g++ -std=c++17 -O1 -pthread -shared -fPIC tools/combine_selftest.cpp -o combine_selftest.so
// The test calls cst_submit from Python threads through ctypes (which releases the interpreter lock for the call).
#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>

#include "../comorag_amd/csrc/combine.h"

namespace {

struct Call { long long key; int tag, want_rc, fail_batch, batch = -1; };
struct BatchRecord { long long key; int leader, n, total; int tags[cmr_combine::kMaxWidth]; };

struct Harness {
    cmr_combine::Combiner comb;
    std::mutex mu;
    std::condition_variable gate_cv;
    bool gate_closed = false;
    std::vector<BatchRecord> batches;
    std::atomic<int> running{0};      // callbacks entered so far
};

void run_batch(void* ctx, cmr_combine::Request** reqs, int n) {
    Harness* h = (Harness*)ctx;
    BatchRecord rec{};
    const Call* lead = (const Call*)reqs[0]->args;
    rec.key = lead->key; rec.leader = lead->tag; rec.n = n;
    int culprit = -1;
    for (int i = 0; i < n; ++i) {
        const Call* c = (const Call*)reqs[i]->args;
        rec.tags[i] = c->tag;
        rec.total += reqs[i]->nq;
        if (c->fail_batch) culprit = c->tag;
    }
    int seq;
    {
        std::unique_lock<std::mutex> lk(h->mu);
        seq = (int)h->batches.size();
        h->batches.push_back(rec);
        h->running.fetch_add(1);
        h->gate_cv.wait(lk, [&] { return !h->gate_closed; });      // "on the device" for as long as the test says
    }
    for (int i = 0; i < n; ++i) {
        Call* c = (Call*)reqs[i]->args;
        c->batch = seq;
        char buf[96];
        if (culprit >= 0) {      // the combined call failed: everybody gets its error
            snprintf(buf, sizeof(buf), "batch failed by request %d", culprit);
            reqs[i]->rc = -5; reqs[i]->err = buf;
        } else if (c->want_rc) {      // one participant refused
            snprintf(buf, sizeof(buf), "request %d refused", c->tag);
            reqs[i]->rc = c->want_rc; reqs[i]->err = buf;
        } else {
            reqs[i]->rc = 0;
        }
    }
}

}  // namespace

extern "C" {

void* cst_create() { return new Harness(); }
void cst_destroy(void* h) { delete (Harness*)h; }

// one call: returns the code the batch gave this caller, its message in err, the batch it was served by in *batch
int cst_submit(void* hv, long long key, int tag, int nq, int width, long long wait_us, int want_rc, int fail_batch, char* err, int err_len, int* batch) {
    Harness* h = (Harness*)hv;
    Call c{key, tag, want_rc, fail_batch};
    cmr_combine::Request r;
    r.args = &c; r.nq = nq;
    cmr_combine::Key k;
    k.w[0] = (uint64_t)key;
    h->comb.submit(k, &r, width, wait_us, run_batch, h);
    if (err && err_len > 0) { strncpy(err, r.err.c_str(), (size_t)err_len - 1); err[err_len - 1] = 0; }
    if (batch) *batch = c.batch;
    return r.rc;
}

void cst_gate(void* hv, int closed) {
    Harness* h = (Harness*)hv;
    std::lock_guard<std::mutex> g(h->mu);
    h->gate_closed = closed != 0;
    h->gate_cv.notify_all();
}
int cst_running(void* hv) { return ((Harness*)hv)->running.load(); }
int cst_waiting(void* hv) { return ((Harness*)hv)->comb.waiting(); }

int cst_n_batches(void* hv) {
    Harness* h = (Harness*)hv;
    std::lock_guard<std::mutex> g(h->mu);
    return (int)h->batches.size();
}
// record i: [key, leader, n, total, tags[16]] as 20 long longs
void cst_batch(void* hv, int i, long long* out) {
    Harness* h = (Harness*)hv;
    std::lock_guard<std::mutex> g(h->mu);
    const BatchRecord& b = h->batches[(size_t)i];
    out[0] = b.key; out[1] = b.leader; out[2] = b.n; out[3] = b.total;
    for (int t = 0; t < cmr_combine::kMaxWidth; ++t) out[4 + t] = t < b.n ? b.tags[t] : -1;
}
void cst_counters(void* hv, long long* out) {
    Harness* h = (Harness*)hv;
    out[0] = h->comb.batches(); out[1] = h->comb.queries(); out[2] = h->comb.max_width();
}

}  // extern "C"
