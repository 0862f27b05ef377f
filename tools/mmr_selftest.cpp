// Stand-alone driver of csrc/mmr_select.h (the host selection behind cmr_mmr_select and the shard path of cmr_mindex_search_mmr): random
// and degenerate inputs, checked against the properties the contract states.  No HIP, no device.  Meant for a sanitizer build on the host:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/mmr_selftest.cpp -o mmr_selftest && ./mmr_selftest
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../comorag_amd/csrc/mmr_select.h"

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_fail; std::printf("FAIL %s:%d  ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

struct Case {
    int F, k;
    float lam;
    std::vector<float> rel, gram;
    std::vector<int64_t> ids;
    std::vector<unsigned char> extra;      // empty: none
};

static void run(const Case& c, const char* what) {
    // the outputs sit at the very end of exact-size heap blocks: a write past k is a sanitizer report
    std::vector<int64_t> oi((size_t)c.k);
    std::vector<float> os((size_t)c.k);
    cmr_mmr::select_one(c.rel.data(), c.gram.data(), c.ids.data(), c.F, c.k, c.lam, c.extra.empty() ? nullptr : c.extra.data(), oi.data(), os.data());
    std::vector<char> isvoid((size_t)c.F);
    int live = 0;
    for (int p = 0; p < c.F; ++p) {
        bool v = c.ids[p] < 0 || (!c.extra.empty() && c.extra[p]);
        for (int e = 0; e < p && !v; ++e) v = c.ids[e] == c.ids[p];
        isvoid[p] = v;
        live += !v;
    }
    const int want = live < c.k ? live : c.k;
    std::set<int64_t> seen;
    float best_rel = -INFINITY;
    int best_pos = -1;
    for (int p = 0; p < c.F; ++p) if (!isvoid[p] && (best_pos < 0 || c.rel[p] > best_rel)) { best_rel = c.rel[p]; best_pos = p; }
    for (int j = 0; j < c.k; ++j) {
        if (j >= want) { CHECK(oi[j] == -1 && os[j] == -INFINITY, "%s: column %d not padded", what, j); continue; }
        CHECK(oi[j] >= 0 && seen.insert(oi[j]).second, "%s: pick %d repeats or is void (id %lld)", what, j, (long long)oi[j]);
        int pos = -1;
        for (int p = 0; p < c.F; ++p) if (!isvoid[p] && c.ids[p] == oi[j]) pos = p;
        CHECK(pos >= 0, "%s: pick %d is no live candidate", what, j);
        if (pos >= 0) {
            uint32_t a, b;
            memcpy(&a, &os[j], 4); memcpy(&b, &c.rel[pos], 4);
            CHECK(a == b, "%s: pick %d does not carry its relevance bits", what, j);
        }
        if (j == 0) CHECK(pos == best_pos, "%s: the first pick is not the most relevant live position", what);
    }
    if (c.lam == 1.0f)      // relevance order, ties by position
        for (int j = 1; j < want; ++j) CHECK(os[j - 1] >= os[j], "%s: lambda 1 is not in relevance order at %d", what, j);
}

int main() {
    std::mt19937 rng(1234);
    std::normal_distribution<float> nd(0.0f, 1.0f);
    const float lams[] = {0.0f, 0.3f, 0.5f, 1.0f};
    int n_cases = 0;
    for (int F : {1, 2, 3, 31, 32, 33, 64, 65, 127, 128})
        for (int k : {1, F / 2 > 0 ? F / 2 : 1, F})
            for (float lam : lams)
                for (int kind = 0; kind < 6; ++kind) {
                    Case c{F, k, lam, {}, {}, {}, {}};
                    c.rel.resize((size_t)F); c.gram.resize((size_t)F * F); c.ids.resize((size_t)F);
                    for (int p = 0; p < F; ++p) { c.rel[p] = nd(rng); c.ids[p] = 1000 + 7 * p; }
                    for (float& g : c.gram) g = nd(rng);
                    const char* what = "random";
                    if (kind == 1) { what = "all tied"; for (float& r : c.rel) r = 0.25f; for (float& g : c.gram) g = 0.5f; }
                    if (kind == 2) { what = "voids"; for (int p = 0; p < F; p += 3) c.ids[p] = -1; for (int p = 4; p < F; p += 5) c.ids[p] = c.ids[1 % F]; }
                    if (kind == 3) { what = "all void"; for (int64_t& i : c.ids) i = -1; }
                    if (kind == 4) { what = "extra voids, -inf columns"; c.extra.assign((size_t)F, 0); for (int p = 1; p < F; p += 2) { c.extra[p] = 1; for (int s = 0; s < F; ++s) c.gram[(size_t)s * F + p] = c.gram[(size_t)p * F + s] = -INFINITY; } }
                    if (kind == 5) { what = "signed zeros and huge values"; for (int p = 0; p < F; ++p) c.rel[p] = (p & 1) ? -0.0f : 0.0f; for (size_t i = 0; i < c.gram.size(); ++i) c.gram[i] = (i % 3) ? 3.0e38f : -3.0e38f; }
                    run(c, what);
                    ++n_cases;
                }
    // the batch form and the argument rules
    {
        const int nq = 3, F = 5, k = 4;
        std::vector<float> rel((size_t)nq * F), gram((size_t)nq * F * F);
        std::vector<int64_t> ids((size_t)nq * F), oi((size_t)nq * k), oi1((size_t)k);
        std::vector<float> os((size_t)nq * k), os1((size_t)k);
        for (float& r : rel) r = nd(rng);
        for (float& g : gram) g = nd(rng);
        for (size_t i = 0; i < ids.size(); ++i) ids[i] = (int64_t)(i % F);
        cmr_mmr::select(rel.data(), gram.data(), ids.data(), nq, F, k, 0.5f, oi.data(), os.data());
        for (int q = 0; q < nq; ++q) {
            cmr_mmr::select_one(rel.data() + (size_t)q * F, gram.data() + (size_t)q * F * F, ids.data() + (size_t)q * F, F, k, 0.5f, nullptr, oi1.data(), os1.data());
            for (int j = 0; j < k; ++j) CHECK(oi1[j] == oi[(size_t)q * k + j] && os1[j] == os[(size_t)q * k + j], "batch row %d differs at %d", q, j);
        }
        CHECK(cmr_mmr::check_args(1, 8, 4, 0.5, 128) == 0 && cmr_mmr::check_args(1, 128, 128, 1.0, 128) == 0 && cmr_mmr::check_args(1, 8, 4, 0.0, 128) == 0, "valid arguments refused");
        CHECK(cmr_mmr::check_args(0, 8, 4, 0.5, 128) == 1 && cmr_mmr::check_args(1, 8, 0, 0.5, 128) == 1 && cmr_mmr::check_args(1, 8, 9, 0.5, 128) == 1, "nq / k rules");
        CHECK(cmr_mmr::check_args(1, 8, 4, NAN, 128) == 1 && cmr_mmr::check_args(1, 8, 4, 1.5, 128) == 1 && cmr_mmr::check_args(1, 8, 4, -0.1, 128) == 1, "lambda rules");
        CHECK(cmr_mmr::check_args(1, 129, 4, 0.5, 128) == 2, "F above the limit");
        const float nan_in[3] = {0.0f, NAN, 1.0f};
        CHECK(cmr_mmr::any_nan(nan_in, 3) && !cmr_mmr::any_nan(nan_in, 1), "any_nan");
    }
    std::printf("mmr_selftest: %d cases, %d failures\n", n_cases, g_fail);
    return g_fail ? 1 : 0;
}
