// The plan of a sample-map frame (csrc/rt_sample_map.cpp) under AddressSanitizer +
// UndefinedBehaviorSanitizer: a stand-alone program (tests/test_sample_map_native.py compiles and
// runs it; nothing is loaded into python). The edge tables of tests/test_sample_map_plan.py plus
// NULL and zero-length arguments, with exactly sized heap arrays so that any write past an output
// is a report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <vector>

#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_sample_map.h"

namespace sm = rt::sample_map;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) {                                                           \
            ++g_failed;                                                          \
            std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
        }                                                                        \
    } while (0)

// The plan by definition, quadratic and obviously right.
static void brute(const std::vector<uint32_t>& counts, uint32_t quantum, sm::Plan& p) {
    const uint64_t q = quantum > 1 ? quantum : 1;
    p = sm::Plan{};
    for (uint32_t n : counts) p.quantised.push_back(uint32_t((uint64_t(n) + q - 1) / q * q));
    std::vector<bool> used(counts.size(), false);
    for (size_t r = 0; r < counts.size(); r++) {
        size_t best = counts.size();
        for (size_t t = 0; t < counts.size(); t++)
            if (!used[t] && (best == counts.size() || p.quantised[t] > p.quantised[best])) best = t;
        used[best] = true;
        p.order.push_back(uint32_t(best));
    }
    std::vector<uint32_t> s = p.quantised;
    std::sort(s.begin(), s.end());
    s.erase(std::unique(s.begin(), s.end()), s.end());
    for (uint32_t L : s) {
        if (L == 0) continue;
        p.levels.push_back(L);
        p.level_tiles.push_back(uint32_t(std::count_if(p.quantised.begin(), p.quantised.end(), [&](uint32_t n) { return n >= L; })));
    }
}

static void expect_ok(const std::vector<uint32_t>& counts, uint32_t quantum) {
    sm::Plan want, got;
    brute(counts, quantum, want);
    std::string err;
    const int rc = sm::make_plan(counts.empty() ? nullptr : counts.data(), uint32_t(counts.size()), quantum, got, &err);
    CHECK(rc == RT_OK);
    if (rc != RT_OK) {
        std::fprintf(stderr, "  refused: %s\n", err.c_str());
        return;
    }
    CHECK(got.quantised == want.quantised);
    CHECK(got.order == want.order);
    CHECK(got.levels == want.levels);
    CHECK(got.level_tiles == want.level_tiles);
    // the array form, into exactly sized heap arrays
    std::vector<uint32_t> order(counts.size()), quant(counts.size());
    std::vector<uint32_t> levels(sm::kMaxLevels, 0xdeadu), tiles(sm::kMaxLevels, 0xdeadu);
    uint32_t j = 0xdeadu;
    CHECK(sm::plan_arrays(counts.data(), uint32_t(counts.size()), quantum, order.data(), levels.data(), tiles.data(), &j,
                          quant.data(), nullptr) == RT_OK);
    CHECK(j == want.levels.size() && order == want.order && quant == want.quantised);
    CHECK(std::equal(want.levels.begin(), want.levels.end(), levels.begin()));
    CHECK(std::equal(want.level_tiles.begin(), want.level_tiles.end(), tiles.begin()));
    for (size_t k = want.levels.size(); k < levels.size(); k++) CHECK(levels[k] == 0xdeadu && tiles[k] == 0xdeadu);
    // every output optional
    CHECK(sm::plan_arrays(counts.data(), uint32_t(counts.size()), quantum, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr) == RT_OK);
}

static void expect_refused(const std::vector<uint32_t>& counts, uint32_t quantum, const char* needle) {
    sm::Plan keep;
    keep.levels = {77u};
    std::string err;
    CHECK(sm::make_plan(counts.data(), uint32_t(counts.size()), quantum, keep, &err) == RT_ERR_INVALID_ARGUMENT);
    CHECK(err.find(needle) != std::string::npos);
    CHECK(keep.levels.size() == 1 && keep.levels[0] == 77u && keep.order.empty());   // left as it was
    CHECK(sm::make_plan(counts.data(), uint32_t(counts.size()), quantum, keep, nullptr) == RT_ERR_INVALID_ARGUMENT);
    std::vector<uint32_t> order(counts.size(), 0xdeadu);
    uint32_t j = 0xdeadu;
    CHECK(sm::plan_arrays(counts.data(), uint32_t(counts.size()), quantum, order.data(), nullptr, nullptr, &j, nullptr,
                          &err) == RT_ERR_INVALID_ARGUMENT);
    CHECK(j == 0xdeadu && std::all_of(order.begin(), order.end(), [](uint32_t v) { return v == 0xdeadu; }));
}

int main() {
    const std::vector<uint32_t> example = {0, 1, 2, 7, 8, 64, 64, 3, 0, 0, 5, 12, 12, 1, 2, 2, 9, 9, 9, 30, 0, 64, 7, 8};
    expect_ok(example, 0);
    expect_ok(example, 1);
    expect_ok(example, 16);
    expect_ok({5}, 0);
    expect_ok({0}, 0);
    expect_ok({}, 0);
    expect_ok({}, 16);
    expect_ok(std::vector<uint32_t>(24, 0u), 0);
    expect_ok(std::vector<uint32_t>(24, 6u), 4);
    expect_ok({3, sm::kMaxCount, 0}, 0);
    expect_ok({5, sm::kMaxCount - 1}, 2);
    {
        std::vector<uint32_t> c(65);   // 0 and 1 .. 64: exactly kMaxLevels levels
        std::iota(c.begin(), c.end(), 0u);
        expect_ok(c, 0);
        c.push_back(65u);
        expect_refused(c, 0, "65 levels");
        expect_ok(c, 2);
    }
    {
        uint32_t s = 12345u;   // a seeded table of 375 tiles (200x120)
        std::vector<uint32_t> c(375);
        for (uint32_t& v : c) {
            s = s * 1664525u + 1013904223u;
            v = (s >> 24) % 7u;
        }
        expect_ok(c, 0);
        expect_ok(c, 3);
    }
    expect_refused({3, 7, sm::kMaxCount + 1, 0xffffffffu}, 0, "tile_counts[2]");
    expect_refused({5, sm::kMaxCount - 1}, 3, "tile_counts[1]");
    expect_refused({1}, 0xffffffffu, "quantum");
    {   // NULL table
        sm::Plan p;
        std::string err;
        CHECK(sm::make_plan(nullptr, 3, 0, p, &err) == RT_ERR_INVALID_ARGUMENT && err.find("NULL") != std::string::npos);
        CHECK(sm::make_plan(nullptr, 0, 0, p, &err) == RT_OK && p.order.empty() && p.levels.empty());
        CHECK(sm::plan_arrays(nullptr, 3, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID_ARGUMENT);
        CHECK(sm::plan_arrays(nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == RT_OK);
    }
    {   // totals: the ragged 44x27 band, a mismatched band, NULL info
        sm::Plan p;
        CHECK(sm::make_plan(example.data(), 24, 0, p, nullptr) == RT_OK);
        rt_sample_map_info info{};
        std::string err;
        CHECK(sm::totals(p, 44, 27, &info, &err) == RT_OK);
        uint64_t want = 0;
        for (uint32_t t = 0; t < 24; t++) want += uint64_t(example[t]) * (t % 6 == 5 ? 4 : 8) * (t / 6 == 3 ? 3 : 8);
        CHECK(info.samples == want && info.tile_launches == 113 && info.tiles == 24 && info.levels == 10);
        CHECK(info.min_count == 1 && info.max_count == 64);
        CHECK(sm::totals(p, 48, 32, &info, &err) == RT_OK);   // the same 6 x 4 tiles, all whole
        CHECK(info.samples == 64u * std::accumulate(example.begin(), example.end(), uint64_t(0)));
        CHECK(sm::totals(p, 64, 40, &info, &err) == RT_ERR_INVALID_ARGUMENT);
        CHECK(sm::totals(p, 0, 0, &info, nullptr) == RT_ERR_INVALID_ARGUMENT);
        CHECK(sm::totals(p, 44, 27, nullptr, &err) == RT_ERR_INVALID_ARGUMENT);
        CHECK(sm::totals(p, 65535, 65535, &info, nullptr) == RT_ERR_INVALID_ARGUMENT);
    }
    if (g_failed) {
        std::fprintf(stderr, "%d of %d checks FAILED\n", g_failed, g_checks);
        return 1;
    }
    std::printf("sample_map_plan: %d checks passed (ASan + UBSan)\n", g_checks);
    return 0;
}
