// The block table of a one-launch sample-map frame (csrc/rt_sample_map.cpp make_block_plan,
// block_plan_arrays) under AddressSanitizer + UndefinedBehaviorSanitizer: a stand-alone program
// (tests/test_sample_map_blocks_native.py compiles and runs it; nothing is loaded into python). The
// cases of tests/test_sample_map_blocks.py plus NULL and zero-length arguments, with exactly sized
// heap arrays so that any write past an output is a report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
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

// The table by definition: the tiles by (count descending, index ascending), found one at a time.
static std::vector<uint32_t> brute(const std::vector<uint32_t>& counts, uint32_t quantum, uint64_t unit) {
    const uint64_t q = quantum > 1 ? quantum : 1;
    std::vector<uint64_t> n;
    for (uint32_t c : counts) n.push_back((uint64_t(c) + q - 1) / q * q);
    std::vector<bool> used(n.size(), false);
    std::vector<uint32_t> out;
    for (size_t r = 0; r < n.size(); r++) {
        size_t best = n.size();
        for (size_t t = 0; t < n.size(); t++)
            if (!used[t] && (best == n.size() || n[t] > n[best])) best = t;
        used[best] = true;
        if (n[best] == 0) continue;
        const uint64_t k = (n[best] + unit - 1) / unit;
        for (uint64_t c = 0; c < k; c++) {
            const uint32_t row[4] = {uint32_t(best), uint32_t(c * n[best] / k), uint32_t((c + 1) * n[best] / k), 0u};
            out.insert(out.end(), row, row + 4);
        }
    }
    return out;
}

// `unit` 0: automatic, `want_unit` the value the rule gives.
static void expect_ok(const std::vector<uint32_t>& counts, uint32_t quantum, uint32_t unit, uint32_t want_unit) {
    const std::vector<uint32_t> want = brute(counts, quantum, want_unit);
    const uint32_t* table = counts.empty() ? nullptr : counts.data();
    const uint32_t n = uint32_t(counts.size());
    sm::BlockPlan bp;
    std::string err;
    const int rc = sm::make_block_plan(table, n, quantum, unit, bp, &err);
    CHECK(rc == RT_OK);
    if (rc != RT_OK) {
        std::fprintf(stderr, "  refused: %s\n", err.c_str());
        return;
    }
    CHECK(bp.unit_samples == want_unit && bp.blocks.size() * 4u == want.size());
    CHECK(bp.blocks.size() == sm::count_blocks(bp.plan, want_unit));
    uint32_t live = 0;
    for (uint32_t c : counts) live += c != 0u;
    CHECK(bp.live_tiles == live);
    // the array form, into an exactly sized heap array
    std::vector<uint32_t> out(want.size(), 0xdeadu);
    uint64_t nb = 0xdeadu;
    uint32_t used = 0xdeadu;
    CHECK(sm::block_plan_arrays(table, n, quantum, unit, out.data(), want.size() / 4u, &nb, &used, nullptr) == RT_OK);
    CHECK(out == want && nb == want.size() / 4u && used == want_unit);
    // a size query, and every output optional
    nb = 0xdeadu;
    CHECK(sm::block_plan_arrays(table, n, quantum, unit, nullptr, 0, &nb, nullptr, nullptr) == RT_OK && nb == want.size() / 4u);
    CHECK(sm::block_plan_arrays(table, n, quantum, unit, nullptr, 0, nullptr, nullptr, nullptr) == RT_OK);
    if (!want.empty()) {   // one block short: refused, nothing written
        std::vector<uint32_t> small(want.size() - 4u, 0xdeadu);
        nb = 0xdeadu;
        CHECK(sm::block_plan_arrays(table, n, quantum, unit, small.data(), want.size() / 4u - 1u, &nb, &used, &err) ==
              RT_ERR_INVALID_ARGUMENT);
        CHECK(err.find("capacity") != std::string::npos && nb == 0xdeadu);
        CHECK(std::all_of(small.begin(), small.end(), [](uint32_t v) { return v == 0xdeadu; }));
    }
}

static void expect_refused(const std::vector<uint32_t>& counts, uint32_t quantum, uint32_t unit, const char* needle) {
    sm::BlockPlan keep;
    keep.unit_samples = 77u;
    keep.blocks.push_back(sm::Block{1u, 2u, 3u, 0u});
    std::string err;
    CHECK(sm::make_block_plan(counts.data(), uint32_t(counts.size()), quantum, unit, keep, &err) == RT_ERR_INVALID_ARGUMENT);
    CHECK(err.find(needle) != std::string::npos);
    CHECK(keep.unit_samples == 77u && keep.blocks.size() == 1u && keep.plan.order.empty());   // left as it was
    CHECK(sm::make_block_plan(counts.data(), uint32_t(counts.size()), quantum, unit, keep, nullptr) == RT_ERR_INVALID_ARGUMENT);
    std::vector<uint32_t> out(32, 0xdeadu);
    uint64_t nb = 0xdeadu;
    uint32_t used = 0xdeadu;
    CHECK(sm::block_plan_arrays(counts.data(), uint32_t(counts.size()), quantum, unit, out.data(), 8, &nb, &used, &err) ==
          RT_ERR_INVALID_ARGUMENT);
    CHECK(nb == 0xdeadu && used == 0xdeadu && std::all_of(out.begin(), out.end(), [](uint32_t v) { return v == 0xdeadu; }));
}

int main() {
    const std::vector<uint32_t> example = {0, 1, 2, 7, 8, 64, 64, 3, 0, 0, 5, 12, 12, 1, 2, 2, 9, 9, 9, 30, 0, 64, 7, 8};
    for (uint32_t unit : {1u, 3u, 5u, 64u, sm::kMaxUnit}) expect_ok(example, 0, unit, unit);
    expect_ok(example, 0, 0, 32);
    expect_ok(example, 16, 0, 32);
    expect_ok(example, 16, 5, 5);
    expect_ok({7}, 0, 3, 3);
    expect_ok({0}, 0, 0, 32);
    expect_ok({}, 0, 0, 32);
    expect_ok({}, 0, 9, 9);
    expect_ok(std::vector<uint32_t>(24, 0u), 0, 1, 1);
    expect_ok({3, sm::kMaxCount, 0}, 0, 4096, 4096);
    expect_ok({3, sm::kMaxCount, 0}, 0, 0, 128);       // the floor's upper clamp
    expect_ok(std::vector<uint32_t>(24, 2048u), 0, 0, 64);
    {   // 72 tiles with 71 distinct counts: the level plan refuses them, the block plan does not
        std::vector<uint32_t> c(72);
        for (uint32_t t = 0; t < 72; t++) c[t] = 1u + (29u * t) % 71u;
        sm::Plan p;
        std::string err;
        CHECK(sm::make_plan(c.data(), 72, 0, p, &err) == RT_ERR_INVALID_ARGUMENT && err.find("71 levels") != std::string::npos);
        CHECK(sm::make_plan_any_levels(c.data(), 72, 0, p, &err) == RT_OK && p.levels.size() == 71u && p.level_tiles.size() == 71u);
        CHECK(p.levels.front() == 1u && p.levels.back() == 71u && p.level_tiles.front() == 72u && p.level_tiles.back() == 1u);
        expect_ok(c, 0, 0, 32);
        expect_ok(c, 0, 1, 1);
        expect_ok(c, 0, 5, 5);
    }
    {
        uint32_t s = 12345u;   // a seeded table of 1 000 tiles
        std::vector<uint32_t> c(1000);
        for (uint32_t& v : c) {
            s = s * 1664525u + 1013904223u;
            v = (s >> 20) % 301u;
        }
        expect_ok(c, 0, 7, 7);
        expect_ok(c, 3, 40, 40);
        expect_ok(c, 0, 0, 32);
    }
    {   // the automatic unit above its floor: 32 400 tiles of 10 000 samples
        sm::Plan p;
        std::vector<uint32_t> c(32400, 10000u);
        CHECK(sm::make_plan_any_levels(c.data(), 32400, 0, p, nullptr) == RT_OK);
        CHECK(sm::auto_unit(p) == 412u);
        CHECK(sm::count_blocks(p, 412u) == 32400u * 25u);
    }
    expect_refused({3, 7, sm::kMaxCount + 1, 0xffffffffu}, 0, 0, "tile_counts[2]");
    expect_refused({5, sm::kMaxCount - 1}, 3, 0, "tile_counts[1]");
    expect_refused({5, 6}, 0, sm::kMaxUnit + 1, "unit_samples");
    expect_refused({5, 6}, 0, 0xffffffffu, "unit_samples");
    {   // 64 tiles of 2^19 samples: 2^25 blocks at U = 1 (one too many), 2^24 at U = 2, 2^18 at the automatic 128
        const std::vector<uint32_t> c(64, sm::kMaxCount);
        expect_refused(c, 0, 1, "unit_samples that fits is 2");
        uint64_t nb = 0;
        uint32_t used = 0;
        CHECK(sm::block_plan_arrays(c.data(), 64, 0, 0, nullptr, 0, &nb, &used, nullptr) == RT_OK);
        CHECK(used == 128u && nb == (1u << 18) && nb <= sm::kMaxBlocks);
        CHECK(sm::block_plan_arrays(c.data(), 64, 0, 2, nullptr, 0, &nb, &used, nullptr) == RT_OK);
        CHECK(used == 2u && nb == (1u << 24));
    }
    {   // NULL table
        sm::BlockPlan bp;
        std::string err;
        CHECK(sm::make_block_plan(nullptr, 3, 0, 0, bp, &err) == RT_ERR_INVALID_ARGUMENT && err.find("NULL") != std::string::npos);
        CHECK(sm::make_block_plan(nullptr, 0, 0, 0, bp, &err) == RT_OK && bp.blocks.empty() && bp.unit_samples == 32u);
        CHECK(sm::block_plan_arrays(nullptr, 3, 0, 0, nullptr, 0, nullptr, nullptr, nullptr) == RT_ERR_INVALID_ARGUMENT);
    }
    if (g_failed) {
        std::fprintf(stderr, "%d of %d checks FAILED\n", g_failed, g_checks);
        return 1;
    }
    std::printf("sample_map_blocks: %d checks passed (ASan + UBSan)\n", g_checks);
    return 0;
}
