// The host-and-device integer rules of device-planned sample maps under
// AddressSanitizer + UndefinedBehaviorSanitizer: the feedback rule (csrc/rt_sample_map_feedback.h),
// the shared block hand-out (csrc/rt_hand_out.h) and the host twin of the device planner's unit
// (csrc/rt_sample_map.cpp device_unit). A stand-alone program: tests/test_sample_map_feedback_native.py
// compiles and runs it; nothing is loaded into python.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_hand_out.h"
#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_sample_map.h"
#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_sample_map_feedback.h"

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

// The criterion with the compiler's 128-bit integers, the rule restated on it.
static bool converged128(uint64_t E, uint64_t S, uint32_t n, uint32_t m, uint32_t thr) {
    const unsigned __int128 lhs = (unsigned __int128)E << 17;
    const unsigned __int128 rhs = (unsigned __int128)thr * ((unsigned __int128)S + (unsigned __int128)n * 3u * m * 65536u);
    return lhs < rhs;
}
static uint32_t rule128(uint64_t E, uint64_t S, uint32_t n, uint32_t m, uint32_t thr, uint32_t lo, uint32_t hi) {
    if (n == 0) return 0;
    if (!converged128(E, S, n, m, thr)) return uint32_t(std::min<uint64_t>(hi, 2ull * n));
    if (converged128(E, S, n, m, thr >> 1)) return std::max<uint32_t>(lo, (n / 2u + 1u) & ~1u);
    return n;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

static void test_rule() {
    const uint32_t counts[] = {0, 2, 4, 6, 10, 16, 30, 32, 62, 64, 1000, 1u << 18, (1u << 19) - 2, 1u << 19};
    for (uint32_t n : counts) {
        // threshold 0 converges nothing, threshold 16 (q16 = 2^20) everything at either level
        CHECK(rt::sample_map_feedback_count(12345, 67890, n, 64, 0, 4, 64) == (n ? std::min<uint64_t>(64, 2ull * n) : 0));
        CHECK(rt::sample_map_feedback_count(1ull << 40, 1ull << 41, n, 64, 16u << 16, 4, 64) ==
              (n ? std::max<uint32_t>(4, (n / 2 + 1) & ~1u) : 0));
        CHECK(rt::sample_map_feedback_count(0, 0, n, 1, 1, 2, 1u << 19) == rule128(0, 0, n, 1, 1, 2, 1u << 19));
    }
    CHECK(rt::sample_map_feedback_count(1, 1, 1u << 19, 64, 0, 2, 1u << 19) == 1u << 19);   // the clamp at the top
    CHECK(rt::sample_map_feedback_count(0, 1, 2, 64, 16u << 16, 2, 64) == 2);               // and at the bottom
    CHECK(rt::sample_map_feedback_count(0, 1, 6, 64, 16u << 16, 2, 64) == 4);               // 3 rounds up to even
    // E, S near 2^56: the two-word compare
    const uint64_t big = (1ull << 56) - 1u;
    for (uint32_t thr : {0u, 1u, 13107u, 65536u, 1u << 17, (1u << 17) + 1u, 1u << 18, 16u << 16, 0xffffffffu})
        for (uint64_t E : std::vector<uint64_t>{big, big - 1u, big / 2u, big / 2u + 1u, 1ull << 47, (1ull << 47) - 1u})
            for (uint64_t S : std::vector<uint64_t>{big, big - 1u, big / 2u, 1ull << 55, 0ull})
                CHECK(rt::sample_map_feedback_count(E, S, 32, 64, thr, 4, 64) == rule128(E, S, 32, 64, thr, 4, 64));
    for (int i = 0; i < 200000; i++) {
        const uint64_t S = rnd() >> (8 + rnd() % 40), E = S ? rnd() % (S + 1u) >> (rnd() % 8) : 0;
        const uint32_t n = 2u * uint32_t(rnd() % (1u << 18)), m = 1u + uint32_t(rnd() % 64), thr = uint32_t(rnd() >> (32 + rnd() % 20));
        const uint32_t lo = 2u + 2u * uint32_t(rnd() % 32), hi = lo + 2u * uint32_t(rnd() % 1000);
        CHECK(rt::sample_map_feedback_count(E, S, n, m, thr, lo, hi) == rule128(E, S, n, m, thr, lo, hi));
    }
}

static void test_hand_out() {
    for (uint32_t blocks : {0u, 1u, 63u, 127u, 128u, 129u, 203u, 1u << 22, (1u << 25) - 1u})
        for (uint64_t reserve : {0ull, 640ull, 8192ull, 1ull << 32, ~0ull})
            for (uint64_t waves : {1ull, 12ull, 6144ull, 1ull << 40}) {
                const uint32_t n_units = blocks * 64u;
                const rt::HandOut h = rt::hand_out(n_units, reserve, waves);
                CHECK(h.n_block_units % 64u == 0 && h.n_block_units <= n_units);
                CHECK(n_units <= reserve ? h.n_block_units == 0 : n_units - h.n_block_units >= reserve && n_units - h.n_block_units < reserve + 64u);
                CHECK(h.first_blocks == std::min<uint64_t>(waves, h.n_block_units / 64u));
            }
    CHECK(rt::hand_out(203u * 64u, 640, 6144).n_block_units == 12352u - 12352u % 64u);
    CHECK(rt::hand_out(203u * 64u, 0, 6144).first_blocks == 203u);
}

static void test_device_unit() {
    std::string err;
    uint32_t unit = 0xdead;
    uint64_t blocks = 0xdead;
    const std::vector<uint32_t> c = {0, 1, 2, 7, 8, 64, 64, 3, 100, 65};   // at cap 64: 64 64 64 64 and the small ones
    auto blocks_at = [&](uint32_t cap, uint32_t u) {
        uint64_t b = 0;
        for (uint32_t x : c) b += (std::min(x, cap) + u - 1) / u;
        return b;
    };
    // no doubling: the capacity of a map of these tiles
    CHECK(sm::device_unit(c.data(), 10, 64, 3, sm::device_capacity(10, 64, 3), &unit, &blocks, &err) == RT_OK);
    CHECK(unit == 3 && blocks == blocks_at(64, 3));
    CHECK(sm::device_unit(c.data(), 10, 64, 0, sm::device_capacity(10, 64, 32), &unit, &blocks, &err) == RT_OK);
    CHECK(unit == 32 && sm::device_unit0(0, 64) == 32 && sm::device_unit0(0, 4096) == 128 && sm::device_unit0(0, 1u << 19) == 128);
    // one doubling, several
    CHECK(sm::device_unit(c.data(), 10, 64, 3, blocks_at(64, 3) - 1, &unit, &blocks, &err) == RT_OK);
    CHECK(unit == 6 && blocks == blocks_at(64, 6));
    CHECK(sm::device_unit(c.data(), 10, 64, 1, 9, &unit, &blocks, &err) == RT_OK);   // nine non-zero tiles
    CHECK(unit == 64 && blocks == 9);
    CHECK(sm::device_unit(c.data(), 10, 1u << 19, 3, 9, &unit, &blocks, &err) == RT_OK);
    CHECK(unit == 192 && blocks == 9);   // 3 * 64 >= 100
    // the hold at 2^19
    const std::vector<uint32_t> top = {1u << 19, (1u << 19) + 5u, 1};
    CHECK(sm::device_unit(top.data(), 3, 1u << 19, 3, 3, &unit, &blocks, &err) == RT_OK);
    CHECK(unit == 1u << 19 && blocks == 3);
    CHECK(sm::device_unit_step(3, 19) == 1u << 19 && sm::device_unit_step(1, 19) == 1u << 19 && sm::device_unit_step(1u << 19, 19) == 1u << 19);
    // refusals leave the outputs alone
    unit = 0xdead;
    blocks = 0xdead;
    CHECK(sm::device_unit(c.data(), 10, 64, 1, 8, &unit, &blocks, &err) == RT_ERR_INVALID_ARGUMENT && err.find("no unit fits") != std::string::npos);
    CHECK(sm::device_unit(nullptr, 10, 64, 1, 100, &unit, &blocks, &err) == RT_ERR_INVALID_ARGUMENT);
    CHECK(sm::device_unit(c.data(), 10, (1u << 19) + 1u, 1, 100, &unit, &blocks, &err) == RT_ERR_INVALID_ARGUMENT);
    CHECK(sm::device_unit(c.data(), 10, 64, (1u << 19) + 1u, 100, &unit, &blocks, &err) == RT_ERR_INVALID_ARGUMENT);
    CHECK(unit == 0xdead && blocks == 0xdead);
    CHECK(sm::device_unit(nullptr, 0, 64, 0, 0, &unit, nullptr, nullptr) == RT_OK && unit == 32);   // an empty table, NULL outputs
    CHECK(sm::device_capacity(24, 64, 3) == 24u * 22u && sm::device_capacity(1u << 20, 1u << 19, 1) == 1u << 22 &&
          sm::device_capacity(24, 0, 32) == 24);
    // the table at the chosen unit is make_block_plan's of the clamped counts
    std::vector<uint32_t> clamped;
    for (uint32_t x : c) clamped.push_back(std::min(x, 64u));
    sm::BlockPlan bp;
    CHECK(sm::device_unit(c.data(), 10, 64, 3, blocks_at(64, 3) - 1, &unit, &blocks, &err) == RT_OK);
    CHECK(sm::make_block_plan(clamped.data(), 10, 0, unit, bp, &err) == RT_OK && bp.blocks.size() == blocks);
}

int main() {
    test_rule();
    test_hand_out();
    test_device_unit();
    if (g_failed) {
        std::fprintf(stderr, "%d of %d checks failed\n", g_failed, g_checks);
        return 1;
    }
    std::printf("%d checks passed (ASan + UBSan)\n", g_checks);
    return 0;
}
