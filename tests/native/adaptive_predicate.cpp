// adaptive_predicate.cpp — stand-alone check of the adaptive stop criterion's host form
// (csrc/rt_adaptive.h) against unsigned __int128 arithmetic, meant for a sanitizer build:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tests/native/adaptive_predicate.cpp -o adaptive_predicate && ./adaptive_predicate
//
// Host only: no device, no library. Exit status 0 and "ok" when every case agrees.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_adaptive.h"

static bool wide(uint64_t E, uint64_t S, uint32_t n, uint32_t m, uint32_t thr) {
    const unsigned __int128 s1 = (unsigned __int128)S + ((unsigned __int128)n * 3u * m << 16);
    return ((unsigned __int128)E << 17) < (unsigned __int128)thr * s1;
}

static unsigned long g_cases = 0, g_bad = 0;

static void check(uint64_t E, uint64_t S, uint32_t n, uint32_t m, uint32_t thr) {
    g_cases++;
    if (rt::adaptive_tile_converged(E, S, n, m, thr) != wide(E, S, n, m, thr)) {
        if (g_bad++ < 10)
            std::fprintf(stderr, "mismatch: E=%llu S=%llu n=%u m=%u thr=%u\n", (unsigned long long)E,
                         (unsigned long long)S, n, m, thr);
    }
}

int main() {
    const uint32_t thrs[] = {0u, 1u, 13107u, 65535u, 65536u, 1u << 20, 0xffffffffu};
    const uint32_t ms[] = {1u, 27u, 64u};
    const uint32_t ns[] = {2u, 8u, 64u, 1u << 19};
    const uint64_t top = rt::kAdaptiveMaxSum - 1;
    for (uint32_t thr : thrs)
        for (uint32_t m : ms)
            for (uint32_t n : ns) {
                const uint64_t guard = uint64_t(n) * 3u * m << 16;
                for (uint64_t S : {uint64_t(0), uint64_t(1), (uint64_t(1) << 32) - 1, uint64_t(1) << 32,
                                   (uint64_t(1) << 50) - 1, top}) {
                    // E around thr * S' / 2^17, and at the ends of its range
                    const unsigned __int128 edge = (unsigned __int128)thr * ((unsigned __int128)S + guard) >> 17;
                    const uint64_t e0 = edge > top ? top : uint64_t(edge);
                    for (int d = -2; d <= 2; d++) {
                        const uint64_t E = d < 0 && e0 < uint64_t(-d) ? 0 : e0 + d > top ? top : e0 + d;
                        check(E, S, n, m, thr);
                    }
                    check(0, S, n, m, thr);
                    check((uint64_t(1) << 50) - 1, S, n, m, thr);
                    check(top, S, n, m, thr);
                }
            }
    std::mt19937_64 rng(12345);
    for (int i = 0; i < 200000; i++) {
        const uint64_t S = rng() >> (8 + rng() % 50), E = rng() >> (8 + rng() % 50);
        check(E, S, uint32_t(2 * (1 + rng() % (1u << 18))), uint32_t(1 + rng() % 64), uint32_t(rng() >> (32 + rng() % 32)));
    }
    std::printf("%s: %lu cases, %lu mismatches\n", g_bad ? "FAILED" : "ok", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
