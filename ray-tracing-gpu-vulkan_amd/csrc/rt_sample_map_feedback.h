// rt_sample_map_feedback.h — the rule that turns a tile's measured noise into its next sample count
// (feedback maps): one definition for the update kernel (rt_adaptive.hip), the host
// export rt_sample_map_feedback_count and, through it, the tests. Integers only.
#pragma once

#include "rt_adaptive.h"

namespace rt {

// E, S, n, m: the quantities of adaptive_tile_converged for a tile whose n samples were rendered as
// two halves of n / 2; min_spp and max_spp even, 2 <= min_spp <= max_spp <= 2^19.
//   hot  = the tile misses the threshold:          next = min(max_spp, 2 n)
//   cold = it meets half the threshold:            next = max(min_spp, n / 2 rounded up to even)
//   else                                           next = n
// Noise falls as 1 / sqrt(n): half the samples at half the threshold leave the tile under the
// threshold in expectation, and the band between the two is the rule's hysteresis. n = 0 stays 0 (a
// tile the map leaves out has nothing to measure). Threshold 0 converges nothing (every tile doubles
// up to max_spp); threshold 16 converges every tile at either level (every tile halves down to
// min_spp).
RT_ADAPTIVE_HD inline uint32_t sample_map_feedback_count(uint64_t E, uint64_t S, uint32_t n, uint32_t m,
                                                         uint32_t thr_q16, uint32_t min_spp, uint32_t max_spp) {
    if (n == 0u) return 0u;
    if (!adaptive_tile_converged(E, S, n, m, thr_q16)) {
        const uint64_t up = 2ull * n;
        return up < max_spp ? uint32_t(up) : max_spp;
    }
    if (adaptive_tile_converged(E, S, n, m, thr_q16 >> 1)) {
        const uint32_t down = (n / 2u + 1u) & ~1u;
        return down > min_spp ? down : min_spp;
    }
    return n;
}

}  // namespace rt
