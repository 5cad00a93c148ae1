// rt_adaptive.h — the stop criterion of adaptive frames (rt_render_adaptive_device, DESIGN.md
// §3.1.1): one definition, evaluated by the error kernel (rt_adaptive.hip), by the host export
// rt_adaptive_tile_converged and, through that export, by the tests. Exact integer arithmetic.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RT_ADAPTIVE_HD __host__ __device__
#else
#define RT_ADAPTIVE_HD
#endif

namespace rt {

// Ranges the 128-bit comparison below is exact for (the export refuses anything beyond): a tile's
// sums over m <= 64 pixels x 3 channels of n <= 2^19 samples of at most 2^24 each stay below
// 192 * 2^43 < 2^51; the guard term is at most 2^19 * 3 * 64 * 2^16 < 2^43.
constexpr uint64_t kAdaptiveMaxSum = 1ull << 56;
constexpr uint32_t kAdaptiveMaxSpp = 1u << 19;      // = kHashMaxSpp; any 32-bit thr_q16 is exact

// The tile converges iff 2^17 E < thr_q16 S', strictly, with
//   E  = sum over the tile's m in-band pixels and 3 channels of |A - B| (the two half-buffers),
//   S  = the same sum of A + B,
//   S' = S + n * 3 * m * 2^16 (dark-tile guard: a mean channel level of 1/256 in 8.24).
// Both sides as 128-bit integers in two 64-bit words: the left one exceeds 64 bits (E < 2^51).
RT_ADAPTIVE_HD inline bool adaptive_tile_converged(uint64_t E, uint64_t S, uint32_t n, uint32_t m,
                                                   uint32_t thr_q16) {
    const uint64_t s1 = S + (uint64_t(n) * 3u * m << 16);
    const uint64_t lhs_hi = E >> 47, lhs_lo = E << 17;
    // thr_q16 * s1 by 32-bit halves of s1: p0 = thr * low, p1 = thr * high (each below 2^64)
    const uint64_t p0 = uint64_t(thr_q16) * (s1 & 0xffffffffull);
    const uint64_t p1 = uint64_t(thr_q16) * (s1 >> 32);
    const uint64_t rhs_lo = p0 + (p1 << 32);
    const uint64_t rhs_hi = (p1 >> 32) + (rhs_lo < p0 ? 1u : 0u);
    return lhs_hi < rhs_hi || (lhs_hi == rhs_hi && lhs_lo < rhs_lo);
}

// thr_q16 = uint32(floor(double(threshold) * 65536 + 0.5)); the caller has checked
// 0 <= threshold <= 16.
inline uint32_t adaptive_thr_q16(float threshold) {
    return uint32_t(double(threshold) * 65536.0 + 0.5);
}


// Device state of an adaptive frame (zeroed before pass 0 by launch_adaptive_init).
struct AdaptiveState {
    uint32_t count[2];           // tiles in list[0] / list[1] (the next pass's list is being appended)
    uint32_t capped;             // tiles that reached max_spp unconverged
    uint32_t pad;
    unsigned long long samples;  // sum over stopped tiles of n * in-band pixels
};

struct AdaptiveErrorParams {
    const unsigned long long* a;   // half-buffers: planes r, g, b of `texels` u64 each
    const unsigned long long* b;
    uint64_t texels;
    uint32_t band_w, band_h, tiles_x;
    const uint32_t* list;          // the tiles that just rendered (null: every tile, row-major)
    uint32_t n_list;
    uint32_t n_done;               // samples every listed tile has now
    uint32_t max_spp;
    uint32_t thr_q16;
    uint32_t cur;                  // index of `list`'s count in the state; the next list is cur ^ 1
    uint32_t* tile_n;              // per tile of the band: its sample count
    uint32_t* next_list;
    AdaptiveState* state;
};

// The update of a feedback frame (rt_render_sample_map_feedback_device): per tile,
// from the two half-buffers of a frame whose tile t rendered tile_n[t] samples in two halves, the
// next count by rt::sample_map_feedback_count.
struct FeedbackParams {
    const unsigned long long* a;   // half-buffers, as AdaptiveErrorParams
    const unsigned long long* b;
    uint64_t texels;
    uint32_t band_w, band_h, tiles_x, n_tiles;
    const uint32_t* tile_n;        // per tile: the samples it rendered (even)
    uint32_t thr_q16, min_spp, max_spp;
    uint32_t* next;                // out, per tile
    unsigned long long* tile_error;   // optional out: (E, S) per tile
    unsigned long long* moved;     // += tiles raised | tiles lowered << 32, one atomic per block
};

}  // namespace rt
