// rt_hand_out.h — the block hand-out of a trace launch as one rule for the host
// plan (rt_launch.cpp hand_out_units) and for the device, which sizes a launch whose block table was
// planned there (rt_frame_kernels.hip rt_tab_size_kernel). No HIP, integers only.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RT_HAND_OUT_HD __host__ __device__
#else
#define RT_HAND_OUT_HD
#endif

namespace rt {

struct HandOut {
    uint32_t n_block_units;   // units [0, n_block_units) go out as whole 64-unit blocks
    uint32_t first_blocks;    // blocks [0, first_blocks) start on wave id = block
};

// The last `reserve` units go out one by one; the block phase ends at a multiple of 64 units; the
// grid's `grid_waves` waves take the first blocks by wave id. A grid sized by the work has at least
// n_units / 64 waves and the full persistent grid is never smaller, so where the work sizes the grid
// both give first_blocks = n_block_units / 64: the device may assume the full grid.
RT_HAND_OUT_HD inline HandOut hand_out(uint32_t n_units, uint64_t reserve, uint64_t grid_waves) {
    HandOut h;
    h.n_block_units = n_units > reserve ? uint32_t((uint64_t(n_units) - reserve) & ~uint64_t(63)) : 0u;
    const uint64_t blocks = h.n_block_units / 64u;
    h.first_blocks = uint32_t(grid_waves < blocks ? grid_waves : blocks);
    return h;
}

// The 16-byte device record a device-sized table launch reads at entry (TraceParams::tab_size).
struct alignas(16) TabSize {
    uint32_t n_units, n_block_units, first_blocks, zero;
};

}  // namespace rt
