// rt_sample_map_device.h — what the device planner of a sample map (rt_sample_map_plan.hip, DESIGN.md
// §3.1.2) shares with the host: the unit rule, the capacity of the block table and the summary the
// planner leaves in device memory. No HIP, integers only: rt_sample_map.cpp's device_unit is the host
// twin of the device's choice and the tests compare the two.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define RT_MAP_DEVICE_HD __host__ __device__
#else
#define RT_MAP_DEVICE_HD
#endif

namespace rt {
namespace sample_map {

constexpr uint32_t kDeviceMaxCount = 1u << 19;          // = kMaxCount = kMaxUnit
constexpr uint32_t kDeviceUnitSteps = 20;               // U0 2^j, j < 20: U0 2^19 >= any count
constexpr uint64_t kDeviceMaxBlocks = 1ull << 22;       // 4 Mi entries, 64 MiB of table

// The first unit the planner tries: the caller's, or the floor of the host's automatic unit from the
// cap (the host rule's other term needs the table's sum, which the host does not know here).
RT_MAP_DEVICE_HD inline uint32_t device_unit0(uint32_t unit_samples, uint32_t count_cap) {
    if (unit_samples) return unit_samples;
    const uint32_t f = count_cap / 32u;
    return f < 32u ? 32u : f > 128u ? 128u : f;
}
// Candidate j: U0 2^j, held at 2^19 (a longer unit changes no table: one block per tile).
RT_MAP_DEVICE_HD inline uint32_t device_unit_step(uint32_t unit0, uint32_t j) {
    const uint64_t u = uint64_t(unit0) << j;
    return u < kDeviceMaxCount ? uint32_t(u) : kDeviceMaxCount;
}
// Entries the block table of a map is allocated for: every tile at the cap in units of U0, at most
// kDeviceMaxBlocks. The planner doubles the unit until the table it builds fits.
RT_MAP_DEVICE_HD inline uint64_t device_capacity(uint64_t n_tiles, uint32_t count_cap, uint32_t unit0) {
    const uint64_t per_tile = (uint64_t(count_cap) + unit0 - 1u) / unit0;
    const uint64_t c = n_tiles * (per_tile ? per_tile : 1u);
    return c < kDeviceMaxBlocks ? c : kDeviceMaxBlocks;
}

// What the planner leaves in device memory (rt_sample_map_get_info / get_schedule copy it back).
struct DeviceSummary {
    uint32_t n_blocks;        // entries of the table (halves mode: of both halves together)
    uint32_t unit_used;       // U
    uint32_t max_count;       // largest clamped count
    uint32_t live_tiles;      // tiles of count > 0
    uint32_t half_blocks;     // halves mode: entries of one half (0 otherwise)
    uint32_t pad;
    unsigned long long samples;                   // sum over tiles of count x in-band pixels
    unsigned long long blocks_at[kDeviceUnitSteps];   // entries the table would have at candidate j
};

// One planner run, every pointer device memory. Scratch: four arrays of n_tiles words and `temp`
// (device_plan_temp_bytes) for the sort and the scan.
struct DevicePlanParams {
    const uint32_t* counts;   // the caller's per-tile counts
    uint32_t n_tiles, band_w, band_h, tiles_x;
    uint32_t count_cap, unit0;
    // Halves mode (feedback frames): every count is rounded up to even, n = 2 h (count_cap is even),
    // and the table is the plan of the h table over [0, h), the A half, followed by the same entries
    // over [h, 2 h), the B half: read as a whole, a block table of [0, n). `capacity` bounds one
    // half; `blocks` holds 3 x capacity entries, the B half once more from entry 2 x capacity, where
    // a launch of that half alone finds it without knowing the A half's size.
    uint32_t halves;
    uint64_t capacity;        // entries the table (halves mode: one half) may have
    uint32_t* order;          // out, n_tiles: rank -> tile
    uint32_t* clamped;        // out, n_tiles: the counts the resolve divides by
    void* blocks;             // out: BlockEntry[capacity]
    DeviceSummary* summary;   // out
    uint32_t *keys, *vals, *keys_sorted, *offsets;
    void* temp;
    uint64_t temp_bytes;
};

}  // namespace sample_map
}  // namespace rt
