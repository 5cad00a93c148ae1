// rt_sample_map.h — the plan of a sample-map frame as host data (no HIP): from a
// table of per-tile sample counts, the quantised table, the tile order (count descending, tile index
// ascending), the distinct non-zero counts L_0 < ... < L_{J-1} and the prefix lengths c_j = #{t :
// n[t] >= L_j}. Launch j of the frame renders samples [L_{j-1}, L_j) on the first c_j tiles of the
// order. Plain C++ so that the CPU tests (rt_sample_map_plan) and the sanitizer build
// (tests/native/sample_map_plan_main.cpp) exercise exactly the code the set calls of rt_api.cpp run.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_mi355x.h"

namespace rt {
namespace sample_map {

constexpr uint32_t kMaxLevels = RT_SAMPLE_MAP_MAX_LEVELS;   // = the launches rt_launch_ms keeps
constexpr uint32_t kMaxCount = 1u << 19;                    // = kHashMaxSpp

struct Plan {
    std::vector<uint32_t> quantised;     // per tile: its count rounded up to the quantum
    std::vector<uint32_t> order;         // rank -> tile
    std::vector<uint32_t> levels;        // L_j, ascending
    std::vector<uint32_t> level_tiles;   // c_j, descending
};

// The plan of `n_tiles` counts. quantum 0 or 1: none; else every non-zero count is rounded up to a
// multiple of it first. RT_OK, or RT_ERR_INVALID_ARGUMENT with *err (optional) naming the cause: a
// NULL table of n_tiles > 0, the first tile whose count (before or after the quantum) exceeds 2^19,
// more than kMaxLevels distinct non-zero counts. A refusal leaves `p` as it was.
int make_plan(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, Plan& p, std::string* err);

// The totals of a plan over a band of band_w x band_h texels (its tiles row-major, ceil(band_w / 8)
// per tile row): `samples` counts the in-band pixels of ragged edge tiles only. The plan must hold
// ceil(band_w / 8) * ceil(band_h / 8) tiles (RT_ERR_INVALID_ARGUMENT otherwise).
int totals(const Plan& p, uint32_t band_w, uint32_t band_h, rt_sample_map_info* out, std::string* err);

// make_plan into caller arrays (rt_sample_map_plan): order and quantised hold n_tiles words, levels
// and level_tiles kMaxLevels; every output may be NULL. Nothing is written on a refusal.
int plan_arrays(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, uint32_t* order, uint32_t* levels,
                uint32_t* level_tiles, uint32_t* n_levels, uint32_t* quantised, std::string* err);

}  // namespace sample_map
}  // namespace rt
