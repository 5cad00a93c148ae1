// rt_sample_map.h — the plan of a sample-map frame as host data (no HIP): from a
// table of per-tile sample counts, the quantised table, the tile order (count descending, tile index
// ascending), the distinct non-zero counts L_0 < ... < L_{J-1} and the prefix lengths c_j = #{t :
// n[t] >= L_j}. Launch j of the frame renders samples [L_{j-1}, L_j) on the first c_j tiles of the
// order. Plain C++ so that the CPU tests (rt_sample_map_plan) and the sanitizer build
// (tests/native/sample_map_plan_main.cpp) exercise exactly the code the set calls of
// rt_sample_map_frame.cpp run.
// The one-launch schedule (RT_SAMPLE_MAP_ONE_LAUNCH) renders the same table from a block table
// instead: make_block_plan below.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_sample_map_device.h"

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

// ---- the one-launch schedule: a block table ---------------------------------
// The tiles in `order`, those of count 0 dropped; a tile of count n in k = ceil(n / U) chunks, chunk
// c = samples [c n / k, (c + 1) n / k) (64-bit arithmetic): the chunks partition [0, n) in order and
// each holds 1 .. U samples. The table is the chunks tile by tile, chunk ascending, one 16-byte entry
// per block of 64 units (rt_internal.h BlockEntry has this layout). The high-count tiles' ~U-sample
// units lead, the single short units of the low-count tiles are the tail.
struct Block {
    uint32_t tile, s0, s1, zero;
};
constexpr uint32_t kMaxUnit = kMaxCount;            // a unit longer than the largest count changes nothing
constexpr uint64_t kMaxBlocks = (1ull << 25) - 1u;  // unit ids in 32 bits: 64 n_blocks < 2^31
// The automatic unit length is sized for this many lanes: 256 CUs x 1536, the resident lanes of the
// shipped walk forms (two blocks of 768) on a full MI355X. Nominal: the plan is host data and the
// same on every device; a partitioned or smaller device gets somewhat more units per lane.
constexpr uint64_t kNominalLanes = 256u * 1536u;

struct BlockPlan {
    Plan plan;                  // as make_plan's, but `levels` / `level_tiles` hold every distinct count
    uint32_t unit_samples = 0;  // U
    uint32_t live_tiles = 0;    // tiles of count > 0
    std::vector<Block> blocks;
};

// make_plan without the limit on levels.
int make_plan_any_levels(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, Plan& p, std::string* err);

// U of a plan when the caller passes 0: max(floor, ceil(sum_t 64 n[t] / (kNominalLanes * 128))) with
// floor = clamp(max_count / 32, 32, 128), the targets of the uniform launches' chunk rule
// (rt_launch.cpp uniform_chunks: ~128 units per lane, units of >= spp / 32 samples between 32 and
// 128) applied to the frame's total samples; doubled until the table has at most kMaxBlocks blocks.
uint32_t auto_unit(const Plan& p);

// Blocks of a plan at unit length U >= 1.
uint64_t count_blocks(const Plan& p, uint32_t unit);

// The block plan of `n_tiles` counts. unit_samples 0: auto_unit; else 1 .. kMaxUnit. Refusals
// (RT_ERR_INVALID_ARGUMENT, `bp` left as it was): make_plan's but the level limit, a unit above
// kMaxUnit, a caller's unit whose table exceeds kMaxBlocks (the message names the smallest unit
// that fits), a table no unit fits.
int make_block_plan(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, uint32_t unit_samples,
                    BlockPlan& bp, std::string* err);

// make_block_plan into caller arrays (rt_sample_map_block_plan): blocks_out holds 4 words per block,
// `capacity` blocks (fewer than the plan's: refused, the message names the count); every output may be
// NULL (blocks_out NULL: a size query). Nothing is written on a refusal.
int block_plan_arrays(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, uint32_t unit_samples,
                      uint32_t* blocks_out, uint64_t capacity, uint64_t* n_blocks, uint32_t* unit_samples_used,
                      std::string* err);

// ---- maps planned on the device (rt_sample_map_set_device_async, rt_sample_map_plan.hip) ---------
// The unit the device planner chooses for a table (rt_sample_map_device.h): the smallest U0 2^j, held
// at 2^19, whose block table of the counts clamped to count_cap has at most `capacity` entries; the
// table is then make_block_plan's of the clamped counts at that unit. Refusals
// (RT_ERR_INVALID_ARGUMENT, nothing written): a NULL table, a cap or unit above 2^19, more non-zero
// tiles than the capacity (no unit fits).
int device_unit(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t count_cap, uint32_t unit_samples,
                uint64_t capacity, uint32_t* unit_used, uint64_t* n_blocks, std::string* err);

}  // namespace sample_map
}  // namespace rt
