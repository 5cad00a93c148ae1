// rt_sample_map.cpp — the plan of a sample-map frame (rt_sample_map.h). Host only, no HIP.
#include "rt_sample_map.h"

#include <algorithm>
#include <numeric>

namespace rt {
namespace sample_map {

namespace {
int refuse(std::string* err, const std::string& msg) {
    if (err) *err = msg;
    return RT_ERR_INVALID_ARGUMENT;
}

int plan_levels(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, uint64_t max_levels, Plan& p,
                std::string* err) {
    if (n_tiles != 0 && !tile_counts) return refuse(err, "tile_counts is NULL");
    const uint64_t q = quantum > 1u ? quantum : 1u;
    Plan r;
    r.quantised.resize(n_tiles);
    for (uint32_t t = 0; t < n_tiles; t++) {
        const uint32_t n = tile_counts[t];
        if (n > kMaxCount)
            return refuse(err, "tile_counts[" + std::to_string(t) + "] = " + std::to_string(n) + " is above 2^19");
        const uint64_t up = (uint64_t(n) + q - 1u) / q * q;
        if (up > kMaxCount)
            return refuse(err, "tile_counts[" + std::to_string(t) + "] = " + std::to_string(n) + " rounds up to " +
                                   std::to_string(up) + " with quantum " + std::to_string(quantum) + ", above 2^19");
        r.quantised[t] = uint32_t(up);
    }
    r.order.resize(n_tiles);
    std::iota(r.order.begin(), r.order.end(), 0u);
    std::stable_sort(r.order.begin(), r.order.end(),
                     [&](uint32_t a, uint32_t b) { return r.quantised[a] > r.quantised[b]; });
    // the order runs through the levels from the highest down: a level's prefix ends where its count does
    uint64_t n_levels = 0;
    for (uint32_t i = 0; i < n_tiles; i++) {
        const uint32_t n = r.quantised[r.order[i]];
        if (n == 0u) break;
        if (i + 1u == n_tiles || r.quantised[r.order[i + 1u]] != n) {
            n_levels++;
            if (n_levels <= max_levels) {
                r.levels.push_back(n);
                r.level_tiles.push_back(i + 1u);
            }
        }
    }
    if (n_levels > max_levels)
        return refuse(err, "the table has " + std::to_string(n_levels) + " levels (distinct non-zero counts), more than " +
                               std::to_string(kMaxLevels) + ": pass a quantum that rounds the counts to fewer");
    std::reverse(r.levels.begin(), r.levels.end());
    std::reverse(r.level_tiles.begin(), r.level_tiles.end());
    p = std::move(r);
    return RT_OK;
}
}  // namespace

int make_plan(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, Plan& p, std::string* err) {
    return plan_levels(tile_counts, n_tiles, quantum, kMaxLevels, p, err);
}

int make_plan_any_levels(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, Plan& p, std::string* err) {
    return plan_levels(tile_counts, n_tiles, quantum, ~0ull, p, err);
}

int totals(const Plan& p, uint32_t band_w, uint32_t band_h, rt_sample_map_info* out, std::string* err) {
    if (!out) return refuse(err, "info is NULL");
    const uint64_t tiles_x = (uint64_t(band_w) + 7u) / 8u, tiles_y = (uint64_t(band_h) + 7u) / 8u;
    if (tiles_x * tiles_y != p.quantised.size())
        return refuse(err, "the plan's tile count does not match the band");
    rt_sample_map_info info{};
    info.tiles = uint32_t(p.quantised.size());
    info.levels = uint32_t(p.levels.size());
    info.min_count = p.levels.empty() ? 0u : p.levels.front();
    info.max_count = p.levels.empty() ? 0u : p.levels.back();
    for (uint64_t ty = 0; ty < tiles_y; ty++) {
        const uint64_t h = std::min<uint64_t>(8u, band_h - ty * 8u);
        for (uint64_t tx = 0; tx < tiles_x; tx++) {
            const uint64_t w = std::min<uint64_t>(8u, band_w - tx * 8u);
            info.samples += uint64_t(p.quantised[ty * tiles_x + tx]) * w * h;
        }
    }
    for (uint32_t c : p.level_tiles) info.tile_launches += c;
    *out = info;
    return RT_OK;
}

int plan_arrays(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, uint32_t* order, uint32_t* levels,
                uint32_t* level_tiles, uint32_t* n_levels, uint32_t* quantised, std::string* err) {
    Plan p;
    if (int rc = make_plan(tile_counts, n_tiles, quantum, p, err)) return rc;
    if (order) std::copy(p.order.begin(), p.order.end(), order);
    if (quantised) std::copy(p.quantised.begin(), p.quantised.end(), quantised);
    if (levels) std::copy(p.levels.begin(), p.levels.end(), levels);
    if (level_tiles) std::copy(p.level_tiles.begin(), p.level_tiles.end(), level_tiles);
    if (n_levels) *n_levels = uint32_t(p.levels.size());
    return RT_OK;
}

uint64_t count_blocks(const Plan& p, uint32_t unit) {
    uint64_t n = 0;
    for (uint32_t t : p.order) {
        const uint32_t c = p.quantised[t];
        if (c == 0u) break;   // the order ends with the zero tiles
        n += (uint64_t(c) + unit - 1u) / unit;
    }
    return n;
}

uint32_t auto_unit(const Plan& p) {
    uint64_t total = 0;
    for (uint32_t c : p.quantised) total += 64u * uint64_t(c);
    const uint64_t max_count = p.levels.empty() ? 0u : p.levels.back();
    const uint64_t floor = std::min<uint64_t>(128u, std::max<uint64_t>(32u, max_count / 32u));
    const uint64_t per_unit = kNominalLanes * 128u;
    uint64_t unit = std::max(floor, (total + per_unit - 1u) / per_unit);
    unit = std::min<uint64_t>(unit, kMaxUnit);
    while (unit < kMaxUnit && count_blocks(p, uint32_t(unit)) > kMaxBlocks) unit = std::min<uint64_t>(unit * 2u, kMaxUnit);
    return uint32_t(unit);
}

int make_block_plan(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, uint32_t unit_samples,
                    BlockPlan& bp, std::string* err) {
    if (unit_samples > kMaxUnit)
        return refuse(err, "unit_samples = " + std::to_string(unit_samples) + " is above 2^19");
    BlockPlan r;
    if (int rc = make_plan_any_levels(tile_counts, n_tiles, quantum, r.plan, err)) return rc;
    const uint32_t unit = unit_samples ? unit_samples : auto_unit(r.plan);
    const uint64_t n_blocks = count_blocks(r.plan, unit);
    if (n_blocks > kMaxBlocks) {
        // count_blocks falls as the unit grows: the smallest unit that fits, by bisection
        if (count_blocks(r.plan, kMaxUnit) > kMaxBlocks)
            return refuse(err, "the table has " + std::to_string(count_blocks(r.plan, kMaxUnit)) +
                                   " non-zero tiles: no block table of it has unit ids of 32 bits");
        uint32_t lo = unit, hi = kMaxUnit;   // lo does not fit, hi does
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            (count_blocks(r.plan, mid) > kMaxBlocks ? lo : hi) = mid;
        }
        return refuse(err, "unit_samples = " + std::to_string(unit) + " gives " + std::to_string(n_blocks) +
                               " blocks, more than 2^25 - 1 (unit ids of 32 bits): the smallest unit_samples that fits is " +
                               std::to_string(hi));
    }
    r.unit_samples = unit;
    r.blocks.reserve(size_t(n_blocks));
    for (uint32_t t : r.plan.order) {
        const uint64_t n = r.plan.quantised[t];
        if (n == 0u) break;
        r.live_tiles++;
        const uint64_t k = (n + unit - 1u) / unit;
        for (uint64_t c = 0; c < k; c++) r.blocks.push_back(Block{t, uint32_t(c * n / k), uint32_t((c + 1u) * n / k), 0u});
    }
    bp = std::move(r);
    return RT_OK;
}

int block_plan_arrays(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, uint32_t unit_samples,
                      uint32_t* blocks_out, uint64_t capacity, uint64_t* n_blocks, uint32_t* unit_samples_used,
                      std::string* err) {
    BlockPlan bp;
    if (int rc = make_block_plan(tile_counts, n_tiles, quantum, unit_samples, bp, err)) return rc;
    if (blocks_out && capacity < bp.blocks.size())
        return refuse(err, "capacity " + std::to_string(capacity) + " is below the table's " +
                               std::to_string(bp.blocks.size()) + " blocks");
    if (blocks_out) {
        for (size_t b = 0; b < bp.blocks.size(); b++) {
            const Block& e = bp.blocks[b];
            blocks_out[4u * b] = e.tile;
            blocks_out[4u * b + 1u] = e.s0;
            blocks_out[4u * b + 2u] = e.s1;
            blocks_out[4u * b + 3u] = 0u;
        }
    }
    if (n_blocks) *n_blocks = bp.blocks.size();
    if (unit_samples_used) *unit_samples_used = bp.unit_samples;
    return RT_OK;
}

int device_unit(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t count_cap, uint32_t unit_samples,
                uint64_t capacity, uint32_t* unit_used, uint64_t* n_blocks, std::string* err) {
    if (n_tiles != 0 && !tile_counts) return refuse(err, "tile_counts is NULL");
    if (count_cap > kMaxCount) return refuse(err, "count_cap = " + std::to_string(count_cap) + " is above 2^19");
    if (unit_samples > kMaxUnit)
        return refuse(err, "unit_samples = " + std::to_string(unit_samples) + " is above 2^19");
    const uint32_t unit0 = device_unit0(unit_samples, count_cap);
    uint64_t blocks = 0;
    for (uint32_t j = 0; j < kDeviceUnitSteps; j++) {
        const uint64_t unit = device_unit_step(unit0, j);
        blocks = 0;
        for (uint32_t t = 0; t < n_tiles; t++) blocks += (std::min<uint64_t>(tile_counts[t], count_cap) + unit - 1u) / unit;
        if (blocks <= capacity) {
            if (unit_used) *unit_used = uint32_t(unit);
            if (n_blocks) *n_blocks = blocks;
            return RT_OK;
        }
    }
    return refuse(err, "the table has " + std::to_string(blocks) + " non-zero tiles, more than the capacity " +
                           std::to_string(capacity) + ": no unit fits");
}

}  // namespace sample_map
}  // namespace rt
