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
}  // namespace

int make_plan(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, Plan& p, std::string* err) {
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
            if (n_levels <= kMaxLevels) {
                r.levels.push_back(n);
                r.level_tiles.push_back(i + 1u);
            }
        }
    }
    if (n_levels > kMaxLevels)
        return refuse(err, "the table has " + std::to_string(n_levels) + " levels (distinct non-zero counts), more than " +
                               std::to_string(kMaxLevels) + ": pass a quantum that rounds the counts to fewer");
    std::reverse(r.levels.begin(), r.levels.end());
    std::reverse(r.level_tiles.begin(), r.level_tiles.end());
    p = std::move(r);
    return RT_OK;
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

}  // namespace sample_map
}  // namespace rt
