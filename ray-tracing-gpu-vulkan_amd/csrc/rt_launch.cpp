// rt_launch.cpp — the single-device launch plan (rt_launch.h): host-only C++.
#include "rt_launch.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rt {
namespace launch {

namespace {
// LDS budget of the staged forms: 160 KiB per CU, one 1024-thread block per CU; 4 KiB kept free.
constexpr size_t kMaxLdsBytes = 156 * 1024;
// ... and of a form that must keep two 768-thread blocks per CU (static + dynamic LDS).
constexpr size_t kTwoBlockLdsBytes = 78 * 1024;
// The LDS walk's leaf words hold a leaf index in 10 bits (<= 4096 slots of 4) and an escape node
// of the 8 copies in 19 bits.
constexpr uint32_t kMaxLdsLeafSlots = 4096;
constexpr uint32_t kMaxLdsNodes = 0x7fffeu / 8u;

const struct { const char* name; double Tuning::*field; } kKeys[] = {
    {"grid", &Tuning::grid}, {"grid_scale", &Tuning::grid_scale}, {"grid_coop", &Tuning::grid_coop},
    {"grid_cq", &Tuning::grid_cq},
    {"grid_rec", &Tuning::grid_rec}, {"grid_full_slack", &Tuning::grid_full_slack},
    {"units_per_lane", &Tuning::units_per_lane}, {"unit_min_samples", &Tuning::unit_min_samples},
    {"sample_chunks", &Tuning::sample_chunks}, {"head_chunks", &Tuning::head_chunks},
    {"tail_tiles_pm", &Tuning::tail_tiles_pm}, {"schedule", &Tuning::schedule},
    {"refill_reserve", &Tuning::refill_reserve}, {"isolate_tiles", &Tuning::isolate_tiles},
    {"sah_knobs", &Tuning::sah_knobs}};
static_assert(sizeof(kKeys) / sizeof(kKeys[0]) == kTuningKeys, "one key per Tuning field");
static_assert(sizeof(Tuning) == kTuningKeys * sizeof(double), "Tuning is its doubles");
static_assert(sizeof(Inputs) == 70 * 4 + (7 + kTuningKeys) * 8, "Inputs: 4-byte words, then doubles");
static_assert(sizeof(Plan) == 22 * 4 + 4 * 8, "Plan: 4-byte words, then doubles");

int table_occupancy(void* user, uint32_t accel, bool count, int mode, bool flat, size_t lds, bool) {
    const Inputs& in = *static_cast<const Inputs*>(user);
    const uint32_t flags = (count ? 1u : 0u) | (uint32_t(mode) << 1) | (flat ? 4u : 0u);
    for (uint32_t i = 0; i < in.n_occ && i < kOccRows; i++) {
        const OccRow& r = in.occ[i];
        if ((r.accel == 0u || r.accel == accel) && (r.flags == 0xffffffffu || r.flags == flags) && lds >= r.lds_lo &&
            lds <= r.lds_hi)
            return r.blocks > 0x7fffffffu ? -1 : int(r.blocks);
    }
    return -1;
}
bool table_flat(void* user, const Inputs&, uint32_t, bool) { return static_cast<const Inputs*>(user)->flat_grid != 0; }
uint32_t table_block(void* user, uint32_t accel) {
    const Inputs& in = *static_cast<const Inputs*>(user);
    return accel == ACCEL_BRUTE ? in.block_brute : in.block_walk;
}
}  // namespace

double Tuning::*tuning_field(const char* key) {
    for (const auto& k : kKeys)
        if (std::strcmp(k.name, key) == 0) return k.field;
    return nullptr;
}
const char* tuning_key(uint32_t index) { return index < kTuningKeys ? kKeys[index].name : nullptr; }

bool tuning_value_ok(double value) { return (value >= 0.0 && value <= 4294967296.0) || value == Tuning::kUnset; }

Device table_device(const Inputs& in) {
    return Device{const_cast<Inputs*>(&in), table_occupancy, table_flat, table_block};
}

bool grid_walk(uint32_t accel) {
    return accel == ACCEL_GRID || accel == ACCEL_GRID_GLOBAL || accel == ACCEL_GRID_COOP ||
           accel == ACCEL_GRID_GLOBAL_COOP || accel == ACCEL_GRID_REC || accel == ACCEL_GRID_CQ ||
           accel == ACCEL_GRID_REC_CQ;
}

void size_lds_forms(const Inputs& in, Plan& p) {
    const size_t tree = size_t(2 * in.n_nodes + in.n_leaf + (in.n_leaf + 3) / 4) * 16;
    const size_t lds1 = tree;   // shading records stay in HBM (rt_kernels.hip rt_trace_lds_kernel)
    const bool ok = in.n_nodes && in.n_leaf <= kMaxLdsLeafSlots && in.n_nodes <= kMaxLdsNodes;
    p.lds1_bytes = (ok && lds1 <= kMaxLdsBytes) ? lds1 : 0;
    const size_t oct = lds1 + size_t(14u) * in.n_nodes * 16u;
    p.oct_bytes = (ok && oct <= kMaxLdsBytes) ? oct : 0;
    const uint32_t n_refs = in.grid_n_refs;
    const size_t grid = (size_t(n_refs) + (n_refs + 3) / 4 + (size_t(in.grid_n_cells) + 4) / 4) * 16;
    p.grid_bytes = (n_refs && grid + rt::kLaneSumLdsBytes <= kMaxLdsBytes) ? grid : 0;
}

// Kernel form of a launch (rt_internal.h ACCEL_*) and its dynamic LDS bytes. form =
// options.reserved[1] (A/B and tests, 0 = automatic): 6 one LDS node copy, 8 octant copies, 10
// every node from L2, 12 the grid, 14 the grid with the wave-cooperative walk, 16 the grid in LDS
// with the wave-wide candidate queue; cam_r = the camera's distance from the origin (the grid's
// margin covers cameras within its pad radius).
uint32_t choose_accel(const Inputs& in, const Plan& p, bool brute, uint32_t form, float cam_r, size_t* lds_out) {
    const Tuning& tu = in.tune;
    uint32_t accel;
    size_t lds = 0;
    if (brute) {
        accel = rt::ACCEL_BRUTE;
    } else if (in.has_grid && cam_r <= float(in.grid_pad_radius) &&
               (form == 12u || form == 14u || form == 16u || (form == 0u && (p.grid_bytes || !p.oct_bytes)))) {
        // the grid: staged in LDS when it fits (config 3: 1 % faster than the
        // octant tree), else the octant tree when that fits LDS (a device-built scene of ~1000
        // spheres, whose grid would be read from L2), else the grid from L2
        accel = p.grid_bytes ? rt::ACCEL_GRID : rt::ACCEL_GRID_GLOBAL;
        lds = p.grid_bytes;   // 0: the grid from L2
        // the wave-cooperative walk: form 14, or tuning grid_coop = 1
        const bool coop = form == 14u || (form == 0u && Tuning::get(tu.grid_coop, 0) == 1);
        if (coop && accel == rt::ACCEL_GRID &&
            p.grid_bytes + rt::kLaneSumLdsBytes + rt::kCoopLdsBytes <= kMaxLdsBytes)
            accel = rt::ACCEL_GRID_COOP;
        else if (coop && accel == rt::ACCEL_GRID_GLOBAL)
            accel = rt::ACCEL_GRID_GLOBAL_COOP;
        // the LDS grid kernel also stages the winner's gate and shading records ({c, r} + the
        // material record, 48 B per sphere) when two blocks per CU still fit;
        // tuning grid_rec = 0: not (A/B)
        // (the kernel's static table of kRecStatic records: scenes of at most that many spheres)
        const size_t rec_bytes = in.n_spheres <= rt::kRecStatic ? size_t(rt::kRecStatic) * 48u : kMaxLdsBytes;
        // the wave-wide candidate queue: form 16, or tuning grid_cq = 1
        const bool cq = accel == rt::ACCEL_GRID && (form == 16u || (form == 0u && Tuning::get(tu.grid_cq, 0) == 1));
        const size_t cq_bytes = cq ? rt::kCqLdsBytes : 0u;
        if (accel == rt::ACCEL_GRID && Tuning::get(tu.grid_rec, 1) != 0 &&
            p.grid_bytes + rec_bytes + rt::kLaneSumLdsBytes + cq_bytes <= kTwoBlockLdsBytes) {
            accel = cq ? rt::ACCEL_GRID_REC_CQ : rt::ACCEL_GRID_REC;
            lds = p.grid_bytes;   // (the records: static LDS of the kernel)
        } else if (cq && p.grid_bytes + rt::kLaneSumLdsBytes + cq_bytes <= kMaxLdsBytes) {
            accel = rt::ACCEL_GRID_CQ;
        }
    } else if (p.oct_bytes && (form == 0u || form == 8u)) {
        accel = rt::ACCEL_LBVH_OCT;
        lds = p.oct_bytes;
    } else if (p.lds1_bytes && (form == 0u || form == 6u || form == 8u)) {
        accel = rt::ACCEL_LBVH_LDS;
        lds = p.lds1_bytes;
    } else if (in.gpu_tree && in.has_treelet && in.n_nodes && in.n_leaf < (1u << 26) && form != 10u) {
        // (treelet leaf words carry first_count in 30 bits)
        accel = rt::ACCEL_LBVH_TOP;
        lds = size_t(rt::kTreeletCap) * 32u;
    } else {
        accel = rt::ACCEL_LBVH_GLOBAL;
    }
    *lds_out = lds;
    return accel;
}

int plan_form(const Inputs& in, const Device& dev, Plan& p, const char** err) {
    p = Plan{};
    p.bytes = uint32_t(sizeof(Plan));
    {   // no split of this band's tiles has unit ids of 32 bits (split_units): refused before the
        // caller sizes anything by it
        const uint64_t tiles_x = (in.band_w + 7u) / 8u, tiles_y = (in.band_h + 7u) / 8u;
        if (tiles_x * tiles_y * 64u >= (1ull << 32)) {
            *err = "band too large";
            return RT_ERR_INVALID_ARGUMENT;
        }
    }
    size_lds_forms(in, p);
    const int mode = in.rng_mode == RT_RNG_SAMPLE_HASH ? rt::MODE_HASH : rt::MODE_STREAM;
    // the binary32 values the slack is computed in
    const float small_rmax = float(in.small_rmax), small_rmin = float(in.small_rmin);
    // reserved[1] (internal, A/B only): walk form, 0 = automatic (choose_accel)
    size_t lds = 0;
    const uint32_t accel = choose_accel(in, p, in.accel == RT_ACCEL_BRUTE, in.reserved1, float(in.cam_r), &lds);
    const bool count = (in.reserved0 & 1u) != 0;  // internal: count box / sphere tests
    // Node-cull slack: a candidate's AABB entry lies at most
    // 2.75 r + 1.15e-3 t beyond its reported t.
    p.cull_abs = 3.0f * small_rmax + 1e-3f;
    p.cull_rel = 2e-3f;
    // Grid walks: the r-term of the slack is there for quadratic false positives
    // (computed D >= 0, the line passing eps_d <= 7 u |oc|^2 / r outside the sphere, u = 2^-24)
    // whose AABB entry lies up to ~1.42 r past t. The grid registers a sphere in every cell its AABB
    // widened by 64 u R + 1e-3 cell overlaps; the 1e-3-cell part is spare (64 u R covers the DDA's
    // rounding), so while eps_d <= 1e-3 cell the cell holding the ray's closest approach, reached by
    // best + 1e-3 + 2e-3 best, already references the sphere. eps_d <= 1e-3 cell holds for |oc| <= T
    // = sqrt(1e-3 cs r_min / 7u) (3/4 of that budget below), and t <= 0.95 T - r_max - 1e-3 cs implies
    // |oc| <= T. The reported
    // t lies within 9.1e-4 |oc| (sqrt of D's error, 14 u |oc|^2) of the true or closest-approach t.
    p.cull_near_t = -1.0f;
    p.cull_near_abs = p.cull_abs;
    if (grid_walk(accel) && small_rmin > 0.0f && std::isfinite(small_rmin)) {
        const double m = RT_GRID_SPARE * std::min<double>(float(in.grid_cs[0]),
                                                          std::min<double>(float(in.grid_cs[1]), float(in.grid_cs[2])));
        // budget: 3/4 of the spare part for eps_d, 1/4 for a walk that starts (at tmin) up to
        // 9.1e-4 |oc| ~ 9.1e-4 (r + tmin) past a closest approach just behind tmin
        const double T = std::sqrt(0.75 * m * double(small_rmin) / (7.0 * 0x1p-24));
        const double tn = 0.95 * T - double(small_rmax) - m;
        const bool start_ok = 9.1e-4 * (double(small_rmax) + 1e-3) <= 0.25 * m;
        if (tn > 0.0 && start_ok && Tuning::get(in.tune.grid_full_slack, 0) == 0) {   // grid_full_slack: A/B only
            p.cull_near_t = float(tn);
            p.cull_near_abs = 1e-3f + 1e-3f * small_rmax;   // covers 9.1e-4 (r + eps_d) of |oc| - t
        }
    }
    // The row map of a banded launch (N > 1 strips) is staged in the walk kernels' dynamic LDS
    // after their own data (band_row, rt_trace_units.h) when that keeps the blocks per CU; else it
    // is read from global memory.
    uint32_t rows_lds = rt::kNoRowsLds;
    const bool flat = dev.flat_grid_form(dev.user, in, accel, count);   // the kernel launch_trace picks
    if (in.has_rows && accel != rt::ACCEL_BRUTE) {
        const size_t off = (lds + 15) & ~size_t(15), with = off + size_t(in.band_h) * 4u;
        int b0 = 0, b1 = 0;
        if (with <= kMaxLdsBytes && (b0 = dev.occupancy(dev.user, accel, count, mode, flat, lds, true)) >= 0 &&
            (b1 = dev.occupancy(dev.user, accel, count, mode, flat, with, true)) >= 0 && b1 >= b0 && b1 > 0) {
            rows_lds = uint32_t(off);
            lds = with;
        }
    }
    // Grid: one persistent block per CU slot the occupancy allows.
    const int b = dev.occupancy(dev.user, accel, count, mode, flat, lds, false);
    if (b < 0) {
        *err = "occupancy query failed";
        return RT_ERR_DEVICE;
    }
    p.blocks_per_cu = uint32_t(std::max(1, b));
    p.accel = accel;
    p.count = count;
    p.flat = flat;
    p.mode = uint32_t(mode);
    p.lds = uint32_t(lds);
    p.rows_lds = rows_lds;
    p.block = dev.block_size(dev.user, accel);
    return 0;
}

namespace {
// Sample chunks per pixel (HASH only: the image does not depend on them):
// enough units for ~128 per lane, but units of at least 256 samples, so the frame is
// throughput-bound and its tail (the units running when the queue runs dry, about one unit
// long) short, without paying a unit's start and flush too often (config 3,
// 10 000 spp, 4 -> 25 chunks -2.0 %; config 5, 1000 spp 4K: 1 / 3 / 7 / 14 chunks 658.6 /
// 655.3 / 666.0 / 685.9 ms). Tuning sample_chunks forces a count, units_per_lane /
// unit_min_samples set the targets. The brute-force walk's samples cost ~n/10 times a grid
// sample, so its floor scales down with n (488 spheres: 5 samples; config 2, 100 spp: 1 -> 20
// chunks).
// `pixels` / `n_tiles`: the pixels and 8x8 tiles the launch hands out (the band's, or those of an
// adaptive pass's tile list).
uint64_t uniform_chunks(const Inputs& in, const Plan& p, uint32_t spp, uint64_t pixels, uint64_t n_tiles,
                        bool* forced) {
    const int mode = int(p.mode);
    const uint32_t accel = p.accel;
    const uint64_t lanes = uint64_t(in.cu_count) * p.blocks_per_cu * p.block;
    uint64_t chunks = 1;
    *forced = false;
    if (mode == rt::MODE_HASH && spp > 1) {
        // units of >= spp / 32 samples, between 32 and 128 (256 until round 5; 128 for every spp
        // until round 6): a band of the N = 8 frame (135 rows at 10 000 spp) is capped by this
        // floor, not by the lanes, and its 256-sample tail units left a tail after the queue ran
        // dry of 4.9 % of the band; config 5's 270-row band at 1 000 spp had 7
        // chunks of 143 samples under the 128 floor, a 6-7 ms tail of a 68 ms band: 15 chunks
        // (32-sample floor) -1.1 / -2.0 % on two bands, configs 3 / 4 unchanged (10 000 / 32 >
        // 128; profiles/r06d_tune2_*.txt)
        uint64_t per_lane = 128, min_samples = std::min<uint64_t>(128, std::max<uint64_t>(32, spp / 32));
        if (accel == rt::ACCEL_BRUTE) min_samples = std::min<uint64_t>(256, std::max<uint64_t>(4, 2560 / std::max(1u, in.n_spheres)));
        per_lane = std::max<uint64_t>(1, uint64_t(Tuning::get(in.tune.units_per_lane, double(per_lane))));
        min_samples = std::max<uint64_t>(1, uint64_t(Tuning::get(in.tune.unit_min_samples, double(min_samples))));
        chunks = std::min<uint64_t>((lanes * per_lane + pixels - 1) / pixels, std::max<uint64_t>(1, spp / min_samples));
        if (in.tune.sample_chunks != Tuning::kUnset) {
            chunks = uint64_t(in.tune.sample_chunks);
            *forced = true;
        }
        chunks = std::max<uint64_t>(1, std::min<uint64_t>({chunks, spp, 4096}));
        while (chunks > 1 && n_tiles * chunks * 64u >= (1ull << 31)) chunks /= 2;   // unit ids in 32 bits
    }
    return chunks;
}
}  // namespace

int split_units(const Inputs& in, Plan& P, uint32_t spp, uint64_t pixels, uint64_t n_tiles, bool tile_order,
                bool head_tail, const char** err) {
    const int mode = int(P.mode);
    const uint64_t blk = P.block;
    const uint64_t lanes = uint64_t(in.cu_count) * P.blocks_per_cu * blk;
    bool chunks_forced = false;
    uint64_t chunks = uniform_chunks(in, P, spp, pixels, n_tiles, &chunks_forced);
    if (n_tiles * chunks * 64u >= (1ull << 32)) {
        *err = "band too large";
        return RT_ERR_INVALID_ARGUMENT;
    }
    P.chunks = uint32_t(chunks);
    P.lpt = tile_order ? 1u : 0u;
    // Head and tail of the LPT order (HASH): the frame's tail is made of the units
    // still running when the queue runs dry, so only the last ranks (the shortest fifth of the
    // tiles) need short units, 2/5 of `chunks` (the count that keeps a uniform split
    // throughput-bound); the head ranks run longer ones, about 12 per lane (a head unit ~1/12 of
    // the frame, so it ends while the tail runs), and only when that is fewer chunks than the
    // tail's (not at 1080p / 1000 spp, whose uniform units are already that long). Config 3:
    // 25 -> 3 head / 10 tail chunks, config 5: 3 -> 1 / 3. A sixth of the units at config 3, so
    // fewer unit starts and flushes, and fewer 64-bit fixed-point atomics, whose memory-side requests are most of the
    // kernel's HBM traffic: 6.6 -> 0.98 GB per frame at -0.6 % frame time (10 tail chunks; 25:
    // 1.6 GB at -0.9 %; profiles/r03_tail_chunks_traffic.txt). Tuning head_chunks / tail_tiles_pm
    // (tail tiles per mille) override; sample_chunks sets the tail count itself.
    uint64_t head_tiles = 0, head_chunks = chunks;
    if (mode == rt::MODE_HASH && chunks > 1 && tile_order && head_tail) {
        head_chunks = std::max<uint64_t>(1, (12u * lanes + pixels - 1) / std::max<uint64_t>(1, pixels));
        // tail units: at most 2.5x the uniform ones, and at least 3x shorter than the head's
        const uint64_t tail_chunks =
            chunks_forced ? chunks : std::max<uint64_t>((chunks * 2 + 4) / 5, std::min<uint64_t>(chunks, 3 * head_chunks));
        head_chunks = uint64_t(Tuning::get(in.tune.head_chunks, double(head_chunks)));
        // the last 30 % of the tiles (20 % until round 5: the frame's tail after the queue ran
        // dry 25.5 -> 16.4 ms at config 3, -0.7 %; the N = 8 band with 128-sample units -1.8 %)
        const uint64_t tail_pm = uint64_t(Tuning::get(in.tune.tail_tiles_pm, 300));
        head_chunks = std::max<uint64_t>(1, std::min<uint64_t>(head_chunks, tail_chunks));
        const uint64_t tail = std::min<uint64_t>(n_tiles, (n_tiles * std::min<uint64_t>(tail_pm, 1000) + 999) / 1000);
        if (head_chunks < tail_chunks) {
            head_tiles = n_tiles - tail;
            P.chunks = uint32_t(tail_chunks);
        }
    }
    chunks = P.chunks;
    P.head_tiles = uint32_t(head_tiles);
    P.head_chunks = uint32_t(head_tiles ? head_chunks : chunks);
    P.n_units = uint32_t((head_tiles * P.head_chunks + (n_tiles - head_tiles) * chunks) * 64u);
    hand_out_units(in, P, tile_order);
    return 0;
}

uint64_t refill_reserve(const Inputs& in) { return uint64_t(Tuning::get(in.tune.refill_reserve, 8192)); }

void hand_out_units(const Inputs& in, Plan& P, bool tile_order) {
    const int mode = int(P.mode);
    const uint64_t blk = P.block;
    const uint64_t full = uint64_t(in.cu_count) * P.blocks_per_cu;
    const uint64_t by_work = (uint64_t(P.n_units) + blk - 1) / blk;
    const int grid = int(std::max<uint64_t>(1, std::min(full, by_work)));
    P.grid = uint32_t(grid);
    {   // Block hand-out: the last `reserve` units go out one by one. Measured
        // (scripts/refill_ab.py, 1080p): 0 to 32 Ki are within 1 %, one pixel per lane of the
        // grid (262 Ki) is 10-15 % slower at 13-50 spp.
        const uint64_t reserve = refill_reserve(in);
        const rt::HandOut h = rt::hand_out(P.n_units, reserve, uint64_t(grid) * blk / 64u);   // (rt_hand_out.h)
        P.n_block_units = h.n_block_units;
        P.first_blocks = h.first_blocks;
        // A STREAM frame is as long as its longest pixel chain; the waves that
        // start on the longest-chain tiles of the LPT order take no further work, so no refill of
        // their other lanes slows the chain down. 1/512 of the waves (32 on a full MI355X):
        // 12 spp -3.4 %, 50 spp -3 %, 100 spp +-0 (scripts/env_ab.py isolate_tiles). HASH
        // units are short: no isolation.
        const uint64_t iso = uint64_t(Tuning::get(in.tune.isolate_tiles, double(uint64_t(grid) * blk / 64u / 512u)));
        P.isolate_blocks = (tile_order && mode == rt::MODE_STREAM) ? uint32_t(std::min<uint64_t>(P.first_blocks, iso)) : 0u;
    }
}

uint32_t camera_batches(const Inputs& in, const Plan& p, double tune, uint32_t max_depth, bool table,
                        uint32_t static_lds, int kernel_blocks, uint32_t* lds_total) {
    *lds_total = static_lds + p.lds;
    if (Tuning::get(tune, kCameraBatchesDefault) == 0) return BATCH_OFF_TUNE;
    if (p.mode != uint32_t(rt::MODE_HASH)) return BATCH_OFF_STREAM;
    if (table) return BATCH_OFF_TABLE;
    if (p.count) return BATCH_OFF_COUNT;
    if (p.accel != rt::ACCEL_GRID_REC || !p.flat) return BATCH_OFF_FORM;   // (the L2 grid, the trees, brute force,
                                                                           // the A/B forms, a grid of several layers)
    if (!in.pinhole_lf) return BATCH_OFF_PINHOLE;
    if (max_depth > rt::kBatchMaxDepth) return BATCH_OFF_DEPTH;
    if (size_t(static_lds) + p.lds > kTwoBlockLdsBytes || p.blocks_per_cu < 2u) return BATCH_OFF_LDS;
    if (kernel_blocks >= 0 && uint32_t(kernel_blocks) < p.blocks_per_cu) return BATCH_OFF_OCCUPANCY;
    return BATCH_ON;
}

int make_plan(const Inputs& in, const Device& dev, Plan& p, const char** err) {
    if (int rc = plan_form(in, dev, p, err)) return rc;
    const uint64_t tiles_x = (in.band_w + 7u) / 8u, tiles_y = (in.band_h + 7u) / 8u;
    const uint64_t n_tiles = tiles_x * tiles_y;
    const double sched = Tuning::get(in.tune.schedule, 0);
    const bool lpt = sched != 1;
    const bool tile_order = p.accel != rt::ACCEL_BRUTE && lpt && in.lpt_valid;
    return split_units(in, p, in.spp, uint64_t(in.band_w) * in.band_h, n_tiles, tile_order, true, err);
}

void row_weights(const uint32_t* cost, const uint32_t* order, uint32_t n, uint32_t tiles_x, uint32_t band_h,
                 uint32_t head_tiles, uint32_t head_chunks, uint32_t chunks, std::vector<double>& w) {
    // a tile's record is its longest unit chain; x the chunk count of the rank it ran at (the
    // LPT head / tail split) it estimates its longest pixel's chain, the key the LPT order uses
    std::vector<uint32_t> rank;
    if (order && head_tiles) {
        rank.assign(n, 0u);
        for (uint32_t r = 0; r < n; r++)
            if (order[r] < n) rank[order[r]] = r;
    }
    const uint32_t tiles_y = tiles_x ? n / tiles_x : 0;
    std::vector<double> tile_row(tiles_y, 0.0);
    for (uint32_t t = 0; t < n && tiles_x; t++) {
        const double mult = rank.empty() ? 1.0 : double(rank[t] < head_tiles ? head_chunks : chunks);
        if (t / tiles_x < tiles_y) tile_row[t / tiles_x] += double(cost[t]) * mult;
    }
    w.assign(band_h, 0.0);
    for (uint32_t i = 0; i < band_h; i++) {
        const uint32_t ty = i / 8u;
        const uint32_t rows_in = std::min<uint32_t>(8u, band_h - ty * 8u);
        if (ty < tiles_y) w[i] = tile_row[ty] / double(rows_in);
    }
}

}  // namespace launch
}  // namespace rt
