// rt_launch.h — the single-device launch plan as host data (no HIP): every host decision that
// shapes a trace launch — the kernel form and its LDS bytes, the cull slack, the sample-chunk rule,
// the head / tail split of the LPT order, the block hand-out — and the per-row weights the
// cross-device balancer reads, as functions of plain inputs. Plain C++ so the CPU tests
// (rt_debug_launch_plan, tests/test_launch_plan.py) and the sanitizer build (tests/native/Makefile
// `sanitize`) exercise exactly the code rt_render_device runs. What only the kernels' translation
// unit knows (the occupancy of a kernel form, its one-layer grid form, its block size) reaches the
// plan through `Device`: rt_api.cpp's fill_trace, which every frame kind goes through, passes the
// real ones (rt_launchers.h), tests pass tables.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_grid.h"
#include "rt_internal.h"

namespace rt {
namespace launch {

// Launch-plan parameters that tests and A/B scripts vary through rt_debug_tune() (per context; the
// shipped defaults are the measured best). None changes an image. The library reads
// no environment variable for them: only RT_RNG (ray_trace) and RT_BVH_BUILD are read, both
// documented.
struct Tuning {
    static constexpr double kUnset = -1.0;
    double grid = kUnset;               // 0: no uniform grid (LBVH walks only)
    double grid_scale = kUnset;         // cell size scale (rt_grid.h kGridCellScale)
    double grid_coop = kUnset;          // 1: the wave-cooperative grid walk
    double grid_cq = kUnset;            // 1: the wave-wide candidate queue in the LDS grid walk (§4.9)
    double grid_rec = kUnset;           // 0: no shading records in the LDS grid kernel's LDS
    double grid_full_slack = kUnset;    // 1: the full cull slack in grid walks
    double units_per_lane = kUnset;     // sample-chunk targets (counter-based stream)
    double unit_min_samples = kUnset;
    double sample_chunks = kUnset;      // forced chunk count (tail count when the LPT order is split)
    double head_chunks = kUnset;        // head / tail split of the LPT order
    double tail_tiles_pm = kUnset;
    double schedule = kUnset;           // 0 LPT (longest unit chain), 1 row-major
    double refill_reserve = kUnset;     // units handed out one by one at the end of the queue
    double isolate_tiles = kUnset;      // reference stream: waves on the first LPT blocks take no more
    double sah_knobs = kUnset;          // host SAH builder variants (rt_bvh.h)
    static double get(double v, double def) { return v == kUnset ? def : v; }
};
// rt_debug_tune: the field of a key (null: unknown key), and the values it accepts: -1 (restore
// the default) or a finite value in [0, 2^32] (the plan casts them to 64-bit integers).
double Tuning::*tuning_field(const char* key);
bool tuning_value_ok(double value);
constexpr uint32_t kTuningKeys = 15;
const char* tuning_key(uint32_t index);

// What the kernels' translation unit answered for one launch (rt_kernels.hip trace_occupancy,
// flat_grid_form, block_size), kept with the inputs so that a plan is recomputable on the host.
// An occupancy row answers a query of form `accel` (0: any), `flags` (count | mode << 1 |
// flat << 2; 0xffffffff: any) and lds_lo <= dynamic LDS bytes <= lds_hi with `blocks` per CU; the
// first matching row counts, a query without one fails.
struct OccRow {
    uint32_t accel, flags, lds_lo, lds_hi, blocks;
};
constexpr uint32_t kOccRows = 8;
constexpr uint32_t kVersion = 1;

// Everything a plan depends on. Flat layout of 4-byte words, then doubles (rt_debug_launch_plan;
// rtvk/abi.py LaunchInputs mirrors it): binary32 values are carried as doubles.
struct Inputs {
    uint32_t version = kVersion;
    uint32_t bytes = 0;                 // sizeof(Inputs)
    // scene summary
    uint32_t n_spheres = 0, n_big = 0, n_nodes = 0, n_leaf = 0;
    uint32_t has_grid = 0, gpu_tree = 0, has_treelet = 0;
    uint32_t grid_n[3] = {0, 0, 0}, grid_n_cells = 0, grid_n_refs = 0;   // the GridInfo words the plan reads
    // device
    uint32_t cu_count = 0;
    // the request
    uint32_t band_w = 0, band_h = 0, spp = 0;
    uint32_t rng_mode = 0, accel = 0;   // rt_options::rng_mode, ::accel
    uint32_t reserved0 = 0, reserved1 = 0;
    uint32_t has_rows = 0;              // a rows map is given
    uint32_t lpt_valid = 0;             // the context holds an LPT order for this band geometry
    uint32_t pinhole_lf = 0;            // TraceParams::pinhole_lf
    // the kernels' answers
    uint32_t block_brute = 0, block_walk = 0;
    uint32_t flat_grid = 0;             // flat_grid_form of the chosen form
    uint32_t n_occ = 0;
    OccRow occ[kOccRows] = {};
    uint32_t pad_ = 0;
    // binary32 values
    double small_rmin = 0.0, small_rmax = 0.0;
    double grid_cs[3] = {0.0, 0.0, 0.0};   // GridInfo::cs
    double grid_pad_radius = 0.0;
    double cam_r = 0.0;                 // the camera's distance from the origin
    Tuning tune;
};

// Everything the launch then uses. Flat layout as Inputs (rtvk/abi.py LaunchPlan).
struct Plan {
    uint32_t version = kVersion;
    uint32_t bytes = 0;                 // sizeof(Plan)
    uint32_t accel = 0;                 // kernel form (rt::ACCEL_*)
    uint32_t count = 0;                 // instrumented build (options.reserved[0] bit 0)
    uint32_t flat = 0;                  // one-layer grid walk
    uint32_t mode = 0;                  // rt::MODE_*
    uint32_t lds = 0;                   // dynamic LDS bytes
    uint32_t rows_lds = kNoRowsLds;     // TraceParams::rows_lds
    uint32_t block = 0, grid = 0;       // block size, grid size
    uint32_t blocks_per_cu = 0;         // occupancy of the form at `lds`
    uint32_t lpt = 0;                   // the tiles go out in the LPT order
    uint32_t chunks = 1, head_tiles = 0, head_chunks = 1, n_units = 0;
    uint32_t n_block_units = 0, first_blocks = 0, isolate_blocks = 0;
    uint32_t lds1_bytes = 0;            // one node copy + leaves + big table (0: no fit)
    uint32_t oct_bytes = 0;             // 8 octant node copies + leaves + big table (0: no fit)
    uint32_t grid_bytes = 0;            // grid references + offsets + big table (0: no grid / no fit)
    double cull_abs = 0.0, cull_rel = 0.0, cull_near_t = 0.0, cull_near_abs = 0.0;   // binary32 values
};

// The kernels' translation unit, as the plan sees it.
struct Device {
    void* user;
    // blocks per CU of a form at `lds` dynamic bytes (< 0: the query failed). probe: a what-if
    // query of the rows-map decision, not the launch's own (which rt_api.cpp caches per context)
    int (*occupancy)(void* user, uint32_t accel, bool count, int mode, bool flat, size_t lds, bool probe);
    bool (*flat_grid_form)(void* user, const Inputs& in, uint32_t accel, bool count);
    uint32_t (*block_size)(void* user, uint32_t accel);
};
// The Device that answers from the tables inside `in` (user = &in).
Device table_device(const Inputs& in);

// true for the forms that walk the uniform grid.
bool grid_walk(uint32_t accel);

// LDS bytes of the staged forms of a scene (Plan::lds1_bytes, oct_bytes, grid_bytes).
void size_lds_forms(const Inputs& in, Plan& p);

// Kernel form of a launch (rt_internal.h ACCEL_*) and its dynamic LDS bytes, from the LDS form sizes
// in `p`.
uint32_t choose_accel(const Inputs& in, const Plan& p, bool brute, uint32_t form, float cam_r, size_t* lds_out);

// First half of a plan, everything that does not depend on how the band's samples are split into
// units: the form, its LDS bytes (with the rows map's place), the cull slack, the block size and
// the occupancy. RT_OK, or RT_ERR_DEVICE when an occupancy query failed and RT_ERR_INVALID_ARGUMENT
// for a band with 2^26 tiles ("band too large"), with *err a static message.
int plan_form(const Inputs& in, const Device& dev, Plan& p, const char** err);

// Second half: the sample chunks, the head / tail split of the LPT order, the grid and the block
// hand-out of one launch of `spp` samples over `pixels` pixels in `n_tiles` 8x8 tiles (the band's,
// or those of an adaptive pass's tile list). tile_order: the tiles go out in a given order;
// head_tail: that order is the LPT order, which may be split. RT_OK, or RT_ERR_INVALID_ARGUMENT
// with *err "band too large".
int split_units(const Inputs& in, Plan& p, uint32_t spp, uint64_t pixels, uint64_t n_tiles, bool tile_order,
                bool head_tail, const char** err);

// The tail of split_units, for any launch whose p.n_units is set (a uniform split's, or 64 x the
// entries of a block table, rt_sample_map.h): the grid size and the block hand-out (n_block_units,
// first_blocks, isolate_blocks; the refill_reserve rule).
void hand_out_units(const Inputs& in, Plan& p, bool tile_order);
// The units handed out one by one at the end of the queue (Tuning::refill_reserve or the default);
// rt::hand_out (rt_hand_out.h) derives n_block_units and first_blocks from it, on the host here and
// on the device for a table planned there.
uint64_t refill_reserve(const Inputs& in);

// The camera-batch form of the headline kernel (rt_trace_batch.h): whether a launch
// planned as `p` runs it. Only rt_render_device's launches ask. The form is taken for a HASH launch
// with the uniform hand-out (table: a block-table launch) that is not instrumented, planned as the
// one-layer LDS grid walk with shading records (ACCEL_GRID_REC, p.flat), whose camera the host
// proved pinhole_lf, with max_depth <= kBatchMaxDepth, when the form's own LDS (static_lds of the
// kernel + the plan's dynamic bytes, rows map included) keeps two blocks per CU and, where the
// kernels' translation unit was asked (kernel_blocks >= 0), its kernel runs at least the plan's
// blocks per CU. `tune`: rt_debug_tune's "camera_batches" (0 switches the form off; unset: the
// default, kCameraBatchesDefault). Returns BATCH_ON or the first reason against, *lds_total the
// form's static + dynamic LDS bytes.
enum : uint32_t { BATCH_ON = 0, BATCH_OFF_TUNE = 1, BATCH_OFF_STREAM = 2, BATCH_OFF_TABLE = 3, BATCH_OFF_COUNT = 4,
                  BATCH_OFF_FORM = 5, BATCH_OFF_PINHOLE = 6, BATCH_OFF_DEPTH = 7, BATCH_OFF_LDS = 8,
                  BATCH_OFF_OCCUPANCY = 9 };
constexpr double kCameraBatchesDefault = 1;
// Static LDS of rt_trace_grid_batch_kernel: the pixel sums (18 432 B), kBatchLdsBytes (36 864 B: the
// queue, the chain counters, the gate table and the camera-origin terms, rt_internal.h), and the
// walk parameters every walk kernel stages (s_walk_axis, s_walk_slack, s_walk_entry: 104 B, laid out
// in 112): 55 408 B.
constexpr uint32_t kBatchStaticLdsBytes = rt::kLaneSumLdsBytes + rt::kBatchLdsBytes + 112u;
uint32_t camera_batches(const Inputs& in, const Plan& p, double tune, uint32_t max_depth, bool table,
                        uint32_t static_lds, int kernel_blocks, uint32_t* lds_total);

// Both halves for the band of `in` (rt_debug_launch_plan without a context).
int make_plan(const Inputs& in, const Device& dev, Plan& p, const char** err);

// Per band row of a launch, its share of the launch's work from its tile-cost record `cost` (n
// tiles, row-major, tiles_x per row) and the order the tiles ran in (`order`: rank -> tile, null:
// none kept): rt_launch_row_weights.
void row_weights(const uint32_t* cost, const uint32_t* order, uint32_t n, uint32_t tiles_x, uint32_t band_h,
                 uint32_t head_tiles, uint32_t head_chunks, uint32_t chunks, std::vector<double>& w);

}  // namespace launch
}  // namespace rt
