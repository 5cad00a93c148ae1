// rt_context.h — the device context and the sample map as the host runtime files see them
// (rt_api.cpp, rt_adaptive_frame.cpp, rt_sample_map_frame.cpp), and the steps of a frame that more
// than one of them takes. Private and host only: never included by a .hip file, and not by
// rt_multi.cpp, whose interface to a context is rt_host.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/rt_mi355x.h"
#include "rt_adaptive.h"
#include "rt_build.h"
#include "rt_host.h"
#include "rt_internal.h"
#include "rt_launch.h"
#include "rt_sample_map.h"

// One arena of device-built scenes (rt_context::slot; rt_api.cpp device_build_begin).
struct SceneSlot {
    rt::DeviceScene scene;            // its arrays (pointers into mem / grid_mem) and counts
    void* mem = nullptr;              // every per-sphere array of the build, one allocation
    uint32_t cap_n = 0;               // spheres it holds
    void* grid_mem = nullptr;         // cell offsets, fill cursor, references, ids, scan scratch
    size_t grid_cap = 0;              // bytes
    hipEvent_t ev_free = nullptr;     // recorded after every launch that reads this arena
    bool used = false;                // ev_free has been recorded
};

// The launch parameters rt_render_device and rt_render_adaptive_device share: everything that
// does not depend on how the band's samples are split into units.
struct TraceSetup {
    rt::TraceParams P;
    rt::launch::Inputs in;       // what the plan is computed from
    rt::launch::Plan plan;       // the form half (plan_form); split_units fills the rest per launch
    uint64_t tiles_x = 0, n_tiles = 0;
    const uint32_t* tab_blocks = nullptr;   // with P.tab_size: the device word that holds the table's block count
    bool camera_batches = false;            // launch_units runs the camera-batch form (rt_render_device's decision)
};

struct rt_context {
    int device = 0;
    rt::launch::Tuning tune;
    int cu_count = 0;
    rt::DeviceScene scene;                       // the current scene (host blob or an arena)
    bool scene_set = false;                      // a set/refit call has succeeded (RT_ERR_NO_SCENE)
    // device-built scenes: two arenas used alternately, built on the context's own stream
    SceneSlot slot[2];
    int slot_cur = -1;                           // arena of the current scene (-1: host-built / none)
    hipStream_t build_stream = nullptr;
    hipEvent_t ev_summary = nullptr;             // the build's summary has reached pinned memory
    hipEvent_t ev_caller = nullptr;              // device spheres: the caller's stream reached the call
    rt::BuildSummary* summary = nullptr;         // pinned
    void* sph_stage = nullptr;                   // pinned staging of host spheres
    size_t sph_stage_cap = 0;
    bool pending = false;                        // a build begun, not yet ended (rt_multi_set_scene)
    int pending_slot = 0;
    uint32_t pending_count = 0;
    bool refused = false;                        // device_build_end refused non-finite device spheres:
                                                 // the scene call leaves the previous scene in place
    rt::Counters* counters = nullptr;            // device
    float* big_tab = nullptr;                    // device, in the counters' allocation (TraceParams::big_tab)
    // Every device operation of a context (scene upload / build, render) is ordered after the
    // previous one, whatever streams they are issued on: an op on a stream other than the last
    // one first waits for `ev_last`, and every op records it when issued. A device build runs on
    // the build stream beside the previous op (it waits only for the launches that read its
    // arena), so it does not cover that op: the op's event moves to `ev_prev`,
    // which the next op waits for as well (order_on) until an op issued after both clears it.
    hipStream_t last_stream = nullptr;
    hipEvent_t ev_last = nullptr;
    bool ev_valid = false;
    hipStream_t prev_stream = nullptr;
    hipEvent_t ev_prev = nullptr;
    bool prev_valid = false;
    // the build workspace (ws) holds the topology of a full build that completed: a refit may
    // reuse it (a full build that failed after overwriting ws leaves it false)
    bool topo_ok = false;
    bool pending_refit = false;
    // occupancy cache per kernel form, count flag and rng mode, valid for occ_lds bytes
    int occ[rt::ACCEL_COUNT][3][2] = {};   // [form][plain, count_tests, one-layer grid walk][mode]
    size_t occ_lds[rt::ACCEL_COUNT][3][2] = {};
    bool has_grid = false;                       // the scene has a grid
    float grid_pad_radius = 0.0f;                // camera radius the grid's margin covers
    // unpadded LBVH node boxes (host) and the radius the device copy is padded for
    std::vector<rt::BvhNode> nodes_host;
    float scene_radius = 0.0f;
    float pad_radius = 0.0f;
    float padded_for = 0.0f;                     // pad radius the device node copy currently carries
    bool gpu_tree = false;
    bool treelet_stale = true;                   // ACCEL_LBVH_TOP: the treelet predates the node boxes
    rt::TileSchedule sched;                      // unit hand-out order (LPT from the last launch's costs)
    rt::BuildWorkspace ws;                       // device build scratch, kept for refits
    Sphere* d_spheres = nullptr;                 // staging copy of host-provided spheres (device build)
    uint32_t d_spheres_cap = 0;
    // Host-built scenes: every device array lives in one device blob, rewritten in stream order
    // by one copy from a pinned staging buffer (two, alternating, each guarded by the event of
    // its last copy), so rt_set_scene builds the next frame's tree on the host while the
    // previous frame still renders (no device-wide sync, no per-frame hipMalloc/hipFree).
    void* blob = nullptr;
    size_t blob_cap = 0;
    void* stage[2] = {nullptr, nullptr};
    size_t stage_cap[2] = {0, 0};
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    bool stage_used[2] = {false, false};
    int stage_cur = 0;
    // RT_RNG_SAMPLE_HASH: 3 planes of fixed-point sums, zero between launches (the resolve
    // kernel clears what it reads)
    unsigned long long* fixed = nullptr;
    uint64_t fixed_cap = 0;                      // texels
    // the last launch's plan (rt_launch.h; accel 0 = none yet) and what it was computed from, with
    // the occupancies it queried (rt_debug_launch_info, rt_debug_launch_plan)
    rt::launch::Plan last_plan;
    rt::launch::Inputs last_in;
    // the camera-batch form (rt_launch.h camera_batches): its tuning value (rt_debug_tune
    // "camera_batches"; kept beside `tune`, whose layout is part of the plan's inputs), the occupancy
    // of its kernel at batch_occ_lds dynamic bytes, and whether the last launch ran it
    double tune_camera_batches = rt::launch::Tuning::kUnset;
    int batch_occ = 0;
    size_t batch_occ_lds = ~size_t(0);
    bool last_camera_batches = false;
    // every colour the shaders can return lies in [0, 1] (RT_RNG_SAMPLE_HASH's fixed point needs it)
    bool colours_unit = true;
    // host waits inside render and set calls that are documented as queued without one (buffer
    // growth; rt_debug_host_waits: the feedback tests read 0 once the buffers stand)
    uint64_t host_waits = 0;
    // HIP events bracketing the trace kernel of the last kKernelEvents launches (ring; timing
    // inside a caller's timed region without a host sync per launch, rt_debug_kernel_times)
    static constexpr uint32_t kKernelEvents = 64;
    hipEvent_t kev[kKernelEvents][2] = {};
    uint64_t kev_count = 0;                      // launches recorded so far
    // Host copies of the last launches' tile-cost records (and the LPT order they ran in), copied
    // after the kernel on the launch stream: the cross-device balancer reads a launch's per-row
    // work from them two frames later without a wait on queued work (rt_launch_row_weights).
    struct CostSnap {
        uint32_t* host = nullptr;                // pinned: cost[n], then order[n] when has_order
        uint32_t cap = 0;                        // tiles it holds
        hipEvent_t ev = nullptr;                 // after the copies
        bool pending = false;
        uint64_t launch = ~0ull;                 // launch index the record belongs to
        uint32_t n = 0, tiles_x = 0, band_h = 0, head_tiles = 0, head_chunks = 1, chunks = 1;
        bool has_order = false;
    };
    static constexpr uint32_t kSnaps = 4;
    CostSnap snap[kSnaps];
    bool keep_snaps = false;   // set by the first rt_launch_row_weights (or rt_multi at N > 1):
                               // a one-device frame loop pays no copies it never reads
    // rt_denoise_device (rt_features.cpp): three float4 band planes in one
    // allocation, the two the iterations alternate between and the guide plane the first one stores;
    // rt_denoise_variance_device uses the same three (its variance rides in their w slot)
    struct Denoise {
        float* planes = nullptr;
        uint64_t cap = 0;                        // texels per plane
        uint32_t lds_max_step = 4;               // rt_denoise_host.h kLdsMaxStep; rt_debug_denoise_lds_steps
    } denoise;
    // Adaptive frames (rt_render_adaptive_device) keep their own buffers, so they
    // leave `fixed` and `sched` alone.
    struct Adaptive {
        unsigned long long* planes = nullptr;   // half-buffers A then B, 3 planes of the band's texels
                                                // each; zero between calls (the resolve clears them)
        uint64_t cap = 0;                       // texels the allocation holds (x 6 planes)
        uint32_t* tiles = nullptr;              // per tile: sample count, the two tile lists and the
        uint64_t cap_tiles = 0;                 // walk kernels' cost scratch: 4 x cap_tiles words
        rt::AdaptiveState* state = nullptr;     // device
        rt::AdaptiveState* host = nullptr;      // pinned copy, read after `ev` once per pass
        hipEvent_t ev = nullptr;
        // the band of the last completed adaptive frame, whose count table the head of `tiles` still
        // holds (0 x 0: none): rt_sample_map_set_from_adaptive reads it
        uint32_t last_w = 0, last_h = 0;
        // The frame in flight, between rt::adaptive_begin and rt::adaptive_finish / adaptive_abort
        // (rt_host.h): the pass loop as a state machine, so that one host thread can interleave
        // the passes of several contexts (rt_multi_render_adaptive).
        struct Frame {
            bool open = false;
            bool pending = false;               // a pass is issued and its readback not yet consumed
            TraceSetup S;
            rt_options o{};
            rt_adaptive ad{};
            hipStream_t st = nullptr;
            uint32_t max_spp = 0, done = 0, passes = 0, cur = 0;
            uint64_t active = 0;                // tiles of the next pass
            const uint32_t* list = nullptr;     // their list (null: pass 0, every tile, row-major)
        } frame;
    } adaptive;
};

// A sample map: the plan of its last set call on the host (rt_sample_map.h) and,
// on the device, what the launches and the resolve read. Rewritten only by a set call, which first
// waits for `ev_read`, recorded behind every frame that renders the map.
struct rt_sample_map {
    rt_context* ctx = nullptr;
    uint32_t band_w = 0, band_h = 0, n_tiles = 0;
    uint32_t* table = nullptr;           // device: order[n_tiles], then the quantised counts[n_tiles]
    uint32_t* stage = nullptr;           // pinned, 2 x n_tiles words: the set calls' copies
    bool set = false;
    rt::sample_map::Plan plan;
    rt_sample_map_info info{};
    // the schedule the next set call plans by (rt_sample_map_set_schedule), and the one the held plan has
    uint32_t next_schedule = RT_SAMPLE_MAP_LEVELS, next_unit = 0;
    uint32_t schedule = RT_SAMPLE_MAP_LEVELS, unit_samples = 0;
    rt::BlockEntry* blocks = nullptr;    // device: the block table of a one-launch plan (n_blocks entries)
    uint64_t n_blocks = 0, cap_blocks = 0;
    hipEvent_t ev_read = nullptr;
    mutable bool read_pending = false;   // ev_read has been recorded since the last set call
    // A map planned on the device (rt_sample_map_set_device_async): `table` and `blocks` were written
    // there, in stream order, and the host knows the cap alone; what the planner found (block count,
    // unit, totals) stays in `summary` until an info call copies it back. The planner's buffers are
    // allocated by the first such call.
    bool device_planned = false;
    uint32_t count_cap = 0;
    uint64_t limit_blocks = 0;           // rt_debug_sample_map_limit_blocks (0: none)
    rt::TabSize* tab_size = nullptr;     // device: the size record of the map's launches, then ...
    rt::sample_map::DeviceSummary* summary = nullptr;   // ... the planner's summary (one allocation)
    uint32_t* plan_words = nullptr;      // device: keys, values, sorted keys, offsets (4 x n_tiles)
    void* plan_temp = nullptr;           // device: the sort's and the scan's scratch
    size_t plan_temp_bytes = 0;
    // Feedback frames (rt_render_sample_map_feedback_device): the table is planned in halves mode, one
    // half of at most half_capacity entries; `next` holds the counts the last frame's update chose
    // (in plan_words), `moved` the tiles the updates raised | lowered << 32 (behind the summary).
    bool halves = false;
    uint64_t half_capacity = 0;
    uint32_t* next = nullptr;
    unsigned long long* moved = nullptr;
};

// The state of a temporal stage (rt_temporal_create): three float4 planes of the
// band in one allocation, HA, HB and HG (rt_temporal_host.h), written only by the work that
// rt_temporal_accumulate_device, rt_temporal_reproject_device and rt_temporal_reset queue. A
// reprojected call reads neighbours, so it writes a second set of the three planes (allocated by the
// first such call) and makes that one current; the in-place call and the reset work on the current set.
struct rt_temporal {
    rt_context* ctx = nullptr;
    uint32_t band_w = 0, band_h = 0;
    float* planes = nullptr;
    float* planes2 = nullptr;
    int cur = 0;                         // the current set: 0 = planes, 1 = planes2
    float* set(int k) const { return k ? planes2 : planes; }
};

// The state of a motion pass (rt_motion_create): the scratch of its launches (one
// ray and one (winner, t) answer per texel of the band) and the previous frame, its camera and one
// float4 per sphere id whose xyz is the centre (w is not read).
struct rt_motion {
    rt_context* ctx = nullptr;
    uint32_t band_w = 0, band_h = 0;
    float* rays = nullptr;
    uint32_t* hits = nullptr;
    bool has_prev = false;
    RenderCallInfo prev_rci{};
    float* prev_geom = nullptr;          // device, prev_cap float4
    uint64_t prev_cap = 0;
    uint32_t prev_n = 0;
    float* stage = nullptr;              // pinned staging of rt_motion_set_previous, stage_cap float4
    uint64_t stage_cap = 0;
    hipEvent_t stage_ev = nullptr;       // behind the last copy out of `stage`
    bool stage_used = false;
};

namespace rt {

// Stream chaining of a context's device operations (rt_context::ev_last): order_on before an op on
// `st`, mark_issued after it; render_issued ends a render call (rt_api.cpp).
int order_on(rt_context* ctx, hipStream_t st);
int mark_issued(rt_context* ctx, hipStream_t st);
int render_issued(rt_context* ctx, hipStream_t st);

// A render call's argument checks, the launch parameters of its band and its trace launches
// (rt_api.cpp).
int check_render_args(const rt_context* ctx, const RenderCallInfo* rci, uint32_t band_width, uint32_t band_height,
                      const float* accum, const uint8_t* out, const rt_options* opt, const char* who, rt_options& o,
                      bool* empty);
int fill_trace(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows, uint32_t band_width,
               uint32_t band_height, const rt_options& o, float* accum, uint8_t* out, hipStream_t st, TraceSetup& S);
int fill_trace_at(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows, uint32_t band_width,
                  uint32_t band_height, const rt_options& o, float* accum, uint8_t* out, hipStream_t st, float cam_r,
                  int pinhole_lf, TraceSetup& S);
int launch_units(rt_context* ctx, TraceSetup& S, hipStream_t st);
int launch_tile_prefix(rt_context* ctx, TraceSetup& S, uint32_t spp, uint32_t sample_base, uint64_t c, bool ordered,
                       hipStream_t st);

// The adaptive planes, which sample-map frames sum into as well (rt_adaptive_frame.cpp).
int adaptive_reserve(rt_context* ctx, uint64_t texels, uint64_t n_tiles, hipStream_t st);
int abort_on_planes(rt_context* ctx, hipStream_t st, int rc);

// Grows a device buffer that work queued on `st` may still read to `count` units of `unit` bytes
// (sum planes: zeroed on `st`). An old buffer is freed after the stream has drained (every earlier
// op of ctx is ordered before it); the new buffer and its capacity are set after success only
// (a failed growth leaves none).
template <class T>
int grow_on_stream(T*& buf, uint64_t& cap, uint64_t count, size_t unit, bool zero, hipStream_t st) {
    if (buf) {
        RT_HIP(hipStreamSynchronize(st));
        RT_HIP(hipFree(buf));
    }
    buf = nullptr;
    cap = 0;
    void* p = nullptr;
    RT_HIP(hipMalloc(&p, count * unit));
    if (zero) RT_HIP(hipMemsetAsync(p, 0, count * unit, st));
    buf = static_cast<T*>(p);
    cap = count;
    return RT_OK;
}

}  // namespace rt
