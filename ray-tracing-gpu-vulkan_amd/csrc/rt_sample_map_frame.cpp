// rt_sample_map_frame.cpp — sample maps: the map object with its three set paths
// (from a device table, from the last adaptive frame, planned on the device) and the two frame kinds
// that render one (rt_render_sample_map_device, rt_render_sample_map_feedback_device). The host
// planner is rt_sample_map.cpp, the device planner rt_sample_map_plan.hip; the frames sum into the
// adaptive planes (rt_adaptive_frame.cpp) through rt_api.cpp's launches (rt_context.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <new>
#include <string>
#include <utility>

#include "../../include/rt_mi355x_debug.h"
#include "rt_context.h"
#include "rt_launchers.h"
#include "rt_sample_map_feedback.h"

using rt::fail;
using rt::fail_hip;
using rt::order_on, rt::mark_issued, rt::render_issued, rt::check_render_args, rt::fill_trace, rt::launch_units,
    rt::launch_tile_prefix, rt::adaptive_reserve, rt::abort_on_planes;

namespace {

// Frees a map and what it holds (rt_sample_map_destroy; a failed rt_sample_map_create with its `rc`).
int release_map(rt_sample_map* map, int rc) {
    (void)hipFree(map->table);
    (void)hipFree(map->blocks);
    (void)hipFree(map->tab_size);
    (void)hipFree(map->plan_words);
    (void)hipFree(map->plan_temp);
    if (map->stage) (void)hipHostFree(map->stage);
    if (map->ev_read) (void)hipEventDestroy(map->ev_read);
    delete map;
    return rc;
}

// The set calls of a sample map, the one synchronous step: waits for the frames
// that read the map, brings the count table `d_counts` (written by earlier work on `st`) to the
// host, plans it there and uploads the order and the quantised table, under the one-launch schedule
// the block table too (into a buffer of its own, grown before anything of the map changes). A
// refusal leaves the map as it was.
int sample_map_set(rt_sample_map* map, const uint32_t* d_counts, uint32_t quantum, hipStream_t st,
                   rt_sample_map_info* info) {
    const size_t n = map->n_tiles;
    if (map->read_pending) RT_HIP(hipEventSynchronize(map->ev_read));
    map->read_pending = false;
    RT_HIP(hipMemcpyAsync(map->stage, d_counts, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    rt::sample_map::Plan plan;
    rt::sample_map::BlockPlan bp;
    rt_sample_map_info fresh{};
    std::string err;
    const bool one = map->next_schedule == RT_SAMPLE_MAP_ONE_LAUNCH;
    if (one) {
        if (int rc = rt::sample_map::make_block_plan(map->stage, map->n_tiles, quantum, map->next_unit, bp, &err))
            return fail(rc, err);
        plan = std::move(bp.plan);
    } else if (int rc = rt::sample_map::make_plan(map->stage, map->n_tiles, quantum, plan, &err)) {
        return fail(rc, err);
    }
    if (int rc = rt::sample_map::totals(plan, map->band_w, map->band_h, &fresh, &err)) return fail(rc, err);
    if (one) fresh.tile_launches = bp.live_tiles;   // every non-zero tile is launched once
    rt::BlockEntry* grown = nullptr;
    if (one && bp.blocks.size() > map->cap_blocks) {
        if (hipError_t e = hipMalloc(reinterpret_cast<void**>(&grown), bp.blocks.size() * sizeof(rt::BlockEntry)); e != hipSuccess)
            return fail_hip(e, "rt_sample_map block table");
    }
    std::copy(plan.order.begin(), plan.order.end(), map->stage);
    std::copy(plan.quantised.begin(), plan.quantised.end(), map->stage + n);
    map->set = false;   // until the upload has landed
    if (grown) {   // (no frame reads the old table: ev_read was waited for above)
        (void)hipFree(map->blocks);
        map->blocks = grown;
        map->cap_blocks = bp.blocks.size();
    }
    map->n_blocks = 0;
    RT_HIP(hipMemcpyAsync(map->table, map->stage, 2u * n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (one && !bp.blocks.empty())
        RT_HIP(hipMemcpyAsync(map->blocks, bp.blocks.data(), bp.blocks.size() * sizeof(rt::BlockEntry),
                              hipMemcpyHostToDevice, st));
    RT_HIP(hipStreamSynchronize(st));   // frames on any stream of the context may follow
    map->plan = std::move(plan);
    map->info = fresh;
    map->schedule = map->next_schedule;
    map->unit_samples = one ? bp.unit_samples : 0u;
    map->n_blocks = one ? bp.blocks.size() : 0u;
    map->set = true;
    map->device_planned = false;
    map->halves = false;
    if (info) *info = fresh;
    return RT_OK;
}

// The planner's summary of a device-planned map, after a host wait for the planner (and whatever was
// queued on the map since): the one synchronisation such a map has, in the info calls only.
int device_summary(const rt_sample_map* map, rt::sample_map::DeviceSummary* s) {
    if (map->read_pending) RT_HIP(hipEventSynchronize(map->ev_read));
    RT_HIP(hipMemcpy(s, map->summary, sizeof(*s), hipMemcpyDeviceToHost));
    return RT_OK;
}

// The set call without a host wait: the table never leaves the device. Behind the
// frames queued on the map (events) the planner (rt_sample_map_plan.hip) clamps, sorts, chooses the
// unit and writes the order, the clamped counts and the block table; the host keeps the cap. Buffers
// are allocated here and the block table grows here only (a growth waits for the frames that read
// the old one: the one host wait this call can contain, at most once per cap and unit).
// `halves`: the plan of a feedback frame (rt_sample_map_device.h DevicePlanParams::halves; count_cap
// even). d_tile_counts null: the map's own feedback counts (rt_sample_map::next).
int queue_device_plan(rt_sample_map* map, const uint32_t* d_tile_counts, uint32_t unit_samples, uint32_t count_cap,
                      bool halves, hipStream_t st, const char* who) {
    if (count_cap > rt::sample_map::kMaxCount)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": count_cap = " + std::to_string(count_cap) + " is above 2^19");
    if (unit_samples > rt::sample_map::kMaxUnit)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": unit_samples = " + std::to_string(unit_samples) + " is above 2^19");
    if (map->n_tiles > rt::sample_map::kDeviceMaxBlocks)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": the band has " + std::to_string(map->n_tiles) +
                                                 " tiles, more than the 2^22 entries of a device-planned block table");
    rt_context* ctx = map->ctx;
    const size_t n = map->n_tiles;
    if (!map->tab_size) {   // the planner's buffers, once per map
        size_t temp = 0;
        if (hipError_t e = rt::device_plan_temp_bytes(map->n_tiles, &temp); e != hipSuccess) return fail_hip(e, who);
        void *rec = nullptr, *words = nullptr, *tmp = nullptr;
        static_assert(sizeof(rt::TabSize) == 16, "the summary follows the size record, 16-byte aligned");
        static_assert(sizeof(rt::sample_map::DeviceSummary) % 8 == 0, "the feedback frames' counter follows the summary");
        const size_t rec_bytes = sizeof(rt::TabSize) + sizeof(rt::sample_map::DeviceSummary) + sizeof(unsigned long long);
        hipError_t e = hipMalloc(&rec, rec_bytes);
        if (e == hipSuccess) e = hipMemset(rec, 0, rec_bytes);
        if (e == hipSuccess) e = hipMalloc(&words, 5u * n * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&tmp, temp ? temp : 16u);
        if (e != hipSuccess) {
            (void)hipFree(rec);
            (void)hipFree(words);
            (void)hipFree(tmp);
            return fail_hip(e, who);
        }
        map->tab_size = static_cast<rt::TabSize*>(rec);
        map->summary = reinterpret_cast<rt::sample_map::DeviceSummary*>(map->tab_size + 1);
        map->moved = reinterpret_cast<unsigned long long*>(map->summary + 1);
        map->plan_words = static_cast<uint32_t*>(words);
        map->next = map->plan_words + 4u * n;
        map->plan_temp = tmp;
        map->plan_temp_bytes = temp;
    }
    const uint32_t unit0 = rt::sample_map::device_unit0(unit_samples, count_cap);
    // (halves: the capacity of one half; the buffer holds the two halves and the B half's second copy)
    const uint64_t natural = std::max<uint64_t>(1u, rt::sample_map::device_capacity(n, halves ? count_cap / 2u : count_cap, unit0));
    const uint64_t entries = halves ? 3u * natural : natural;
    if (entries > map->cap_blocks) {
        rt::BlockEntry* grown = nullptr;
        if (hipError_t e = hipMalloc(reinterpret_cast<void**>(&grown), entries * sizeof(rt::BlockEntry)); e != hipSuccess)
            return fail_hip(e, who);
        if (map->blocks) {   // frames queued on the map read the old table
            if (map->read_pending) {
                ctx->host_waits++;
                RT_HIP(hipEventSynchronize(map->ev_read));
            }
            (void)hipFree(map->blocks);
        }
        map->blocks = grown;
        map->cap_blocks = entries;
    }
    // (a test's limit below the non-zero tiles would leave no unit that fits: never below n_tiles)
    const uint64_t capacity = map->limit_blocks ? std::min(natural, std::max<uint64_t>(map->limit_blocks, n)) : natural;
    if (int rc = order_on(ctx, st)) return rc;
    if (map->read_pending) RT_HIP(hipStreamWaitEvent(st, map->ev_read, 0));
    rt::sample_map::DevicePlanParams K{};
    K.counts = d_tile_counts ? d_tile_counts : map->next;
    K.halves = halves ? 1u : 0u;
    K.n_tiles = map->n_tiles;
    K.band_w = map->band_w;
    K.band_h = map->band_h;
    K.tiles_x = (map->band_w + 7u) / 8u;
    K.count_cap = count_cap;
    K.unit0 = unit0;
    K.capacity = capacity;
    K.order = map->table;
    K.clamped = map->table + n;
    K.blocks = map->blocks;
    K.summary = map->summary;
    K.keys = map->plan_words;
    K.vals = map->plan_words + n;
    K.keys_sorted = map->plan_words + 2u * n;
    K.offsets = map->plan_words + 3u * n;
    K.temp = map->plan_temp;
    K.temp_bytes = map->plan_temp_bytes;
    map->set = false;   // until the planner is queued whole
    if (hipError_t e = rt::launch_device_plan(K, st); e != hipSuccess)
        return fail(RT_ERR_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    RT_HIP(hipEventRecord(map->ev_read, st));   // whoever rewrites the map next waits for the planner too
    map->read_pending = true;
    if (int rc = mark_issued(ctx, st)) return rc;
    map->plan = rt::sample_map::Plan{};
    map->info = rt_sample_map_info{};
    map->info.tiles = map->n_tiles;
    map->schedule = RT_SAMPLE_MAP_ONE_LAUNCH;
    map->unit_samples = 0;
    map->n_blocks = 0;
    map->count_cap = count_cap;
    map->device_planned = true;
    map->halves = halves;
    map->half_capacity = halves ? capacity : 0u;
    map->set = true;
    return RT_OK;
}

// The checks the two frame calls share once `map` is known not to be null, in the order they fire:
// the map is the context's, of the band's size and set; the frame sums in fixed point from zero.
int check_map_frame(const rt_context* ctx, const rt_sample_map* map, uint32_t band_width, uint32_t band_height,
                    const rt_options& o, const std::string& who) {
    if (map->ctx != ctx) return fail(RT_ERR_INVALID_ARGUMENT, who + ": the map belongs to another context");
    if (band_width != map->band_w || band_height != map->band_h)
        return fail(RT_ERR_INVALID_ARGUMENT, who + ": band size " + std::to_string(band_width) + " x " +
                                                 std::to_string(band_height) + " is not the map's " +
                                                 std::to_string(map->band_w) + " x " + std::to_string(map->band_h));
    if (!map->set) return fail(RT_ERR_INVALID_ARGUMENT, who + ": the map was never set");
    if (o.rng_mode != RT_RNG_SAMPLE_HASH) return fail(RT_ERR_INVALID_ARGUMENT, who + " needs rng_mode RT_RNG_SAMPLE_HASH");
    if (o.accumulate) return fail(RT_ERR_INVALID_ARGUMENT, who + ": accumulate must be 0");
    return RT_OK;
}

// ... and their tail: the cap covers what the map holds (of a device-planned map the host knows the
// cap alone), and the sample indices stay within 32 bits.
int check_map_cap(const rt_sample_map* map, uint32_t cap, const rt_options& o, const std::string& who) {
    const uint32_t held = map->device_planned ? map->count_cap : map->info.max_count;
    if (cap < held)
        return fail(RT_ERR_INVALID_ARGUMENT, who + ": samplesPerRenderCall (the cap) " + std::to_string(cap) +
                                                 " is below the map's " + (map->device_planned ? "count_cap " : "max_count ") +
                                                 std::to_string(held));
    if (uint64_t(o.sample_base) + cap > 0xffffffffull)
        return fail(RT_ERR_INVALID_ARGUMENT, "sample_base + samplesPerRenderCall overflows 32 bits");
    return RT_OK;
}

// Puts S into its "launch from a block table" state: one unit per lane of a table block, no tile
// order, chunks or head split. The table holds `n_blocks` entries, or, with `size`, as many as the
// device word `size_blocks` says: the launch then takes its size from the record `size`, filled on
// the stream from that word (launch_units), and runs on the full persistent grid, whatever the
// table holds (an empty one retires every wave at its first refill).
void table_launch(TraceSetup& S, const rt::BlockEntry* tab, uint64_t n_blocks, const rt::TabSize* size,
                  const uint32_t* size_blocks) {
    rt::TraceParams& P = S.P;
    P.block_tab = tab;
    P.tab_size = size;
    P.tile_order = nullptr;
    P.chunks = P.head_chunks = 1u;
    P.n_units = uint32_t(n_blocks * 64u);   // < 2^31 (rt_sample_map.h kMaxBlocks)
    S.tab_blocks = size_blocks;
    S.plan.lpt = 1u;
    S.plan.chunks = S.plan.head_chunks = 1u;
    S.plan.head_tiles = 0u;
    S.plan.n_units = P.n_units;
    rt::launch::hand_out_units(S.in, S.plan, true);
    if (size) S.plan.grid = uint32_t(std::max<uint64_t>(1u, uint64_t(S.in.cu_count) * S.plan.blocks_per_cu));
}

}  // namespace

extern "C" {

int rt_sample_map_create(rt_context* ctx, uint32_t band_width, uint32_t band_height, rt_sample_map** out) {
    if (!ctx || !out) return fail(RT_ERR_INVALID_ARGUMENT, "ctx or out is NULL");
    *out = nullptr;
    if (band_width == 0 || band_height == 0 || band_width > 65535u || band_height > 65535u)
        return fail(RT_ERR_INVALID_ARGUMENT, "band width and height must be within 1 .. 65535");
    const uint64_t n_tiles = uint64_t((band_width + 7u) / 8u) * ((band_height + 7u) / 8u);
    if (n_tiles >= (1ull << 26)) return fail(RT_ERR_INVALID_ARGUMENT, "band too large");
    rt::DeviceGuard g(ctx->device);
    rt_sample_map* m = new (std::nothrow) rt_sample_map;
    if (!m) return fail(RT_ERR_OUT_OF_MEMORY, "rt_sample_map_create: out of host memory");
    m->ctx = ctx;
    m->band_w = band_width;
    m->band_h = band_height;
    m->n_tiles = uint32_t(n_tiles);
    m->info.tiles = m->n_tiles;
    const size_t bytes = size_t(n_tiles) * 2u * sizeof(uint32_t);
    if (hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->table), bytes); e != hipSuccess)
        return release_map(m, fail_hip(e, "rt_sample_map_create"));
    if (hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&m->stage), bytes, hipHostMallocDefault); e != hipSuccess)
        return release_map(m, fail(RT_ERR_OUT_OF_MEMORY, std::string("rt_sample_map_create: ") + hipGetErrorString(e)));
    if (hipError_t e = hipEventCreateWithFlags(&m->ev_read, hipEventDisableTiming); e != hipSuccess)
        return release_map(m, fail(RT_ERR_DEVICE, std::string("rt_sample_map_create: ") + hipGetErrorString(e)));
    *out = m;
    return RT_OK;
}

int rt_sample_map_destroy(rt_sample_map* map) {
    if (!map) return RT_OK;
    rt::DeviceGuard g(map->ctx->device);
    if (map->read_pending) (void)hipEventSynchronize(map->ev_read);   // the frames that read it
    return release_map(map, RT_OK);
}

int rt_sample_map_set_device(rt_sample_map* map, const uint32_t* d_tile_counts, uint32_t quantum, void* stream,
                             rt_sample_map_info* info) {
    if (!map || !d_tile_counts) return fail(RT_ERR_INVALID_ARGUMENT, "map or d_tile_counts is NULL");
    rt::DeviceGuard g(map->ctx->device);
    return sample_map_set(map, d_tile_counts, quantum, static_cast<hipStream_t>(stream), info);
}

int rt_sample_map_set_from_adaptive(rt_sample_map* map, uint32_t quantum, void* stream, rt_sample_map_info* info) {
    if (!map) return fail(RT_ERR_INVALID_ARGUMENT, "map is NULL");
    rt_context* ctx = map->ctx;
    const rt_context::Adaptive& a = ctx->adaptive;
    if (a.frame.open)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_sample_map_set_from_adaptive: an adaptive frame is open on this context");
    if (a.last_w == 0 || !a.tiles)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_sample_map_set_from_adaptive: the context has no completed adaptive frame");
    if (a.last_w != map->band_w || a.last_h != map->band_h)
        return fail(RT_ERR_INVALID_ARGUMENT,
                    "rt_sample_map_set_from_adaptive: the last adaptive frame's band size " + std::to_string(a.last_w) +
                        " x " + std::to_string(a.last_h) + " is not the map's " + std::to_string(map->band_w) + " x " +
                        std::to_string(map->band_h));
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = order_on(ctx, st)) return rc;   // behind the adaptive frame, whatever stream it ran on
    return sample_map_set(map, a.tiles, quantum, st, info);
}

int rt_sample_map_set_device_async(rt_sample_map* map, const uint32_t* d_tile_counts, uint32_t unit_samples,
                                   uint32_t count_cap, void* stream) {
    if (!map || !d_tile_counts) return fail(RT_ERR_INVALID_ARGUMENT, "map or d_tile_counts is NULL");
    rt::DeviceGuard g(map->ctx->device);
    return queue_device_plan(map, d_tile_counts, unit_samples, count_cap, false, static_cast<hipStream_t>(stream),
                             "rt_sample_map_set_device_async");
}

int rt_sample_map_device_unit(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t count_cap, uint32_t unit_samples,
                              uint64_t capacity, uint32_t* unit_used) {
    std::string err;
    if (int rc = rt::sample_map::device_unit(tile_counts, n_tiles, count_cap, unit_samples, capacity, unit_used, nullptr, &err))
        return fail(rc, err);
    return RT_OK;
}

int rt_sample_map_feedback_count(uint64_t E, uint64_t S, uint32_t n, uint32_t m, uint32_t thr_q16, uint32_t min_spp,
                                 uint32_t max_spp, uint32_t* next) {
    if (!next) return fail(RT_ERR_INVALID_ARGUMENT, "next is NULL");
    if (E >= rt::kAdaptiveMaxSum || S >= rt::kAdaptiveMaxSum) return fail(RT_ERR_INVALID_ARGUMENT, "E and S must be below 2^56");
    if (n > rt::kAdaptiveMaxSpp) return fail(RT_ERR_INVALID_ARGUMENT, "n must be at most 2^19");
    if (m == 0 || m > 64u) return fail(RT_ERR_INVALID_ARGUMENT, "m must be within 1 .. 64");
    if (min_spp < 2u || (min_spp & 1u) || (max_spp & 1u) || min_spp > max_spp || max_spp > rt::kAdaptiveMaxSpp)
        return fail(RT_ERR_INVALID_ARGUMENT, "min_spp and max_spp must be even with 2 <= min_spp <= max_spp <= 2^19");
    *next = rt::sample_map_feedback_count(E, S, n, m, thr_q16, min_spp, max_spp);
    return RT_OK;
}

int rt_debug_hand_out(uint32_t n_units, uint64_t reserve, uint64_t grid_waves, uint32_t* n_block_units,
                      uint32_t* first_blocks) {
    if (!n_block_units || !first_blocks) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    const rt::HandOut h = rt::hand_out(n_units, reserve, grid_waves);
    *n_block_units = h.n_block_units;
    *first_blocks = h.first_blocks;
    return RT_OK;
}

int rt_debug_sample_map_limit_blocks(rt_sample_map* map, uint64_t limit) {
    if (!map) return fail(RT_ERR_INVALID_ARGUMENT, "map is NULL");
    map->limit_blocks = limit;
    return RT_OK;
}

int rt_sample_map_get_info(const rt_sample_map* map, rt_sample_map_info* out) {
    if (!map || !out) return fail(RT_ERR_INVALID_ARGUMENT, "map or out is NULL");
    *out = map->info;
    if (map->set && map->device_planned) {   // (levels and min_count stay 0: the planner does not count them)
        rt::DeviceGuard g(map->ctx->device);
        rt::sample_map::DeviceSummary s;
        if (int rc = device_summary(map, &s)) return rc;
        out->max_count = s.max_count;
        out->samples = s.samples;
        out->tile_launches = s.live_tiles;
    }
    return RT_OK;
}

int rt_sample_map_set_schedule(rt_sample_map* map, uint32_t schedule, uint32_t unit_samples) {
    if (!map) return fail(RT_ERR_INVALID_ARGUMENT, "map is NULL");
    if (schedule != RT_SAMPLE_MAP_LEVELS && schedule != RT_SAMPLE_MAP_ONE_LAUNCH)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_sample_map_set_schedule: unknown schedule " + std::to_string(schedule));
    if (schedule == RT_SAMPLE_MAP_LEVELS && unit_samples != 0)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_sample_map_set_schedule: unit_samples must be 0 with RT_SAMPLE_MAP_LEVELS");
    if (unit_samples > rt::sample_map::kMaxUnit)
        return fail(RT_ERR_INVALID_ARGUMENT,
                    "rt_sample_map_set_schedule: unit_samples = " + std::to_string(unit_samples) + " is above 2^19");
    map->next_schedule = schedule;
    map->next_unit = unit_samples;
    return RT_OK;
}

int rt_sample_map_get_schedule(const rt_sample_map* map, uint32_t* schedule, uint32_t* unit_samples_used,
                               uint64_t* n_blocks) {
    if (!map) return fail(RT_ERR_INVALID_ARGUMENT, "map is NULL");
    if (schedule) *schedule = map->schedule;
    if (unit_samples_used) *unit_samples_used = map->unit_samples;
    if (n_blocks) *n_blocks = map->n_blocks;
    if (map->set && map->device_planned && (unit_samples_used || n_blocks)) {
        rt::DeviceGuard g(map->ctx->device);
        rt::sample_map::DeviceSummary s;
        if (int rc = device_summary(map, &s)) return rc;
        if (unit_samples_used) *unit_samples_used = s.unit_used;
        if (n_blocks) *n_blocks = s.n_blocks;
    }
    return RT_OK;
}

int rt_sample_map_block_plan(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, uint32_t unit_samples,
                             uint32_t* blocks_out, uint64_t capacity, uint64_t* n_blocks, uint32_t* unit_samples_used) {
    std::string err;
    if (int rc = rt::sample_map::block_plan_arrays(tile_counts, n_tiles, quantum, unit_samples, blocks_out, capacity,
                                                   n_blocks, unit_samples_used, &err))
        return fail(rc, err);
    return RT_OK;
}

int rt_debug_sample_map_blocks(const rt_sample_map* map, uint32_t* out, uint64_t capacity, uint64_t* n) {
    if (!map || !n) return fail(RT_ERR_INVALID_ARGUMENT, "map or n is NULL");
    if (!map->set) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_sample_map_blocks: the map was never set");
    rt::DeviceGuard g(map->ctx->device);
    uint64_t n_blocks = map->n_blocks;
    if (map->device_planned) {   // the count is the planner's
        rt::sample_map::DeviceSummary s;
        if (int rc = device_summary(map, &s)) return rc;
        n_blocks = std::min<uint64_t>(s.n_blocks, map->cap_blocks);
    }
    if (out && capacity < n_blocks)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_sample_map_blocks: capacity is below the table's " +
                                                 std::to_string(n_blocks) + " blocks");
    if (out && n_blocks) {
        if (map->read_pending) RT_HIP(hipEventSynchronize(map->ev_read));
        RT_HIP(hipMemcpy(out, map->blocks, n_blocks * sizeof(rt::BlockEntry), hipMemcpyDeviceToHost));
    }
    *n = n_blocks;
    return RT_OK;
}

int rt_sample_map_plan(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum, uint32_t* order,
                       uint32_t* levels, uint32_t* level_tiles, uint32_t* n_levels, uint32_t* quantised) {
    std::string err;
    if (int rc = rt::sample_map::plan_arrays(tile_counts, n_tiles, quantum, order, levels, level_tiles, n_levels,
                                             quantised, &err))
        return fail(rc, err);
    return RT_OK;
}

int rt_debug_sample_map_info(const uint32_t* tile_counts, uint32_t band_width, uint32_t band_height, uint32_t quantum,
                             rt_sample_map_info* out) {
    if (band_width == 0 || band_height == 0 || band_width > 65535u || band_height > 65535u)
        return fail(RT_ERR_INVALID_ARGUMENT, "band width and height must be within 1 .. 65535");
    const uint32_t n_tiles = ((band_width + 7u) / 8u) * ((band_height + 7u) / 8u);
    rt::sample_map::Plan plan;
    std::string err;
    if (int rc = rt::sample_map::make_plan(tile_counts, n_tiles, quantum, plan, &err)) return fail(rc, err);
    if (int rc = rt::sample_map::totals(plan, band_width, band_height, out, &err)) return fail(rc, err);
    return RT_OK;
}

int rt_debug_sample_map(const rt_sample_map* map, uint32_t* order, uint32_t* levels, uint32_t* level_tiles,
                        uint32_t* quantised) {
    if (!map) return fail(RT_ERR_INVALID_ARGUMENT, "map is NULL");
    if (!map->set) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_sample_map: the map was never set");
    rt::DeviceGuard g(map->ctx->device);
    if (map->read_pending) RT_HIP(hipEventSynchronize(map->ev_read));
    const size_t n = map->n_tiles;
    if (order) RT_HIP(hipMemcpy(order, map->table, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (quantised) RT_HIP(hipMemcpy(quantised, map->table + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    // (a one-launch plan may hold more levels than the arrays: the lowest RT_SAMPLE_MAP_MAX_LEVELS)
    const size_t j = std::min<size_t>(map->plan.levels.size(), RT_SAMPLE_MAP_MAX_LEVELS);
    if (levels) std::copy_n(map->plan.levels.begin(), j, levels);
    if (level_tiles) std::copy_n(map->plan.level_tiles.begin(), j, level_tiles);
    return RT_OK;
}

// The whole frame is queued: one trace launch per level on the nested prefixes of the map's order
// (a one-launch plan: one launch of its block table), then the resolve with the map as per-tile
// divisors. No host wait, no event synchronisation and no
// blocking copy below (the buffers' first allocation and growth in adaptive_reserve aside).
int rt_render_sample_map_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows, uint32_t band_width,
                                uint32_t band_height, float* accum, uint8_t* out, uint32_t* sample_count,
                                const rt_options* opt, const rt_sample_map* map, void* stream) {
    static const char* const who = "rt_render_sample_map_device";
    rt_options o{};
    bool empty = false;
    if (int rc = check_render_args(ctx, rci, band_width, band_height, accum, out, opt, who, o, &empty)) return rc;
    if (!map) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": map is NULL");
    if (int rc = check_map_frame(ctx, map, band_width, band_height, o, who)) return rc;
    if (int rc = check_map_cap(map, rci->samplesPerRenderCall, o, who)) return rc;
    rt_context::Adaptive& a = ctx->adaptive;
    if (a.frame.open)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": an adaptive frame is open on this context");
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = order_on(ctx, st)) return rc;
    TraceSetup S;
    if (int rc = fill_trace(ctx, rci, rows, band_width, band_height, o, accum, out, st, S)) return rc;
    const uint64_t texels = uint64_t(band_width) * band_height;
    if (int rc = adaptive_reserve(ctx, texels, S.n_tiles, st)) return rc;
    rt::TraceParams& P = S.P;
    // the adaptive planes, half A alone (B stays zero; the resolve leaves both zero), and for the walk
    // kernels' unconditional tile-cost record a scratch table behind everything an adaptive frame
    // uses of `tiles`: the last adaptive frame's count table stays in place
    P.fixed = a.planes;
    P.tile_cost = S.plan.accel != rt::ACCEL_BRUTE ? a.tiles + 3u * a.cap_tiles : nullptr;
    P.tile_order = map->table;
    P.accumulate = 0u;
    P.head_tiles = 0u;
    // (after a failure between the first launch and the resolve the planes hold partial sums:
    // abort_on_planes)
    if (map->device_planned) {   // the table's size is device data
        table_launch(S, map->blocks, 0u, map->tab_size, &map->summary->n_blocks);
        if (int rc = launch_units(ctx, S, st)) return abort_on_planes(ctx, st, rc);
    } else if (map->schedule == RT_SAMPLE_MAP_ONE_LAUNCH) {
        if (map->n_blocks) {   // (an all-zero map: the resolve alone)
            table_launch(S, map->blocks, map->n_blocks, nullptr, nullptr);
            if (int rc = launch_units(ctx, S, st)) return abort_on_planes(ctx, st, rc);
        }
    }
    uint32_t prev = 0;
    for (size_t j = 0; map->schedule == RT_SAMPLE_MAP_LEVELS && j < map->plan.levels.size(); j++) {   // samples [L_{j-1}, L_j) on the first c_j tiles
        const uint32_t level = map->plan.levels[j];
        if (int rc = launch_tile_prefix(ctx, S, level - prev, o.sample_base + prev, map->plan.level_tiles[j], true, st))
            return abort_on_planes(ctx, st, rc);
        prev = level;
    }
    if (hipError_t e = rt::launch_adaptive_resolve(a.planes, a.planes + 3u * texels, texels, band_width, P.tiles_x,
                                                   map->table + map->n_tiles, accum, out, sample_count, nullptr, nullptr,
                                                   nullptr, st);
        e != hipSuccess)
        return abort_on_planes(ctx, st, fail(RT_ERR_DEVICE, std::string("launch_adaptive_resolve: ") + hipGetErrorString(e)));
    RT_HIP(hipEventRecord(map->ev_read, st));   // the next set call waits for this frame
    map->read_pending = true;
    return render_issued(ctx, st);
}

}  // extern "C"

namespace {

// A feedback frame: the map's A half into planes A and its B half into planes B
// (two table launches sized on the device), the update (the next counts from the two halves'
// difference), the resolve (A + B by the map's counts; zeroes both) and the planner in halves mode
// on the next counts. Everything is queued; the context orders it behind whatever it queued before,
// so the one table of the map is rebuilt only after the frames that read it.
// `halves` (rt_render_sample_map_feedback_halves_device, checked by the caller; null: the plain call):
// the resolve also writes the two halves and the half counts.
int feedback_frame(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows, uint32_t band_width,
                   uint32_t band_height, float* accum, uint8_t* out, uint32_t* sample_count, const rt_options* opt,
                   rt_sample_map* map, const rt_sample_map_feedback* fb, uint64_t* d_tile_error,
                   const rt_half_outputs* halves, void* stream, const char* who) {
    rt_options o{};
    bool empty = false;
    if (int rc = check_render_args(ctx, rci, band_width, band_height, accum, out, opt, who, o, &empty)) return rc;
    if (!map || !fb) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": map or feedback is NULL");
    if (int rc = check_map_frame(ctx, map, band_width, band_height, o, who)) return rc;
    const uint32_t cap = rci->samplesPerRenderCall;
    if (cap & 1u) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": samplesPerRenderCall (the cap) must be even");
    if (!(std::isfinite(fb->threshold) && fb->threshold >= 0.0f && fb->threshold <= 16.0f))
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": feedback threshold must be finite and within [0, 16]");
    if (fb->min_spp < 2u || (fb->min_spp & 1u) || (fb->max_spp & 1u) || fb->min_spp > fb->max_spp ||
        fb->max_spp > rt::kAdaptiveMaxSpp)
        return fail(RT_ERR_INVALID_ARGUMENT,
                    std::string(who) + ": feedback min_spp and max_spp must be even with 2 <= min_spp <= max_spp <= 2^19");
    if (cap < fb->max_spp)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": samplesPerRenderCall (the cap) " + std::to_string(cap) +
                                                 " is below the feedback max_spp " + std::to_string(fb->max_spp));
    if (fb->unit_samples > rt::sample_map::kMaxUnit)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": feedback unit_samples is above 2^19");
    if (fb->reserved != 0) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": feedback reserved must be 0");
    if (int rc = check_map_cap(map, cap, o, who)) return rc;
    if (map->n_tiles > rt::sample_map::kDeviceMaxBlocks)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": the band has more than 2^22 tiles");
    rt_context::Adaptive& a = ctx->adaptive;
    if (a.frame.open)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": an adaptive frame is open on this context");
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = order_on(ctx, st)) return rc;
    const size_t n = map->n_tiles;
    if (!(map->device_planned && map->halves && map->count_cap == cap)) {
        // the first feedback frame on this map (or at this cap): its current counts, in halves
        if (int rc = queue_device_plan(map, map->table + n, fb->unit_samples, cap, true, st, who)) return rc;
    }
    TraceSetup S;
    if (int rc = fill_trace(ctx, rci, rows, band_width, band_height, o, accum, out, st, S)) return rc;
    const uint64_t texels = uint64_t(band_width) * band_height;
    if (int rc = adaptive_reserve(ctx, texels, S.n_tiles, st)) return rc;
    rt::TraceParams& P = S.P;
    P.tile_cost = S.plan.accel != rt::ACCEL_BRUTE ? a.tiles + 3u * a.cap_tiles : nullptr;
    P.accumulate = 0u;
    P.head_tiles = 0u;
    table_launch(S, map->blocks, 0u, map->tab_size, &map->summary->half_blocks);
    unsigned long long* half[2] = {a.planes, a.planes + 3u * texels};
    for (int h = 0; h < 2; h++) {   // the B half's entries once more from entry 2 x half_capacity
        P.fixed = half[h];
        P.block_tab = map->blocks + (h ? 2u * map->half_capacity : 0u);
        if (int rc = launch_units(ctx, S, st)) return abort_on_planes(ctx, st, rc);
    }
    rt::FeedbackParams F{};
    F.a = half[0];
    F.b = half[1];
    F.texels = texels;
    F.band_w = band_width;
    F.band_h = band_height;
    F.tiles_x = P.tiles_x;
    F.n_tiles = map->n_tiles;
    F.tile_n = map->table + n;
    F.thr_q16 = rt::adaptive_thr_q16(fb->threshold);
    F.min_spp = fb->min_spp;
    F.max_spp = fb->max_spp;
    F.next = map->next;
    F.tile_error = reinterpret_cast<unsigned long long*>(d_tile_error);
    F.moved = map->moved;
    if (hipError_t e = rt::launch_feedback_update(F, st); e != hipSuccess)
        return abort_on_planes(ctx, st, fail(RT_ERR_DEVICE, std::string("launch_feedback_update: ") + hipGetErrorString(e)));
    if (hipError_t e = rt::launch_adaptive_resolve(half[0], half[1], texels, band_width, P.tiles_x, map->table + n, accum, out,
                                                   sample_count, halves ? halves->accum_a : nullptr,
                                                   halves ? halves->accum_b : nullptr,
                                                   halves ? halves->half_count : nullptr, st);
        e != hipSuccess)
        return abort_on_planes(ctx, st, fail(RT_ERR_DEVICE, std::string("launch_adaptive_resolve: ") + hipGetErrorString(e)));
    if (int rc = render_issued(ctx, st)) return rc;
    // the next frame's table, from the counts the update chose (<= max_spp <= cap)
    return queue_device_plan(map, nullptr, fb->unit_samples, cap, true, st, who);
}

}  // namespace

extern "C" {

int rt_render_sample_map_feedback_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows,
                                         uint32_t band_width, uint32_t band_height, float* accum, uint8_t* out,
                                         uint32_t* sample_count, const rt_options* opt, rt_sample_map* map,
                                         const rt_sample_map_feedback* fb, uint64_t* d_tile_error, void* stream) {
    return feedback_frame(ctx, rci, rows, band_width, band_height, accum, out, sample_count, opt, map, fb, d_tile_error,
                          nullptr, stream, "rt_render_sample_map_feedback_device");
}

int rt_render_sample_map_feedback_halves_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows,
                                                uint32_t band_width, uint32_t band_height, float* accum, uint8_t* out,
                                                uint32_t* sample_count, const rt_options* opt, rt_sample_map* map,
                                                const rt_sample_map_feedback* fb, uint64_t* d_tile_error,
                                                const rt_half_outputs* halves, void* stream) {
    if (int rc = rt::half_outputs_check(halves, accum)) return rc;
    return feedback_frame(ctx, rci, rows, band_width, band_height, accum, out, sample_count, opt, map, fb, d_tile_error,
                          halves, stream, "rt_render_sample_map_feedback_halves_device");
}

int rt_debug_sample_map_feedback(rt_sample_map* map, uint32_t* next, uint64_t* raised, uint64_t* lowered) {
    if (!map) return fail(RT_ERR_INVALID_ARGUMENT, "map is NULL");
    if (!map->next) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_sample_map_feedback: the map was never planned on the device");
    rt::DeviceGuard g(map->ctx->device);
    if (map->read_pending) RT_HIP(hipEventSynchronize(map->ev_read));
    unsigned long long moved = 0;
    RT_HIP(hipMemcpy(&moved, map->moved, sizeof(moved), hipMemcpyDeviceToHost));
    if (next) RT_HIP(hipMemcpy(next, map->next, size_t(map->n_tiles) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (raised) *raised = moved & 0xffffffffull;
    if (lowered) *lowered = moved >> 32;
    return RT_OK;
}

}  // extern "C"
