/*
 * rt_mi355x.h — C-ABI boundary of the MI355X path tracer (librt_mi355x.so).
 *
 * Plain C: pointers, sizes and the byte-exact structs of rt_abi.h. No torch, no
 * HIP types in the signatures (streams travel as void*).
 *
 * What each entry point replaces in the reference (water-chika/ray-tracing-gpu-vulkan):
 *
 *   ray_trace()              src/ray_trace.h:5-15 / src/ray_trace.cpp:922-972 — same symbol and
 *                            signature; headless, renders once, honours `storeRenderResult`
 *                            (the reference accepts but ignores it, src/ray_trace.cpp:928) and
 *                            RETURNS (the reference loops until its window closes, :88/:567).
 *   rt_generate_scene()      src/scene.h:79-157 generateRandomScene(), with the wall-clock time
 *                            (:82-83) made an explicit argument and the 22x22 grid generalised to
 *                            a (2K)x(2K) grid (K = 11 is the reference scene; K = 158 is config 5).
 *   rt_canonical_render_call_info()
 *                            the RenderCallInfo the reference fills per frame,
 *                            src/ray_trace.cpp:660-676 (number 0, camera (13,11,-3) -> origin).
 *   rt_context_create() + rt_set_scene()
 *                            the per-frame scene upload + acceleration-structure build:
 *                            AABBs src/ray_trace.cpp:583-599, BLAS src/vulkan.h:395-453,
 *                            TLAS src/vulkan.h:463-554, rebuild src/vulkan.h:1020-1059,
 *                            UBO upload src/vulkan.h:1239-1254.
 *   rt_render_device()       the per-frame GPU work of one device: clear accumulator
 *                            (src/vulkan.h:1061-1106) + vkCmdTraceRaysKHR(W, band_h, 1)
 *                            (src/vulkan.h:994-995) executing shaders/shader.{rgen,rint,rchit,rmiss}.
 *                            Device pointers, caller's stream, asynchronous.
 *   rt_multi_*()             one process driving N devices (src/ray_trace.cpp:42-105 creates one
 *                            Vulkan device per GPU, :74-93 splits the image into bands): one RCCL
 *                            communicator over the devices (ncclCommInitAll; none for one device,
 *                            whose frame has no collective), the image tiled into row-exact
 *                            interleaved 8-row strips, every device's rows gathered to
 *                            device 0 over xGMI (grouped ncclSend/ncclRecv) and reordered there,
 *                            the rows re-dealt from measured device times between frames.
 *   rt_partition_*()         the row split and its re-deal (src/ray_trace.cpp:74-81 band extents,
 *                            src/workload_tuner.hpp:38-104 get_workload fed by the per-GPU frame
 *                            times of src/ray_trace.cpp:750-762), host only, for callers that run
 *                            one process per GPU (rtvk/dist.py).
 *   rt_render()              host-pointer convenience wrapper (one call = one frame); rci_count > 1
 *                            renders one band per GPU like src/ray_trace.cpp:74-93, gathered by RCCL.
 *
 * Error model: every rt_* call returns RT_OK (0) or a negative rt_status; the message of the
 * calling thread's last failure is rt_last_error(). Exceptions never cross this boundary (the
 * reference lets C++ exceptions escape its extern "C" function). ray_trace() has
 * no return value in the reference; it prints the error to stderr, as src/main.cpp:61-63 does.
 *
 * Threading: a context is thread-compatible (one call at a time per context); distinct contexts
 * may be used concurrently from distinct threads.
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stdbool.h>
#include <stdint.h>
#include "rt_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 2u

typedef enum rt_status {
    RT_OK = 0,
    RT_ERR_INVALID_ARGUMENT = -1,
    RT_ERR_DEVICE = -2,       /* a HIP runtime call failed                         */
    RT_ERR_OUT_OF_MEMORY = -3,
    RT_ERR_NO_SCENE = -4,     /* rt_render_device() before rt_set_scene()          */
    RT_ERR_IO = -5,           /* image store failed                                */
    RT_ERR_NO_DEVICE = -6     /* no HIP device visible                             */
} rt_status;

/* Per-pixel seed coordinates. */
typedef enum rt_seed_mode {
    RT_SEED_GLOBAL = 0,        /* seed = TEA(TEA(x_global, y_global), number): image independent of GPU count */
    RT_SEED_LAUNCH_LOCAL = 1   /* seed = TEA(TEA(launchID.x, launchID.y), number): shader.rgen:40 verbatim  */
} rt_seed_mode;

/* Random stream layout. */
typedef enum rt_rng_mode {
    RT_RNG_PIXEL_STREAM = 0,   /* reference: one LCG stream per pixel runs through every sample (random.glsl)   */
    RT_RNG_SAMPLE_COUNTER = 1, /* counter-based: sample s of a pixel starts at TEA(pixel_seed, s): samples of a
                                  pixel are independent and may be split across launches                        */
    RT_RNG_SAMPLE_HASH = 2     /* counter-based (the north star's RNG): sample s starts its LCG at
                                  lowbias32(pixel_seed + 0x9E3779B9 * s) and per-sample colours are summed in
                                  8.24 fixed point, so the library splits a pixel's samples into chunks run
                                  by any lanes in any order with bit-identical results;
                                  samplesPerRenderCall <= 2^19. The fixed point holds a sample colour
                                  channel in [0, 1] (a NaN channel counts 0): every sample colour is a
                                  product of sphere colours and the sky (0.7, 0.8, 1), so it lies in
                                  [0, 1] exactly when every colour a sphere can return does (colors[0],
                                  and colors[1] of checkered spheres). rt_render_device refuses a scene
                                  with a colour channel outside [0, 1] in this mode
                                  (RT_ERR_INVALID_ARGUMENT) instead of clipping it; the reference sums
                                  unclamped (shader.rgen:55-59): render such scenes with
                                  RT_RNG_PIXEL_STREAM.                                                      */
} rt_rng_mode;

/* Closest-hit search structure (the reference uses the driver's BVH, src/vulkan.h:395-554). */
typedef enum rt_accel {
    RT_ACCEL_AUTO = 0,         /* LBVH                                                   */
    RT_ACCEL_BRUTE = 1,        /* every sphere per segment, sphere list from the scalar cache */
    RT_ACCEL_LBVH = 2          /* linear BVH (Morton order, Karras hierarchy)            */
} rt_accel;

typedef struct rt_options {
    uint32_t max_depth;   /* segments per sample; 0 -> 50 (shader.rgen:27)                       */
    uint32_t seed_mode;   /* rt_seed_mode                                                        */
    uint32_t rng_mode;    /* rt_rng_mode                                                         */
    uint32_t accel;       /* rt_accel                                                            */
    uint32_t accumulate;  /* 0: clear the accumulator first (src/vulkan.h:1081-1086); 1: add on top */
    uint32_t sample_base; /* counter modes only: index of this launch's first sample               */
    uint32_t reserved[2]; /* 0 for production. Diagnostics / A/B only: reserved[0] bit 0 = count box
                             and sphere tests (slower instrumented build, rt_get_stats); bit 1 =
                             recompute every segment's closest hit by the gated brute force that
                             backs the deferred AABB gate (tests);
                             reserved[1] = LBVH walk form: 0 automatic (octant node copies in LDS
                             when they fit, else one copy in LDS, else an LDS treelet over L2
                             subtrees), 6 one LDS node copy, 8 octant copies, 10 every node from
                             L2, 12 the uniform grid, 14 the uniform grid in LDS with the
                             wave-cooperative walk, 16 the uniform grid in LDS
                             with the wave-wide candidate queue */
} rt_options;

/* Statistics of the last rt_render_device() on a context (valid after its stream completes). */
typedef struct rt_stats {
    uint64_t segments;      /* traced segments (one traceRayEXT each, shader.rgen:75)              */
    uint64_t samples;       /* camera samples                                                     */
    uint64_t box_tests;     /* LBVH node-box tests (0 for brute force)                             */
    uint64_t sphere_tests;  /* ray-sphere tests (shader.rint:44-60 evaluations)                    */
} rt_stats;

typedef struct rt_context rt_context;

/* ---- library ---------------------------------------------------------------------- */
uint32_t    rt_abi_version(void);
const char* rt_last_error(void);
int         rt_device_count(int* count);

/* ---- host data API (scene.h / render_call_info.h) --------------------------------- */
/* generateRandomScene(t) with a (2K)x(2K) grid: writes 4 + 4K^2 spheres (488 for K = 11). */
int rt_generate_scene(float t, uint32_t grid_half_extent, Sphere* out, uint32_t capacity,
                      uint32_t* count);
int rt_canonical_render_call_info(uint32_t spp, uint32_t width, uint32_t height,
                                  RenderCallInfo* out);

/* ---- device API ------------------------------------------------------------------- */
int rt_context_create(int device, rt_context** out);
int rt_context_destroy(rt_context* ctx);
/* Uploads `count` spheres (host memory) and builds the closest-hit structure: a binned-SAH tree
 * built on the host for scenes of up to 1024 spheres (the cheaper walk), the parallel device
 * LBVH build (rt_build.hip) + device grid above that. RT_BVH_BUILD=gpu|sah|morton forces one
 * builder (A/B). `spheres` may be reused as soon as it returns. Launches already queued render
 * the old scene; every later launch of ctx renders the new one, on any stream. Host-built scenes
 * are built while queued launches execute and uploaded in order on `stream`. Device builds run on
 * the context's own build stream into the one of two scene arenas that no queued launch reads
 * (the one used two scenes ago, whose launches they wait for), so frame k + 1's build overlaps
 * frame k's tail; the call returns once the build's summary is back on the host (no wait for
 * queued launches) and its grid build is queued.
 * Geometry: finite centres and radii of any sign or size are rendered as the CPU
 * oracle renders them (radius -r is the sphere of radius r, radius 0 is never hit, of coincident
 * spheres the lowest index wins). A sphere with a NaN or infinite centre or radius is refused:
 * RT_ERR_INVALID_ARGUMENT, rt_last_error() names the first such index, and ctx keeps the scene it
 * had. This holds for every scene call below, rt_multi_set_scene and ray_trace() alike. */
int rt_set_scene(rt_context* ctx, const Sphere* spheres, uint32_t count, void* stream);
/* As rt_set_scene, spheres already in DEVICE memory, written by earlier work on `stream` (the
 * build copies them after that work; the caller may reuse them once the call returns). */
int rt_set_scene_device(rt_context* ctx, const Sphere* d_spheres, uint32_t count, void* stream);
/*
 * Per-frame update of an animated scene (the reference rebuilds BLAS/TLAS every frame,
 * src/vulkan.h:1020-1059, because spheres move with t, src/scene.h:94-111): same count, new
 * positions / radii / materials; keeps the tree topology of the last device build and refits its
 * boxes, records and padding on the device. Without a device-built tree of the same count it
 * performs a full rt_set_scene. Rendering stays exact (any topology is), only walk cost changes.
 */
int rt_refit_scene(rt_context* ctx, const Sphere* spheres, uint32_t count, void* stream);
int rt_refit_scene_device(rt_context* ctx, const Sphere* d_spheres, uint32_t count, void* stream);
/*
 * Render one band on ctx's device, asynchronously on `stream` (hipStream_t; NULL = default).
 *   rci          host pointer; rci->offset / rci->image_size / camera / spp / number as in the UBO.
 *   rows         optional DEVICE array of band_height global row indices (strip tiling across
 *                GPUs); NULL means rows rci->offset.y + [0, band_height).
 *   accum_rgba32f / out_rgba8   DEVICE arrays of band_width * band_height texels, row-major by
 *                band row (the reference's per-band storage images, bindings 3 and 0).
 *   band_width, band_height < 65536 (RT_ERR_INVALID_ARGUMENT otherwise); 0 renders nothing.
 */
int rt_render_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows,
                     uint32_t band_width, uint32_t band_height, float* accum_rgba32f,
                     uint8_t* out_rgba8, const rt_options* opt, void* stream);
/*
 * Adaptive frame of the counter-based stream: "render to this noise level, at
 * most rci->samplesPerRenderCall (max_spp) samples per pixel". Pass 0 renders samples
 * [0, min_spp) on every 8x8 tile of the band; every later pass renders the next
 * min(step_spp, max_spp - done) samples on the tiles that have not converged. Each pass is two
 * trace launches, the first half of its samples into fixed-point half-buffer A and the second into
 * B; a tile converges when the difference of the two halves, summed over its in-band pixels and
 * channels, is small against their sum:
 *     E = sum |A - B|,  S = sum (A + B),  S' = S + n * 3 * m * 2^16   (n samples, m pixels)
 *     converged  iff  2^17 * E < thr_q16 * S',   thr_q16 = floor(threshold * 65536 + 0.5)
 * in exact integer arithmetic (rt_adaptive_tile_converged is the same function on the host).
 * Threshold 0 never converges (every tile reaches max_spp), threshold 16 always does after pass 0.
 * A pixel of a tile that stopped at n samples holds, bit for bit, what rt_render_device gives at
 * samplesPerRenderCall = n with the same options: accum = the sum, rgba8 = unorm8(sqrt(sum / n)).
 *   sample_count   optional DEVICE array of band_width * band_height uint32: n per texel.
 *   opt            rng_mode must be RT_RNG_SAMPLE_HASH and accumulate 0; sample_base + max_spp must
 *                  fit 32 bits; max_spp, min_spp and step_spp are even, min_spp <= max_spp <= 2^19.
 *   info           optional, filled on return.
 * Synchronisation: the call's device work is ordered on `stream` like rt_render_device's, but the
 * call is synchronous per pass: it blocks the host once per pass on a small readback of the next
 * pass's tile count (pinned memory, an event on `stream`, no device-wide synchronisation) and
 * returns once the final resolve is queued; the outputs are valid after `stream` completes.
 * rt_get_stats reports the last trace launch (the last half-pass) only, totals come back in
 * `info`; each half-pass counts as one launch for rt_launch_ms. Adaptive calls neither read nor
 * update the tile order of later rt_render_device launches and record no row weights.
 */
typedef struct rt_adaptive {
    uint32_t min_spp;    /* even, >= 2; samples every pixel gets                      */
    uint32_t step_spp;   /* even, >= 2; samples added per later pass                  */
    float    threshold;  /* finite, 0 <= threshold <= 16; see criterion               */
    uint32_t reserved;   /* 0 */
} rt_adaptive;
typedef struct rt_adaptive_info {
    uint32_t passes;          /* passes run (1 .. 1 + ceil((max-min)/step))          */
    uint32_t tiles;           /* 8x8 tiles of the band                               */
    uint32_t tiles_capped;    /* tiles that reached max_spp unconverged              */
    uint32_t reserved;
    uint64_t samples;         /* camera samples rendered (sum of in-band n)          */
} rt_adaptive_info;
int rt_render_adaptive_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows,
                              uint32_t band_width, uint32_t band_height, float* accum_rgba32f,
                              uint8_t* out_rgba8, uint32_t* sample_count, const rt_options* opt,
                              const rt_adaptive* ad, rt_adaptive_info* info, void* stream);
/* The stop criterion above for one tile (host only, no device needed): *converged = 1 or 0.
 * E, S < 2^56, n <= 2^19, 1 <= m <= 64 (RT_ERR_INVALID_ARGUMENT otherwise). */
int rt_adaptive_tile_converged(uint64_t E, uint64_t S, uint32_t n, uint32_t m, uint32_t thr_q16,
                               int* converged);
/*
 * Sample-map frames: "render this band with n[t] samples on 8x8 tile t". A sample
 * map of a band of W x H texels is one uint32 count per tile, row-major with ceil(W/8) tiles per
 * tile row (the layout of the adaptive tile table), each count in [0, 2^19], odd counts allowed.
 * Every in-band pixel of tile t holds, bit for bit, what rt_render_device gives at
 * samplesPerRenderCall = n[t] with the same options (RT_RNG_SAMPLE_HASH, accumulate 0): accum = the
 * float sum with w = 1, rgba8 = unorm8(sqrt(sum / float(n))), the optional per-texel count = n[t].
 * A tile with n = 0 is not traced: accum (0, 0, 0, 1), rgba8 (0, 0, 0, 255), the 0-sample frame.
 * Plan: with L_0 < ... < L_{J-1} the distinct non-zero counts (L_{-1} = 0, J <=
 * RT_SAMPLE_MAP_MAX_LEVELS, the launches rt_launch_ms keeps), the tiles sorted by (count descending,
 * tile index ascending) and c_j = #{t : n[t] >= L_j}, launch j renders samples [L_{j-1}, L_j) on the
 * first c_j tiles of that order: nested prefixes of one list, so every launch size is known before
 * the frame starts and the whole frame is queued without a host wait: J trace launches into one set
 * of fixed-point planes, then one resolve with the map as per-tile divisors.
 *
 * A map belongs to the context it was created on and must be destroyed before it. Setting it is the
 * one synchronous step: the call waits for the queued frames that read the map, copies the table to
 * the host behind the work queued on `stream`, plans it there (rt_sample_map_plan) and uploads the
 * order and the quantised table. `quantum` (0 or 1: none) rounds every non-zero count up to a
 * multiple of itself first: fewer launches for more samples. A count above 2^19 (before or after the
 * quantum; the message names the first such tile) or more than 64 levels (the message suggests a
 * quantum) is RT_ERR_INVALID_ARGUMENT and the map keeps what it held. info: optional.
 */
#define RT_SAMPLE_MAP_MAX_LEVELS 64u
typedef struct rt_sample_map rt_sample_map;
typedef struct rt_sample_map_info {
    uint32_t tiles, levels;        /* tiles of the band; J                                        */
    uint32_t min_count, max_count; /* smallest non-zero and largest count after quantum (0: none) */
    uint64_t samples;              /* sum over tiles of n x in-band pixels                        */
    uint64_t tile_launches;        /* sum of c_j                                                  */
} rt_sample_map_info;
int rt_sample_map_create(rt_context* ctx, uint32_t band_width, uint32_t band_height, rt_sample_map** out);
int rt_sample_map_destroy(rt_sample_map* map);
/* d_tile_counts: DEVICE array of ceil(W/8) * ceil(H/8) words, written by earlier work on `stream`. */
int rt_sample_map_set_device(rt_sample_map* map, const uint32_t* d_tile_counts, uint32_t quantum,
                             void* stream, rt_sample_map_info* info);
/* The count table of the context's last completed adaptive frame (rt_render_adaptive_device; its
 * band size must be the map's, RT_ERR_INVALID_ARGUMENT otherwise or without one). */
int rt_sample_map_set_from_adaptive(rt_sample_map* map, uint32_t quantum, void* stream,
                                    rt_sample_map_info* info);
/* The info of the last successful set call (zeros but `tiles` before one). */
int rt_sample_map_get_info(const rt_sample_map* map, rt_sample_map_info* out);
/*
 * The schedule of a map's frames. RT_SAMPLE_MAP_LEVELS (the default) is the plan above. Under
 * RT_SAMPLE_MAP_ONE_LAUNCH the whole frame is one trace launch of a block table, whatever the number
 * of distinct counts (no limit of 64): the tiles in the same order, those of count 0 dropped, a tile
 * of count n split into k = ceil(n / U) chunks, chunk c = samples [c n / k, (c + 1) n / k); the
 * table lists the chunks tile by tile, one 16-byte entry {tile, s0, s1, 0} per block of 64 units, so
 * the high-count tiles' ~U-sample units lead and the low-count tiles' single short units are the
 * tail. The image is the same bit for bit under either schedule.
 *   unit_samples   U: 0 = automatic, max(clamp(max_count / 32, 32, 128), ceil(sum of 64 n[t] /
 *                  (393 216 lanes x 128))), doubled until 64 x blocks < 2^31; else within [1, 2^19];
 *                  must be 0 with RT_SAMPLE_MAP_LEVELS.
 * The call takes effect at the next set call; the plan the map holds stays until then.
 * RT_ERR_INVALID_ARGUMENT: an unknown schedule, unit_samples above 2^19 or given with LEVELS. A set
 * call whose block table with the caller's U has 2^25 blocks or more is refused (the message names
 * the smallest U that fits) and leaves the map as it was. Under ONE_LAUNCH rt_sample_map_info.levels
 * holds the distinct non-zero counts (it may exceed 64) and tile_launches the non-zero tiles.
 */
#define RT_SAMPLE_MAP_LEVELS 0u
#define RT_SAMPLE_MAP_ONE_LAUNCH 1u
int rt_sample_map_set_schedule(rt_sample_map* map, uint32_t schedule, uint32_t unit_samples);
/* The schedule, U and block count of the plan the map holds (LEVELS, 0, 0 before a set call and for
 * a level plan); every output may be NULL. */
int rt_sample_map_get_schedule(const rt_sample_map* map, uint32_t* schedule, uint32_t* unit_samples_used,
                               uint64_t* n_blocks);
/*
 * One sample-map frame of a band, asynchronous on `stream`: arguments as rt_render_adaptive_device.
 * The call contains no host wait, no event synchronisation and no blocking copy; a map may be
 * rendered any number of times, on any stream of its context, between plain and adaptive calls.
 *   rci->samplesPerRenderCall   the frame's cap, as in adaptive frames: >= the map's max_count,
 *                  <= 2^19, and sample_base + samplesPerRenderCall must fit 32 bits.
 *   opt            rng_mode must be RT_RNG_SAMPLE_HASH and accumulate 0.
 * RT_ERR_INVALID_ARGUMENT before any work is queued (rt_last_error() names the field): rng_mode,
 * accumulate, a band size other than the map's, the cap, a map never set, a map of another context,
 * an adaptive frame open on ctx. RT_ERR_NO_SCENE before rt_set_scene.
 * Each level's launch counts as one launch for rt_launch_ms; rt_get_stats reports the last launch.
 * A one-launch map's frame is one launch for both: that launch is the whole frame.
 * Map frames neither read nor update the tile order of rt_render_device launches, record no row
 * weights and leave the count table of the last adaptive frame in place.
 */
int rt_render_sample_map_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows,
                                uint32_t band_width, uint32_t band_height, float* accum_rgba32f,
                                uint8_t* out_rgba8, uint32_t* sample_count, const rt_options* opt,
                                const rt_sample_map* map, void* stream);
/* The plan of a host table (host only, no device needed; what the two set calls compute): order and
 * quantised hold n_tiles words, levels and level_tiles RT_SAMPLE_MAP_MAX_LEVELS; every output may be
 * NULL. Refusals as the set calls'; nothing is written then. */
int rt_sample_map_plan(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum,
                       uint32_t* order, uint32_t* levels, uint32_t* level_tiles, uint32_t* n_levels,
                       uint32_t* quantised);
/* The block table of a host table under RT_SAMPLE_MAP_ONE_LAUNCH (host only; what the set calls
 * compute): blocks_out holds 4 words {tile, s0, s1, 0} per block, `capacity` blocks; every output may
 * be NULL (blocks_out NULL: a size query). Refusals as rt_sample_map_plan's but the level limit, plus
 * unit_samples above 2^19, a table of 2^25 blocks or more, a capacity below the table; nothing is
 * written then. */
int rt_sample_map_block_plan(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t quantum,
                             uint32_t unit_samples, uint32_t* blocks_out, uint64_t capacity,
                             uint64_t* n_blocks, uint32_t* unit_samples_used);
/*
 * The set call without a host wait: the count table stays on the device. Queued on `stream` behind
 * every frame already queued on the map (events), a device planner builds what
 * rt_sample_map_set_device builds on the host under RT_SAMPLE_MAP_ONE_LAUNCH: every count clamped to
 * count_cap (<= 2^19), the order, the clamped table the resolve divides by and the block table of
 * rt_sample_map_block_plan(clamped counts, 0, U). No quantum.
 *   unit_samples   U0: the first unit tried; 0 = clamp(count_cap / 32, 32, 128) (the floor of the
 *                  automatic unit; its other term needs the table's sum, which the host does not have).
 *                  U is the smallest U0 2^j (held at 2^19) whose table fits the map's block capacity,
 *                  min(tiles x ceil(count_cap / U0), 2^22 entries); rt_sample_map_device_unit below
 *                  computes the same on the host.
 * The map becomes "device-planned": the host knows count_cap alone, rt_render_sample_map_device checks
 * samplesPerRenderCall against count_cap and launches the full persistent grid, which reads the
 * table's size from device memory. rt_sample_map_get_info (tiles, max_count, samples, tile_launches;
 * levels and min_count are 0) and rt_sample_map_get_schedule copy the planner's summary back: they
 * wait for the planner, the one synchronisation such a map has, and it is optional. The planner's
 * buffers are allocated by the first call and the block table grows here only (a growth waits for
 * the frames that read the old one). A later rt_sample_map_set_device / set_from_adaptive makes the
 * map host-planned again. RT_ERR_INVALID_ARGUMENT: a NULL argument, count_cap or unit_samples above
 * 2^19, a band of more than 2^22 tiles; the map keeps what it held. A device error after the first
 * planner step leaves the map unset.
 */
int rt_sample_map_set_device_async(rt_sample_map* map, const uint32_t* d_tile_counts, uint32_t unit_samples,
                                   uint32_t count_cap, void* stream);
/* The unit the device planner chooses for a host table (host only): the smallest unit0 2^j (unit0 = 0:
 * as above), held at 2^19, whose block table of min(count, count_cap) has at most `capacity` entries.
 * RT_ERR_INVALID_ARGUMENT: a NULL table, count_cap or unit0 above 2^19, more non-zero tiles than
 * `capacity` (no unit fits); *unit_used is not written then. */
int rt_sample_map_device_unit(const uint32_t* tile_counts, uint32_t n_tiles, uint32_t count_cap, uint32_t unit0,
                              uint64_t capacity, uint32_t* unit_used);
/*
 * The feedback rule of sample maps (host only, exact integers): a tile whose n
 * samples were rendered as two halves has E, S, m as in rt_adaptive_tile_converged; with
 *   hot  = !converged(E, S, n, m, thr_q16),  cold = converged(E, S, n, m, thr_q16 >> 1)
 * its next count is hot ? min(max_spp, 2 n) : cold ? max(min_spp, (n / 2 + 1) & ~1) : n; n = 0 stays 0.
 * E, S < 2^56, n <= 2^19, 1 <= m <= 64, min_spp and max_spp even with 2 <= min_spp <= max_spp <= 2^19
 * (RT_ERR_INVALID_ARGUMENT otherwise).
 */
int rt_sample_map_feedback_count(uint64_t E, uint64_t S, uint32_t n, uint32_t m, uint32_t thr_q16,
                                 uint32_t min_spp, uint32_t max_spp, uint32_t* next);
/*
 * A feedback frame: the map renders, measures its own noise and plans its
 * successor on the device; nothing is read back and the call contains no host wait (the buffers'
 * first allocation and growth aside). Arguments as rt_render_sample_map_device, plus:
 *   fb             threshold (finite, within [0, 16]), min_spp and max_spp (even, 2 <= min_spp <=
 *                  max_spp <= 2^19, max_spp <= samplesPerRenderCall), unit_samples (the planner's U0,
 *                  0: automatic), reserved 0.
 *   d_tile_error   optional DEVICE array of 2 x tiles uint64: (E, S) of every tile of this frame.
 * samplesPerRenderCall (the cap) must be even and at least what the map holds. The frame:
 *   0. on a map not yet planned for feedback at this cap (a host-set one, one set by
 *      rt_sample_map_set_device_async): its current counts are planned in halves mode first: every
 *      count rounded up to even, n = 2 h, the block table of the h table over [0, h) (the A half)
 *      followed by the same entries over [h, n) (the B half);
 *   1. the A half renders into one set of fixed-point planes, the B half into a second (two launches);
 *   2. per tile, E and S of rt_adaptive_tile_converged from the two, and its next count by
 *      rt_sample_map_feedback_count;
 *   3. the resolve sums both, divides by the map's counts and zeroes both; accum, rgba8 and
 *      sample_count are those of rt_render_sample_map_device at the rendered (even) counts;
 *   4. the next counts are planned in halves mode: the map now holds them.
 * rt_render_sample_map_device on such a map renders both halves in one launch: the same image.
 * RT_ERR_INVALID_ARGUMENT before any work is queued: rt_render_sample_map_device's refusals, an odd
 * cap or one below max_spp, the threshold, min_spp / max_spp, unit_samples above 2^19.
 */
typedef struct rt_sample_map_feedback {
    float threshold;
    uint32_t min_spp, max_spp;
    uint32_t unit_samples;
    uint32_t reserved;
} rt_sample_map_feedback;
int rt_render_sample_map_feedback_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows,
                                         uint32_t band_width, uint32_t band_height, float* accum_rgba32f,
                                         uint8_t* out_rgba8, uint32_t* sample_count, const rt_options* opt,
                                         rt_sample_map* map, const rt_sample_map_feedback* fb,
                                         uint64_t* d_tile_error, void* stream);
/*
 * The hand-over of the two halves. Adaptive and feedback frames sum the first
 * half of every tile's samples into fixed-point planes A and the second into planes B; the two calls
 * below are rt_render_adaptive_device and rt_render_sample_map_feedback_device with one more
 * argument, and their resolve (the same single pass over the planes) also writes the halves, in the
 * form the variance-guided filter and the temporal stage read a frame. With qA, qB the per-channel
 * 8.24 integers the plane sets hold when the frame resolves and n the texel's tile count (even in
 * both frame kinds), per band texel in band order (a row map is honoured exactly as for accum):
 *   accum_a    = (float(double(qA.r) * 2^-24), float(double(qA.g) * 2^-24), float(double(qA.b) * 2^-24), 1)
 *   accum_b    likewise from qB
 *   half_count = n / 2
 *   accum_rgba32f, out_rgba8, sample_count, info and d_tile_error exactly as the calls without
 *   halves write them, from qA + qB.
 * What the halves hold:
 *   Feedback frame. A tile of count n = 2 h at sample_base = b has A = samples [b, b + h) and B =
 *     [b + h, b + n): accum_a equals rt_render_device at samplesPerRenderCall = h, sample_base = b in
 *     every texel of the tile, bit for bit, and accum_b the same call at sample_base = b + h (the
 *     uniform frame's resolve is the same float(double(q) * 2^-24)). A tile of count 0 gives
 *     (0, 0, 0, 1) twice and h = 0.
 *   Adaptive frame. A tile that ran passes of k_0 = min_spp, k_1, ... samples starting at d_0 = 0,
 *     d_1 = k_0, ... has A = the samples of the union over j of [b + d_j, b + d_j + k_j / 2) and B =
 *     the rest of [b, b + n); h = n / 2.
 * RT_ERR_INVALID_ARGUMENT before anything is queued (rt_last_error() names the field), beside the
 * refusals of the calls without halves: halves NULL, accum_a or accum_b NULL, reserved not NULL,
 * accum_a == accum_b, either equal to accum_rgba32f. rt_half_outputs_check is these checks alone
 * (host only, no device and no context needed). Everything else is the plain calls': synchronisation,
 * launch records, what they leave in the context (the planes are zero afterwards); a feedback halves
 * frame still contains no host wait.
 * The planes feed the filters unchanged: rt_denoise_variance_device(accum_a, accum_b, half_count, ...)
 * and rt_temporal_accumulate_device / rt_temporal_reproject_device(accum_a, accum_b, sample_count =
 * half_count, ...), see there.
 */
typedef struct rt_half_outputs {
    float*    accum_a;     /* DEVICE float4 per band texel: (sum of the A half, 1)    */
    float*    accum_b;     /* DEVICE float4 per band texel: (sum of the B half, 1)    */
    uint32_t* half_count;  /* optional DEVICE uint32 per band texel: h = n[tile] / 2  */
    void*     reserved;    /* NULL */
} rt_half_outputs;
int rt_half_outputs_check(const rt_half_outputs* halves, const float* accum_rgba32f);
int rt_render_adaptive_halves_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows,
                                     uint32_t band_width, uint32_t band_height, float* accum_rgba32f,
                                     uint8_t* out_rgba8, uint32_t* sample_count, const rt_options* opt,
                                     const rt_adaptive* ad, rt_adaptive_info* info,
                                     const rt_half_outputs* halves, void* stream);
int rt_render_sample_map_feedback_halves_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows,
                                                uint32_t band_width, uint32_t band_height, float* accum_rgba32f,
                                                uint8_t* out_rgba8, uint32_t* sample_count, const rt_options* opt,
                                                rt_sample_map* map, const rt_sample_map_feedback* fb,
                                                uint64_t* d_tile_error, const rt_half_outputs* halves,
                                                void* stream);
/* Statistics of the last completed rt_render_device (synchronises ctx's last stream). */
int rt_get_stats(rt_context* ctx, rt_stats* out);
/* Trace-kernel duration (ms, HIP events on the launch stream) of ctx's launch `back` launches
 * before its most recent one (0 = the most recent; the last 64 are kept). Waits for that launch's
 * end only, not for launches queued after it: a frame loop reads the launch of two frames ago
 * without draining its queue (the per-GPU frame times the reference's tuner reads,
 * src/ray_trace.cpp:636-644, :750-762). */
int rt_launch_ms(rt_context* ctx, uint32_t back, float* ms);
/* Per band row of the same launch (one of ctx's last 4 grid / LBVH launches; band_rows = its band
 * height), the row's share of the launch's work as its 8x8 tile-cost record estimates it (each
 * tile's longest unit chain x the sample chunks it ran in, split evenly over the tile's rows; the
 * unit is arbitrary, only ratios matter). Waits for that launch's record copy only. A context
 * copies its launches' records (two small device-to-host copies after each kernel) only from the
 * first call on, so the first call finds none (RT_ERR_INVALID_ARGUMENT); rt_multi's contexts keep
 * them from the start when it drives more than one device. */
int rt_launch_row_weights(rt_context* ctx, uint32_t back, double* weights, uint32_t band_rows);
/*
 * Scatter band rows into a full image on the device: dst_row[rows[i]] = src_row[i]
 * (the reorder after the multi-GPU gather). dst has dst_rows rows of `width`
 * texels; map entries >= dst_rows are skipped.
 */
int rt_scatter_rows(rt_context* ctx, const float* src_accum, const uint8_t* src_rgba8,
                    const uint32_t* rows, uint32_t n_rows, uint32_t width, uint32_t dst_rows,
                    float* dst_accum, uint8_t* dst_rgba8, void* stream);

/*
 * Gather full-image rows into a band on the device: dst_row[i] = src_row[rows[i]] (the inverse
 * of rt_scatter_rows: the running sums an accumulating multi-GPU frame hands each device). src
 * has src_rows rows of `width` float4 texels; map entries >= src_rows leave their band row as is.
 */
int rt_gather_rows(rt_context* ctx, const float* src_accum, const uint32_t* rows, uint32_t n_rows,
                   uint32_t width, uint32_t src_rows, float* dst_accum, void* stream);

/*
 * Tonemap a summed accumulator to rgba8 on the device, exactly as the trace kernel's store
 * (shader.rgen:65-66): rgba8 = round(clamp(sqrt(sum / spp), 0, 1) * 255) per channel, alpha 255.
 * spp 0 is accepted and gives the bytes the trace kernel stores for a 0-sample frame.
 * accum_rgba32f: n_texels float4 (DEVICE); out_rgba8: n_texels x 4 bytes (DEVICE).
 */
int rt_resolve_rgba8(rt_context* ctx, const float* accum_rgba32f, uint64_t n_texels, uint32_t spp,
                     uint8_t* out_rgba8, void* stream);

/*
 * First-hit feature buffers: what a denoiser is guided by. For texel p of the
 * band and every s in [opt->sample_base, opt->sample_base + feature_samples), the call traces
 * exactly the camera ray rt_render_device traces for sample s under RT_RNG_SAMPLE_HASH (the same
 * pixel seed, the same two jitter draws and lens draws; seed_mode, rows, rci->offset and
 * rci->number are honoured alike) to its closest hit under the geometry contract ((t, lowest id),
 * tmin / tmax, the AABB gate) and ends there. Per sample, by the expressions the shading uses
 * (p = fma(t, d, o), outward = normalize(p - c), front = dot(d, outward) < 0, the checker):
 *     hit:   albedo = colors[0], or colors[1] where a checkered sphere's checker is not positive;
 *            n = front ? outward : -outward;  depth = t;  hit = 1
 *     miss:  albedo = (0.7, 0.8, 1.0);  n = 0;  depth = 0;  hit = 0
 *     feat0[p] = (sum albedo.rgb, sum hit)     feat1[p] = (sum n.xyz, sum depth)
 * Each sum is a binary32 sum in ascending s that starts from the first sample's value: the order is
 * part of the contract (one lane runs all samples of a pixel), so the buffers are bit-exact
 * functions of the scene, the camera and the sample range.
 *   feat0, feat1      DEVICE float4 arrays of band_width * band_height texels.
 *   feature_samples   1 .. RT_FEATURE_MAX_SAMPLES; independent of the frame's samples per pixel
 *                     (primary rays are cheap: 16 is a good default under 4-64 spp frames).
 *   opt               rng_mode must be RT_RNG_SAMPLE_HASH and accumulate 0 (RT_ERR_INVALID_ARGUMENT
 *                     otherwise); accel and the reserved words select the walk as for a frame;
 *                     max_depth is unused.
 * Asynchronous on `stream` like rt_render_device, without a host wait. A features launch is one
 * launch for rt_launch_ms and rt_get_stats, but it neither reads nor updates the tile order, tile
 * costs and row weights of the context's frames.
 */
#define RT_FEATURE_MAX_SAMPLES 256u
int rt_render_features_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows,
                              uint32_t band_width, uint32_t band_height, float* feat0, float* feat1,
                              uint32_t feature_samples, const rt_options* opt, void* stream);
/*
 * Edge-avoiding a-trous denoise of a summed accumulator, guided by the feature buffers above
 * (DESIGN.md §3.1.3). The band's rows must be contiguous image rows (there is no `rows` argument:
 * the filter's taps are the band's own neighbours), band_width, band_height < 65536. Every operation
 * is one correctly rounded binary32 + - x /, in this order (a restatement on the CPU gives the same
 * bits, tests/denoise_sim.py):
 *     n_p = sample_count ? sample_count[p] : spp;   c = n_p ? accum.rgb / float(n_p) : 0
 *     a = feat0.rgb / float(F);  nrm = feat1.xyz / float(F);  z = feat1.w / float(F)
 *     e_0 = c / (a + 2^-6)                                                   (per channel)
 *     iteration i = 0 .. iterations - 1, step = 1 << i; taps dy = -2..2 (outer), dx = -2..2 (inner),
 *     q = p + step * (dx, dy), taps outside the band skipped:
 *         dn = nrm_p - nrm_q;  dn2 = (dn.x dn.x + dn.y dn.y) + dn.z dn.z
 *         dz = (z_p - z_q) / (z_p + 1)
 *         de = e_i(p) - e_i(q);  de2 = (de.x de.x + de.y de.y) + de.z de.z
 *         x  = ((1 + k_normal dn2) (1 + k_depth (dz dz))) (1 + (k_color 4^i) de2)
 *         w  = (K[|dy|] K[|dx|]) / (x x),   K = {3/8, 1/4, 1/16}
 *         num += w e_i(q);  den += w                      (both from 0, taps in order)
 *     e_{i+1}(p) = num / den
 *     mean = e_I (a + 2^-6);  rgba8 = rt_resolve_rgba8 of (mean, 1) at spp 1
 *   sample_count      optional DEVICE array of band_width * band_height uint32 (as
 *                     rt_render_adaptive_device writes it); NULL: every texel has `spp` samples.
 *   feat0, feat1, feature_samples   as rt_render_features_device wrote them.
 *   params            NULL: {3, 4.0f, 16.0f, 1.0f}.
 *   out_mean_rgba32f  optional DEVICE float4 array: (mean, 1) per texel; out_rgba8: required.
 * One kernel per iteration on `stream`, nothing waits on the host; the two intermediate float4
 * band buffers belong to the context and grow on demand (the growth of an existing buffer drains
 * `stream` once). rt_denoise_check is the call's parameter check alone (host only, no device).
 */
typedef struct rt_denoise {
    uint32_t iterations;               /* 1 .. 6 */
    float k_normal, k_depth, k_color;  /* finite, >= 0 */
} rt_denoise;
int rt_denoise_check(const rt_denoise* params, uint32_t band_width, uint32_t band_height,
                     uint32_t feature_samples);
int rt_denoise_device(rt_context* ctx, const float* accum_rgba32f, const uint32_t* sample_count, uint32_t spp,
                      const float* feat0, const float* feat1, uint32_t feature_samples, uint32_t band_width,
                      uint32_t band_height, const rt_denoise* params, float* out_mean_rgba32f,
                      uint8_t* out_rgba8, void* stream);
/*
 * Variance-guided denoise: the filter above with a colour weight scaled by a
 * per-texel variance, estimated from two half-buffers of the frame and carried through the
 * iterations, so that one setting serves noisy and nearly converged frames alike. accum_a and
 * accum_b are two summed accumulators of the same band, each holding h_p samples of texel p:
 * h_p = half_count ? half_count[p] : half_spp. A uniform frame of n = 2 h spp is two
 * rt_render_device calls with samplesPerRenderCall = h under RT_RNG_SAMPLE_HASH, one at
 * sample_base = b and one at sample_base = b + h; a sample-map frame is two
 * rt_render_sample_map_device frames whose sample_base differ by the cap, and half_count is the
 * sample_count plane either writes; an adaptive or feedback frame rendered once hands its own two
 * halves over (rt_half_outputs above): rt_denoise_variance_device(accum_a, accum_b, half_count, ...),
 * a texel of h = 0 has ma = mb = 0. Every operation is one correctly rounded binary32 + - x /, in
 * this order (tests/denoise_var_sim.py gives the same bits); taps, their order and the borders are
 * rt_denoise_device's, K = {3/8, 1/4, 1/16}:
 *     hf = float(h_p);  ma = h_p ? A.rgb / hf : 0;  mb = h_p ? B.rgb / hf : 0
 *     a = feat0.rgb / float(F) + 2^-6;  nrm = feat1.xyz / float(F);  z = feat1.w / float(F)
 *     e_0 = ((ma + mb) * 0.5) / a                                            (per channel)
 *     d   = (ma - mb) / a;   v_0 = 0.25 * ((d.x d.x + d.y d.y) + d.z d.z)
 *     f(p, q) = (1 + k_normal dn2) (1 + k_depth (dz dz))      dn2, dz as in rt_denoise_device
 *     prefilter pass j = 0 .. prefilter - 1, step = 1 << j (e unchanged):
 *         w = (K[|dy|] K[|dx|]) / (f f);   nv += w v(q);   den += w
 *         v'(p) = nv / den
 *     iteration i = 0 .. iterations - 1, step = 1 << i, v_i the prefiltered variance at i = 0:
 *         de = e_i(p) - e_i(q);  de2 = (de.x de.x + de.y de.y) + de.z de.z
 *         x  = f (1 + k_color (de2 / (v_i(p) + 2^-20)))
 *         w  = (K[|dy|] K[|dx|]) / (x x)
 *         num += w e_i(q);  den += w;  nv += (w w) v_i(q)
 *         e_{i+1}(p) = num / den;      v_{i+1}(p) = nv / (den den)
 *     mean = e_I a;   rgba8 = rt_resolve_rgba8 of (mean, 1) at spp 1
 * k_color is not scaled by 4^i: the tracked variance shrinks as the filter converges. The centre
 * tap has x = 1, so den > 0.
 *   half_count        optional DEVICE array of band_width * band_height uint32; NULL: half_spp.
 *   params            NULL: {3, 2, 4.0f, 16.0f, 0.25f}.
 *   out_mean_rgba32f  optional DEVICE float4 array: (mean, 1) per texel; out_rgba8: required.
 * Refusals are rt_denoise_check's, and prefilter > 3. prefilter + iterations kernels on `stream`,
 * nothing waits on the host; the band buffers are those of rt_denoise_device, with its one
 * exception. rt_denoise_variance_check is the parameter check alone (host only).
 */
typedef struct rt_denoise_variance {
    uint32_t iterations;               /* 1 .. 6 */
    uint32_t prefilter;                /* 0 .. 3 feature-only passes over the variance */
    float k_normal, k_depth, k_color;  /* finite, >= 0 */
} rt_denoise_variance;
int rt_denoise_variance_check(const rt_denoise_variance* params, uint32_t band_width, uint32_t band_height,
                              uint32_t feature_samples);
int rt_denoise_variance_device(rt_context* ctx, const float* accum_a, const float* accum_b,
                               const uint32_t* half_count, uint32_t half_spp, const float* feat0,
                               const float* feat1, uint32_t feature_samples, uint32_t band_width,
                               uint32_t band_height, const rt_denoise_variance* params,
                               float* out_mean_rgba32f, uint8_t* out_rgba8, void* stream);
/*
 * Temporal accumulation: a stage between the render and the two filters above
 * for frame loops. A state object keeps, per texel of its band, the demodulated colour integrated
 * over the frames before, the number of frames it holds and the first-hit guide of the last frame;
 * one call blends the current frame into it wherever the guide still matches and starts over where
 * it does not, and writes accumulators the filters read as they read a frame's. The state of a band
 * of W x H texels is three float4 planes owned by the object:
 *     HA = (eA.rgb, n)    HB = (eB.rgb, n)    HG = (nrm.xyz, z)
 * n, the history length, is held as a float (exact up to 65 535) and is 0 after create and after
 * reset. Every operation is one correctly rounded binary32 + - x /, in this order
 * (tests/temporal_sim.py gives the same bits); no neighbour is read, the update is in place:
 *     h   = sample_count ? sample_count[p] : spp;   hf = float(h)
 *     cA  = h ? A.rgb / hf : 0                          (cB likewise when accum_b is given)
 *     a   = feat0.rgb / float(F) + 2^-6;  nrm = feat1.xyz / float(F);  z = feat1.w / float(F)
 *     eA  = cA / a                                                           (per channel)
 *     dn  = nrm - HG.xyz;  dn2 = (dn.x dn.x + dn.y dn.y) + dn.z dn.z
 *     dz  = (z - HG.w) / (z + 1)
 *     x   = (1 + k_normal dn2) (1 + k_depth (dz dz))
 *     valid = HA.w > 0 and x < 2
 *     h == 0 (no measurement this frame):
 *         valid ? (e' = the history, n' = HA.w) : (e' = 0, n' = 0)
 *     h > 0:
 *         n' = valid ? min(HA.w + 1, float(max_history)) : 1;   alpha = 1 / n'
 *         eA' = valid ? HA.rgb + alpha (eA - HA.rgb) : eA     (eB' with HB, the same valid and alpha)
 *     HA = (eA', n');  HB = (eB', n');  HG = (nrm, z)          (the guide is always the current one)
 *     out_a = (eA' a, 1);  out_b = (eB' a, 1)
 *     out_rgba8 = rt_resolve_rgba8 at spp 1 of the mean: ((eA' + eB') * 0.5) a with two accumulators,
 *                 eA' a with one
 *     history_len[p] = uint32(n')
 * Feeding the filters: out_a alone is an accumulator at 1 sample, which rt_denoise_device takes with
 * spp = 1; out_a and out_b are two halves at half_spp = 1 for rt_denoise_variance_device. Both halves
 * are integrated with the same weights, so they stay independent estimates of equal weight and
 * |A - B|^2 / 4 stays a variance estimate of their mean.
 * Sample ranges: the caller renders every frame from a disjoint sample range (sample_base += spp per
 * frame; under two halves, the halves of frame k at k spp and k spp + spp / 2), or the frames repeat
 * one another's noise and integrating them gains nothing. The features are rendered at the SAME
 * sample_base every frame: a static scene then gives bit-identical guides, x = 1 exactly, and every
 * texel is valid.
 *   accum_a, accum_b  DEVICE float4 arrays of the state's band, summed accumulators of h_p samples
 *                     each; accum_b optional: NULL is one accumulator, HB is then neither read nor
 *                     written and out_b must be NULL too (and the reverse).
 *   sample_count      optional DEVICE array of uint32 per texel; NULL: every texel has `spp` samples.
 *                     The halves of an adaptive or feedback frame (rt_half_outputs above) go in as
 *                     (accum_a, accum_b, sample_count = half_count), here and in
 *                     rt_temporal_reproject_device; the frames' sample_base advances by the cap.
 *   feat0, feat1, feature_samples   as rt_render_features_device wrote them.
 *   params            NULL: {8, 4.0f, 16.0f, 0}.
 *   out_a, out_b      DEVICE float4 arrays; out_rgba8 (4 bytes per texel) and history_len (uint32 per
 *                     texel): optional.
 * The call has no band-size arguments: the band is the state's own, and every array holds that many
 * texels. One kernel launch on `stream`, nothing waits on the host and nothing is allocated: the
 * planes are allocated by rt_temporal_create. RT_ERR_INVALID_ARGUMENT before anything is queued, with
 * rt_last_error() naming the field: rt_denoise_check's size and feature-sample limits, max_history
 * outside 2 .. 65535, a k that is negative or not finite, reserved not 0, a state of another context,
 * out_b without accum_b or the reverse, a required pointer that is NULL. A state belongs to the
 * context it was created on and must be destroyed before it, as a sample map. rt_temporal_reset sets
 * n = 0 everywhere, queued on `stream` without a host wait: the next call is a first frame.
 * rt_temporal_check is the parameter check alone (host only, no device).
 * Not part of the stage: weighting frames by their sample counts, sharing the pass with the filters'
 * prologue. This call compares a texel with itself a frame ago (a texel whose surface changed starts
 * over); under camera or object motion use rt_temporal_reproject_device below.
 */
typedef struct rt_temporal rt_temporal;
typedef struct rt_temporal_params {
    uint32_t max_history;     /* 2 .. 65535: the blend weight never falls below 1 / max_history */
    float k_normal, k_depth;  /* finite, >= 0 */
    uint32_t reserved;        /* 0 */
} rt_temporal_params;
int rt_temporal_create(rt_context* ctx, uint32_t band_width, uint32_t band_height, rt_temporal** out);
int rt_temporal_destroy(rt_temporal* temporal);
int rt_temporal_reset(rt_temporal* temporal, void* stream);
int rt_temporal_check(const rt_temporal_params* params, uint32_t band_width, uint32_t band_height,
                      uint32_t feature_samples);
int rt_temporal_accumulate_device(rt_context* ctx, rt_temporal* temporal, const float* accum_a, const float* accum_b,
                                  const uint32_t* sample_count, uint32_t spp, const float* feat0,
                                  const float* feat1, uint32_t feature_samples, const rt_temporal_params* params,
                                  float* out_a, float* out_b, uint8_t* out_rgba8, uint32_t* history_len,
                                  void* stream);

/* ---- temporal reprojection: a motion pass and a history that follows it ------
 * The motion pass answers, for every texel of a band, where the surface seen through the texel's
 * CENTRE stood in the previous frame's image. A motion object (rt_motion) belongs to one context, as a
 * temporal state does, and must be destroyed before it. It owns the pass's device scratch, one ray (6
 * floats) and one (winner, t) answer (8 bytes) per texel of its band, and the PREVIOUS frame: its
 * RenderCallInfo (the camera) and one float4 per sphere id whose xyz is the sphere's centre.
 *   rt_motion_set_previous   sets the previous frame from host spheres (their geometry.xyz) and its
 *                            RenderCallInfo; copied before the call returns, uploaded on `stream`.
 *   rt_motion_keep_current   makes the context's current scene and `rci` the previous frame: a device
 *                            to device copy of the scene's id-indexed centres on `stream`, ordered
 *                            behind the scene's upload or device build. A frame loop calls
 *                            rt_render_motion_device, then rt_motion_keep_current, every frame.
 * Before either call the previous frame is the current one (nothing moved). Spheres only translate:
 * sphere i of the previous frame is sphere i of this one. If the previous frame holds another number of
 * spheres than the current scene, ids mean other spheres and every texel that hits one gets ok = 0.
 * The previous frame's image_size must be the current one's.
 *
 * rt_render_motion_device writes motion_out, a DEVICE float4 per texel of the object's band: band_h
 * contiguous image rows of band_w texels from rci->offset (no row map: the stage that reads the plane
 * reads neighbours). Three launches on `stream`, no host wait: (1) the pinhole ray through each
 * texel's centre, camera_ray's expressions without the jitter draws,
 *     gx = offset.x + x;  ux = float(double(float(gx) + 0.5f) * (1.0 / double(image_size.x)));  uy likewise
 *     to = (ulc + ux hor) - uy ver;   o = lf;   v = to - lf
 * (2) the closest hit (id, t) of every ray by the walk `opt` selects as for a frame (accel and the
 * walk-form words; everything else of opt is ignored, NULL: the defaults), exactly as a frame's
 * primary ray finds it; (3) the motion, binary32, one operation per step, dot(a, b) = fma(a.z, b.z,
 * fma(a.y, b.y, a.x b.x)), with (lf', hor', ver', ulc') the previous frame's camera and the launch
 * constants u = ulc' - lf', wn = cross(hor', ver') = (hor'.y ver'.z - hor'.z ver'.y, ...), k = dot(u, wn),
 * ihh = 1 / dot(hor', hor'), ivv = 1 / dot(ver', ver') computed on the host in the same arithmetic:
 *     d   = normalize(v) = v * (1 / sqrt(dot(v, v)))
 *     hit:   p = fma(t, d, o);  q = (p - c_now[id]) + c_prev[id];  r = q - lf'
 *            (another sphere count in the previous frame: q = p)
 *     miss:  r = d                                       (the sky is a point at infinity)
 *     den = dot(r, wn);  s = k / den;  rel = s r - u
 *     sx  = ((dot(rel, hor') ihh) float(image_size.x)) - float(offset.x)
 *     sy  = ((-(dot(rel, ver') ivv)) float(image_size.y)) - float(offset.y)
 *     dzm = hit ? sqrt(dot(r, r)) - t : 0       (how far the surface's distance to the camera changed)
 *     ok  = den > 0 and sx, sy finite and not (hit and another sphere count)
 *     motion[p] = (sx, sy, dzm, ok ? 1 : 0)
 * (sx, sy) are band coordinates of the previous frame's image in which texel (x, y)'s centre is
 * (x + 0.5, y + 0.5): a texel nothing moved for gets its own centre back to within rounding (far below
 * 2^-6 of a texel, the snap of the call below). tests/motion_sim.py gives the same bits.
 * RT_ERR_INVALID_ARGUMENT before anything is queued, with rt_last_error() naming the field: the band
 * limits of rt_denoise_check (and a band of 0 texels for rt_motion_create), a NULL pointer, an
 * image_size of 0, a previous frame of another image_size, a motion object of another context, an
 * unknown accel, a call between the halves of a scene build; RT_ERR_NO_SCENE before rt_set_scene.
 * rt_motion_check is the host-only part of these checks (no device, no context).
 */
typedef struct rt_motion rt_motion;
int rt_motion_create(rt_context* ctx, uint32_t band_width, uint32_t band_height, rt_motion** out);
int rt_motion_destroy(rt_motion* motion);
int rt_motion_set_previous(rt_motion* motion, const Sphere* spheres, uint32_t count, const RenderCallInfo* prev_rci,
                           void* stream);
int rt_motion_keep_current(rt_context* ctx, rt_motion* motion, const RenderCallInfo* rci, void* stream);
int rt_motion_check(uint32_t band_width, uint32_t band_height, const RenderCallInfo* rci,
                    const RenderCallInfo* prev_rci);
int rt_render_motion_device(rt_context* ctx, rt_motion* motion, const RenderCallInfo* rci, float* motion_out,
                            const rt_options* opt, void* stream);

/* rt_temporal_reproject_device is rt_temporal_accumulate_device with the history of a texel fetched
 * from where `motion` (rt_render_motion_device's plane of the state's band) says its surface was: the
 * arguments, the parameters, the outputs and every line of that call's arithmetic hold, except that
 * (HA, HB, `valid`) of texel p are replaced as follows, binary32, one operation per step:
 *     (sx, sy, dzm, ok) = motion[p];   bx = sx - 0.5;  by = sy - 0.5
 *     jx = floor(bx + 0.5);  jy = floor(by + 0.5)
 *     snap = |bx - jx| <= 2^-6 and |by - jy| <= 2^-6
 *     snap:       one tap (jx, jy) of weight 1
 *     otherwise:  ix = floor(bx);  fx = bx - ix;  gx = 1 - fx  (y likewise);
 *                 taps (ix, iy) (ix + 1, iy) (ix, iy + 1) (ix + 1, iy + 1)
 *                 of weights gx gy, fx gy, gx fy, fx fy, in this order
 *     ze = z + dzm
 *     tap q of weight w counts iff ok > 0, w > 0, q lies inside the band, HA[q].w > 0 and
 *         (1 + k_normal dn2) (1 + k_depth (dz dz)) < 2  with dn = nrm - HG[q].xyz,
 *         dn2 = (dn.x dn.x + dn.y dn.y) + dn.z dn.z,  dz = (ze - HG[q].w) / (ze + 1)
 *     Wt = the sum of the counting taps' w;  S = the sum of their w HA[q] (all four components);
 *     SB = the sum of their w HB[q].rgb: each sum starts at 0 and adds its terms in tap order, a tap
 *     that does not count adding 0
 *     valid = Wt > 0;   HA = S / Wt;   HB.rgb = SB / Wt              (per component; HA.w is the history's n)
 * The snap is part of the contract, not a tuning knob: a texel whose surface did not move keeps its own
 * history unblurred (one tap of weight 1: S / Wt is HA[q] as stored), so on a static scene the call
 * equals rt_temporal_accumulate_device bit for bit. n, a weighted mean, need not be an integer:
 * history_len = uint32(n') truncates. HG = (nrm, z) of the current frame, as before.
 * The call reads neighbours, so it cannot update the planes in place: the state holds a second set of
 * its three planes, the call reads the current set, writes the other and makes that one current.
 * rt_temporal_accumulate_device works in place on whichever set is current and rt_temporal_reset clears
 * it; the two calls may be mixed on one state. With one accumulator HB is neither read nor written, so
 * the HB of the set written keeps what an earlier call left there. The second set is allocated by the
 * state's first reprojected call, the only one that may wait on the host; every later call is one
 * kernel launch on `stream`. Refusals as rt_temporal_accumulate_device's, and motion NULL.
 * tests/temporal_reproject_sim.py gives the same bits.
 */
int rt_temporal_reproject_device(rt_context* ctx, rt_temporal* temporal, const float* accum_a, const float* accum_b,
                                 const uint32_t* sample_count, uint32_t spp, const float* feat0, const float* feat1,
                                 uint32_t feature_samples, const float* motion, const rt_temporal_params* params,
                                 float* out_a, float* out_b, uint8_t* out_rgba8, uint32_t* history_len,
                                 void* stream);

/* ---- multi-device (one process, N GPUs, RCCL over xGMI) ----------------------------- */
typedef struct rt_multi rt_multi;
/* Devices 0 .. n-1, n = min(gpu_count, visible devices) (>= 1): one context and one stream per
 * device and, for n > 1, one RCCL communicator over them (ncclCommInitAll); one device renders
 * straight into the caller's buffers and builds no communicator. */
int rt_multi_create(uint32_t gpu_count, rt_multi** out);
int rt_multi_destroy(rt_multi* m);
int rt_multi_device_count(const rt_multi* m, uint32_t* n);
/* The scene on every device (host spheres), as rt_set_scene: every device's build is issued before
 * any is waited for (device builds run on all GPUs at once), and a host-built scene is built once
 * and uploaded to every device. */
int rt_multi_set_scene(rt_multi* m, const Sphere* spheres, uint32_t count);
/*
 * One frame of the whole image rci->image_size (rci->offset ignored). The rows start as
 * rt_partition_strips' row-exact strips (device d renders its rows through rt_render_device with
 * a rows map, global seeds) and are re-dealt between frames: each frame reads every device's
 * trace-kernel time of the frame two before (rt_launch_ms), rescales per-row cost estimates to
 * them and moves band-end rows from the slowest device to the fastest (rt_partition_rebalance's
 * rule; the move rewrites rows maps only, waiting for queued frames once); every other device's
 * float4 accumulator rows travel to device 0 in one RCCL group
 * (ncclSend / ncclRecv; device 0's own strips never go through RCCL) and are reordered into
 * accum_rgba32f, then device 0 tonemaps the whole accumulator into out_rgba8 (rt_resolve_rgba8:
 * the rgba8 bytes are a function of the float sum, so they are not sent). accum_rgba32f /
 * out_rgba8: DEVICE pointers on device 0, W*H texels. Asynchronous on `stream` (a hipStream_t of
 * device 0; NULL = the legacy stream): the call returns once everything is queued. The image
 * equals the one-device image bit for bit.
 * opt->accumulate: as rt_render_device, the frame adds to what accum_rgba32f holds when the call's
 * work starts on `stream`, at every device count (device 0 sends each device the running sums of
 * its strips first). One device holding every row renders straight into the caller's buffers (no
 * strip copy, no reorder, no resolve). The frame plan is rt_debug_multi_plan's
 * (include/rt_mi355x_debug.h).
 */
int rt_multi_render(rt_multi* m, const RenderCallInfo* rci, const rt_options* opt,
                    float* accum_rgba32f, uint8_t* out_rgba8, void* stream);
/*
 * One adaptive frame of the whole image over the devices (rci->offset ignored, global seeds): the
 * N-device form of rt_render_adaptive_device, equal to its one-device frame bit for bit
 * (accumulator, rgba8, counts and info). opt and ad follow rt_render_adaptive_device's rules
 * (RT_RNG_SAMPLE_HASH, accumulate 0, even counts, threshold in [0, 16]); every refusal comes
 * before any render work is queued; RT_ERR_NO_SCENE before rt_multi_set_scene.
 * The image is dealt as whole 8-row tile rows (rt_partition_tile_rows: the criterion is per 8x8
 * tile), tile row k on device k % n, statically: adaptive frames are not re-dealt, add nothing to
 * the balancer's history and leave the plain frames' partition and buffers alone. Device d renders
 * its part on the context its plain frames use, with its own rows map; its tiles converge on that
 * device alone. One host thread drives every device: a device's next pass is issued as soon as
 * that device's own small readback has landed (the per-context events are polled, the thread
 * yields between polls), so the devices do not move in lock step. Then one RCCL group brings each
 * remote part's float4 accumulator rows and its per-tile count table (ceil(W/8) * ceil(rows/8)
 * 32-bit words) to device 0 (device 0's own part never goes through RCCL), and one fused kernel
 * per part stores accumulator, rgba8 = unorm8(sqrt(sum / float(n))) and the optional counts at
 * their rows: no row scatter and no whole-image resolve. One device, or device 0 holding every
 * row: rt_render_adaptive_device straight into the caller's buffers.
 *   accum_rgba32f / out_rgba8 / sample_count (optional, W*H uint32): DEVICE pointers on device 0.
 *   info (optional): the frame's totals: passes = the maximum over the devices, tiles,
 *   tiles_capped and samples = the sums.
 * Synchronisation as rt_render_adaptive_device: the host blocks on the per-pass readbacks only,
 * the call returns once the final stores are queued, the outputs are valid after `stream`
 * completes. The frame plan is rt_debug_multi_plan_adaptive's (include/rt_mi355x_debug.h).
 */
int rt_multi_render_adaptive(rt_multi* m, const RenderCallInfo* rci, const rt_options* opt,
                             const rt_adaptive* ad, float* accum_rgba32f, uint8_t* out_rgba8,
                             uint32_t* sample_count, rt_adaptive_info* info, void* stream);
/* The last adaptive frame's numbers of one device (the imbalance the static deal leaves); zeros
 * for a device that rendered nothing. */
int rt_multi_adaptive_device_info(const rt_multi* m, uint32_t device, rt_adaptive_info* out);
/* Sum over the devices of the last frame's statistics (synchronises). */
int rt_multi_stats(rt_multi* m, rt_stats* out);
/* {devices, ranks of the RCCL communicator (ncclCommCount; 0 for one device: no communicator),
 * rows per strip, devices that rendered rows in the last frame}. */
int rt_multi_info(const rt_multi* m, uint32_t* out4);
/* Trace-kernel duration (ms, HIP events on the launch stream) of the last frame on each device
 * that rendered rows, in device order; *count = devices written (synchronises). */
int rt_multi_kernel_times(rt_multi* m, float* out_ms, uint32_t capacity, uint32_t* count);
/* The same for each of the last `frames` frames (at most 64): out_ms[f * devices + d], oldest frame
 * first; *count = frames x devices that rendered rows (synchronises). */
int rt_multi_kernel_times_frames(rt_multi* m, uint32_t frames, float* out_ms, uint32_t capacity, uint32_t* count);
/* The partition the next frame renders with: counts[d] rows on device d (n entries), and with rows
 * non-NULL (capacity >= image height) the rows, device 0's first, each device's in band order.
 * Set up by the first rt_multi_render of an image size (all counts 0 before it). */
int rt_multi_partition(const rt_multi* m, uint32_t* rows, uint32_t* counts, uint32_t capacity);

/* ---- row partition across devices (host only, no device needed) --------------------- */
/* A partition of `height` rows over n devices is rows[] (height entries: device 0's rows, then
 * device 1's, ...; each device's in band order) + counts[] (n entries).
 * rt_partition_strips: the row-exact interleaved strips every multi-device frame starts from: the
 * rows of the R = floor(height / (8 n)) full rounds are 8-row strips dealt round robin (strip k on
 * device k % n), the rest are n contiguous runs (the first (rest % n) one row longer), run d on
 * device d; every device holds floor(height / n) or ceil(height / n) rows (the reference gives the
 * remainder to the first band, src/ray_trace.cpp:74-81). */
int rt_partition_strips(uint32_t n_devices, uint32_t height, uint32_t* rows, uint32_t* counts);
/* rt_partition_tile_rows: the static partition of adaptive frames (rt_multi_render_adaptive), same
 * layout and error rules. The T = ceil(height / 8) tile rows [8k, min(8k + 8, height)) are dealt
 * round robin, tile row k on device k % n; each device's rows ascend and the ragged last tile row
 * is globally last, so band tile row j of a device is exactly one global tile row. A device beyond
 * T gets count 0. */
int rt_partition_tile_rows(uint32_t n_devices, uint32_t height, uint32_t* rows, uint32_t* counts);
/* One balancing step (src/workload_tuner.hpp:38-104, without its random moves and without the
 * teardown, src/ray_trace.cpp:774): with a measurement (meas_rows / meas_counts: the partition a
 * frame ran with, meas_ms: each device's trace-kernel ms of that frame; all three NULL for none),
 * row_cost (height doubles, ms per row; <= 0: unknown, in / out) is rescaled so that each measured
 * device's rows sum to its time (unknown rows at the mean of its known ones). Then rows / counts
 * (the current partition, in / out) are re-dealt: while the most loaded device is above
 * (1 + tolerance) x the mean load, one of its last min(8, rows) band rows moves to the end of
 * another device's band, or is swapped with one of that band's last rows, whichever exchange
 * leaves the pair's larger load lowest, as long as it lowers the most loaded device's load by
 * more than tolerance x the mean. Deterministic: every rank of a one-process-per-GPU job that calls it with
 * the same inputs gets the same partition. *moved = rows moved; *predicted_imbalance = max / mean
 * load afterwards (either may be NULL). */
int rt_partition_rebalance(uint32_t n_devices, uint32_t height, uint32_t* rows, uint32_t* counts, double* row_cost,
                           const uint32_t* meas_rows, const uint32_t* meas_counts, const float* meas_ms,
                           double tolerance, uint32_t* moved, double* predicted_imbalance);

/* ---- host-pointer convenience ------------------------------------------------------ */
/*
 * One frame over the full image rci[0].image_size with host buffers. rci_count bands, band i
 * spanning rows [rci[i].offset.y, rci[i+1].offset.y) (last band to image height), band i on
 * device i % device_count, gathered to device 0 by RCCL (rt_multi), then copied to the host. Each
 * band renders and is tonemapped with its own RenderCallInfo (its own samplesPerRenderCall, as the
 * reference fills one per GPU, src/ray_trace.cpp:660-676).
 * accum_rgba32f: W*H*4 floats (read first when opt->accumulate), out_rgba8: W*H*4 bytes.
 */
int rt_render(const Sphere* spheres, uint32_t sphere_count, const RenderCallInfo* rci,
              uint32_t rci_count, float* accum_rgba32f, uint8_t* out_rgba8,
              const rt_options* opt, rt_stats* stats);

/* Writes an rgba8 image as binary PPM (P6, alpha dropped). */
int rt_store_ppm(const char* path, const uint8_t* rgba8, uint32_t width, uint32_t height);

/* Build provenance of this library: "sources_sha256=<16 hex of the sources it was compiled
 * from>;arch=<offload arch>;flags=<compiler flags>;variant=<A/B variant flags, empty for the
 * shipped build>". Static string. */
const char* rt_build_info(void);

/* src/ray_trace.h:9-15 — identical symbol and parameter list. Renders the canonical scene once
 * (t = 0) on min(gpu_count, visible) GPUs through rt_multi (row-exact strips, RCCL gather, global
 * seeds, so the image does not depend on gpu_count), prints the frame time, stores `render.ppm`
 * when storeRenderResult, and returns. Random stream: the reference's per-pixel LCG stream, or
 * RT_RNG_SAMPLE_HASH when the environment holds RT_RNG=hash (the signature has no parameter for
 * it; any other RT_RNG value than "stream" / "hash" is reported and nothing renders). */
void ray_trace(uint32_t samples, bool storeRenderResult, uint32_t width, uint32_t height,
               uint32_t gpu_count);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_MI355X_H */
