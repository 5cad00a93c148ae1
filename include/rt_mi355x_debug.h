/*
 * rt_mi355x_debug.h — diagnostic and A/B entry points of librt_mi355x.so.
 *
 * Not part of the drop-in boundary (include/rt_mi355x.h is what replaces src/ray_trace.h): the
 * same library exports these for the test suite, bench.py and the A/B scripts (instrumented
 * counters, per-launch timing, launch-plan tuning, the multi-GPU frame plan). Production callers
 * never need them; none of them changes an image.
 */
#ifndef RT_MI355X_DEBUG_H
#define RT_MI355X_DEBUG_H

#include "rt_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic (tests only): evaluates one arithmetic-contract primitive on `device` for n
 * (x, y) pairs: op 0 sqrt(x), 1 x/y, 2 sin(x), 3 fma(x,y,1), 4 normalize(x,y,0.5).x, 5 pow(x,5),
 * 6 sample_seed_hash(bits(x), bits(y)) as bits, 7 / 8 low / high word of the 8.24 fixed-point
 * value of colour x, as bits, 9 checker decision at (x, y, 0.5 (x - y)) as 1 / 0, 10 normalize(x,y,0.5).y
 * as the kernels compute it (by sqrt_rcp_cr, length and reciprocal from one v_rsq_f32, in a build with
 * -DRT_NORMALIZE_RSQ=1), 11 the same by v_sqrt_f32 then v_rcp_f32, which op 10 must equal bit for bit. */
int rt_debug_math(int device, int op, const float* in_pairs, float* out, uint32_t n);
/* Diagnostic (tests only): the kernels' cheap correctly rounded operations against hipcc's
 * correctly rounded ones on `device`: rcp_cr(x) vs 1.0f / x and sqrt_cr(x) vs sqrtf(x) over all 2^32
 * binary32 inputs (mismatches3[0], [1]; NaN == NaN), and the camera's float(double(x) * (1 /
 * double(b))) vs x / b for every binary32 x in [0, 65536) and eleven image sizes b (mismatches3[2]). */
int rt_debug_exact_exhaustive(int device, uint64_t* mismatches3);
/* Diagnostic (tests only): normalize's length and reciprocal from one v_rsq_f32 (csrc/rt_device_math.h
 * sqrt_rcp_cr) over all 2^32 binary32 inputs x on `device`, NaN == NaN: out4[0] mismatches of the
 * length against sqrtf(x), out4[1] of the reciprocal against 1.0f / sqrtf(x), out4[2] of the square
 * root alone by the same chain (sqrt_rsq) against sqrtf(x), out4[3] the x in [2^-100, 2^100] that
 * took the rare branch (the v_sqrt_f32 / v_rcp_f32 form). */
int rt_debug_exact_normalize_exhaustive(int device, uint64_t* out4);
/* Durations (ms) of the trace kernel of ctx's most recent launches (at most 64 are kept), oldest
 * first, from HIP events recorded on the launch stream around the kernel itself (not the resolve):
 * a caller times K launches inside its own timed region and reads them afterwards. *count =
 * min(capacity, launches kept). Synchronises on those events. */
int rt_debug_kernel_times(rt_context* ctx, float* out_ms, uint32_t capacity, uint32_t* count);
/* Diagnostic (tests, A/B timing): sets one launch-plan parameter of ctx (value -1 restores the
 * default). None of them changes an image; the defaults are the measured best. Keys: "grid" (0: no
 * uniform grid), "grid_scale", "grid_coop" (1: wave-cooperative grid walk), "grid_cq" (1: wave-wide
 * candidate queue), "grid_rec" (0: no
 * shading records in LDS), "grid_full_slack", "units_per_lane", "unit_min_samples",
 * "sample_chunks", "head_chunks", "tail_tiles_pm", "schedule" (0 LPT, 1 row-major, 2 LPT by tile
 * sum), "refill_reserve", "isolate_tiles", "sah_knobs", "camera_batches" (0: the unit loop instead
 * of the camera-batch form of the LDS grid kernel). Unknown keys: RT_ERR_INVALID_ARGUMENT.
 * Scene-build keys (grid, grid_scale, sah_knobs) apply from the next rt_set_scene. Values other
 * than -1 must be finite and within [0, 2^32]: RT_ERR_INVALID_ARGUMENT otherwise. The library
 * reads no environment variable for any of them. */
int rt_debug_tune(rt_context* ctx, const char* key, double value);
/* Diagnostic: of ctx's last launch, {sample chunks per pixel (low 16 bits: of the LPT order's tail
 * tiles; high 16 bits: of its head tiles, 0 when the launch had no head), the kernel form it ran
 * (low 16 bits: rt_internal.h ACCEL_*, before any launch the scene's default form; bit 16: its
 * grid walk was the one-layer form, the grid one cell thick in y; bit 17: its camera rays started
 * at the camera position itself, the pinhole shortcut; bit 18: it ran the camera-batch form of the
 * LDS grid kernel), its dynamic LDS bytes, CU count}. */
int rt_debug_launch_info(rt_context* ctx, uint32_t* out4);
/* The single-device launch plan (csrc/rt_launch.h): every host decision that shapes a trace launch,
 * as a function of plain inputs. `inputs` is an rt::launch::Inputs and `plan` an rt::launch::Plan,
 * both flat structs of 4-byte words followed by doubles whose first two words are the layout
 * version (1) and the struct's size (rtvk/abi.py LaunchInputs / LaunchPlan mirror them); in_bytes /
 * plan_bytes must equal those sizes.
 * ctx NULL: computes *plan from *inputs. Host only, no device needed: the kernels' answers (block
 * sizes, the one-layer grid form, occupancies) come from the tables inside *inputs. The inputs must
 * lie in the domain rt_render_device and rt_debug_tune admit (band 1 .. 65535 each way, known accel
 * and rng_mode, tuning values -1 or within [0, 2^32]); a band of 2^26 tiles is refused with "band
 * too large", an occupancy the table does not answer with RT_ERR_DEVICE.
 * ctx given: copies out the inputs and the plan of ctx's last launch, the inputs with the
 * occupancies that launch queried, so the ctx-NULL call on them gives the same plan. (After an
 * adaptive frame: its last pass, whose tile list is not part of the inputs.) RT_ERR_INVALID_ARGUMENT
 * before the first launch of a scene. */
int rt_debug_launch_plan(rt_context* ctx, void* inputs, uint64_t in_bytes, void* plan, uint64_t plan_bytes);
/* Whether rt_render_device runs the camera-batch form of the LDS grid kernel (csrc/rt_launch.h
 * camera_batches) for the launch that rt_debug_launch_plan(NULL, inputs, ...) plans.
 * Host only. tune: the value of rt_debug_tune's "camera_batches" (-1: the default); max_depth: the
 * options' (0: 50); table: a block-table launch; kernel_blocks: blocks per CU of the form's kernel
 * as the device answers (< 0: not asked). out3 = {0 when the form is taken, else the first reason
 * against it (rt_launch.h BATCH_OFF_*: 1 the tuning value, 2 not the counter-based stream, 3 a table
 * launch, 4 instrumented, 5 another kernel form, 6 no pinhole_lf, 7 max_depth, 8 the two-block LDS
 * budget, 9 the kernel's occupancy), the kernel's static LDS bytes, static + dynamic LDS bytes}. */
int rt_debug_camera_batches(void* inputs, uint64_t in_bytes, double tune, uint32_t max_depth, uint32_t table,
                            int kernel_blocks, uint32_t* out3);
/* The per-row weights rt_launch_row_weights derives from a launch's tile-cost record (csrc/rt_launch.h
 * row_weights), on hand-made arrays. Host only. cost: n tile records, row-major, tiles_x per tile
 * row; order: the n tiles in the order they were handed out, or NULL; head_tiles / head_chunks /
 * chunks: the launch's split of that order; weights: band_h doubles. A tile the order does not
 * name (an entry >= n is skipped) counts as rank 0; tiles_x 0 gives zeros. */
int rt_debug_row_weights(const uint32_t* cost, const uint32_t* order, uint32_t n, uint32_t tiles_x, uint32_t band_h,
                         uint32_t head_tiles, uint32_t head_chunks, uint32_t chunks, double* weights);
/* Diagnostic: per-phase cycle sums of ctx's last launch, filled only by -DRT_STAMPS builds. */
int rt_debug_stamps(rt_context* ctx, uint64_t* out8);
/* Diagnostic: lane utilisation of ctx's last launch per kernel code point k (0..15), filled only by
 * -DRT_UTIL builds: out32[2k] wave passes through the point, out32[2k + 1] active lanes summed. */
int rt_debug_util(rt_context* ctx, uint64_t* out32);
/* Diagnostic: histogram of LBVH box tests per segment of the last instrumented launch
 * (options.reserved[0] & 1), 2 x 64 bins: [0] segments that miss, [1] segments that hit. */
int rt_debug_walk_hist(rt_context* ctx, uint64_t* out128);
/* Diagnostic: walk work (cells + references) of ctx's last instrumented launch per segment pass,
   max over the wave's tracing lanes [0] and over its bounce (depth > 0) lanes [1], summed over
   passes; the primary (depth 0) lanes' summed work [2] and their count [3]. */
int rt_debug_walk_split(rt_context* ctx, uint64_t* out4);
/* Diagnostic: of ctx's last instrumented launch of a grid walk, {cells visited, visited cells that
 * hold no reference}. */
int rt_debug_grid_cells(rt_context* ctx, uint64_t* out2);
/* Diagnostic: segment-loop iterations of the last instrumented launch by the number of lanes
 * (0..64) of the wave tracing in that iteration (the persistent kernel's lane occupancy), then
 * three s_memrealtime stamps (100 MHz): first wave start, pixel queue dry, last wave exit. */
int rt_debug_lane_hist(rt_context* ctx, uint64_t* out68);
/* Diagnostic: tail steals of ctx's last instrumented launch (options.reserved[0] & 1;
 * RT_RNG_SAMPLE_HASH: once the work queue is empty, an idle lane takes half of the samples its
 * wave's busiest lane has not started). */
int rt_debug_steals(rt_context* ctx, uint64_t* out);
/* Diagnostic: per 8x8 tile of ctx's last LBVH launch, the traced segments of its most expensive
 * pixel (the key its next launch over the same band geometry hands tiles out by, longest
 * first); *count = tiles (ceil(W/8) x ceil(H/8), row-major), 0 before the first launch. */
int rt_debug_tile_cost(rt_context* ctx, uint32_t* out, uint64_t capacity, uint64_t* count);

/* Diagnostic (tests): what the device holds of a sample map after its last set call, copied back:
 * order and quantised (the map's tile count of words each, either may be NULL) from device memory,
 * levels and level_tiles (RT_SAMPLE_MAP_MAX_LEVELS words each, either may be NULL) from the host
 * plan the launches are sized by (of a one-launch plan with more levels, the lowest
 * RT_SAMPLE_MAP_MAX_LEVELS). Waits for the frames queued on the map. */
int rt_debug_sample_map(const rt_sample_map* map, uint32_t* order, uint32_t* levels, uint32_t* level_tiles,
                        uint32_t* quantised);
/* Diagnostic (tests): the block table the device holds of a map set under RT_SAMPLE_MAP_ONE_LAUNCH,
 * copied back: 4 words {tile, s0, s1, 0} per block into `out` (`capacity` blocks; NULL: a size
 * query), *n = blocks (0 for a level plan). Waits for the frames queued on the map. */
int rt_debug_sample_map_blocks(const rt_sample_map* map, uint32_t* out, uint64_t capacity, uint64_t* n);
/* (For a device-planned map, rt_sample_map_set_device_async, the count is the planner's: the call
 * waits for the planner.) Tests: the next rt_sample_map_set_device_async calls of `map` plan for a
 * block capacity of at most max(limit, tiles) entries, so that a small table shows the doubling of
 * the unit (0: the map's own capacity). */
int rt_debug_sample_map_limit_blocks(rt_sample_map* map, uint64_t limit);
/* The block hand-out rule the host plan and the device share (csrc/rt_hand_out.h; host only): of
 * n_units units, the last `reserve` go out one by one, the others as whole 64-unit blocks, the first
 * of them to the grid's `grid_waves` waves by wave id. */
int rt_debug_hand_out(uint32_t n_units, uint64_t reserve, uint64_t grid_waves, uint32_t* n_block_units,
                      uint32_t* first_blocks);
/* Host waits so far inside ctx's calls that are documented as queued without one: the growth of the
 * adaptive planes and of a device-planned map's block table behind queued work. */
int rt_debug_host_waits(rt_context* ctx, uint64_t* n);
/* Tests: what the feedback frames of `map` left on the device: the counts the last frame's update
 * chose (`next`, tiles words; optional) and the tiles all its frames raised and lowered. Waits for
 * the work queued on the map. */
int rt_debug_sample_map_feedback(rt_sample_map* map, uint32_t* next, uint64_t* raised, uint64_t* lowered);
/* The rt_sample_map_info a set call would report for a host table over a band (host only). */
int rt_debug_sample_map_info(const uint32_t* tile_counts, uint32_t band_width, uint32_t band_height,
                             uint32_t quantum, rt_sample_map_info* out);

/* Diagnostic (tests): copies one scene array of ctx to host memory. what: 0 geometry records,
 * 1 radii, 2 material records, 3 big-sphere ids, 4 LBVH nodes (padded), 5 LBVH nodes (unpadded),
 * 6 leaf geometry, 7 leaf ids, 8 info {u32 n_spheres, n_big, n_nodes, n_leaf_slots,
 * device_built, 0; f32 small_rmax, scene_radius}, 9 grid {u32 cells in x, y, z, cells, references}
 * (zeros without a grid). *bytes = the array's size; RT_ERR_INVALID_ARGUMENT when it exceeds
 * capacity. */
int rt_debug_scene(rt_context* ctx, uint32_t what, void* out, uint64_t capacity, uint64_t* bytes);
/* Diagnostic (tests): the closest hit of n given rays in ctx's scene, by the production walk of the
 * form `options` selects (accel, reserved[1] the form, reserved[0] bit 1 force_regate, as
 * rt_render_device reads them; its other fields are ignored, NULL: zeros). rays6: n host rays {ox,
 * oy, oz, vx, vy, vz}; the direction traced is the kernels' normalize(v), as for every segment of a
 * frame, and every value must be finite and each v have a nonzero component (RT_ERR_INVALID_ARGUMENT
 * otherwise, as for n above 2^24). The launch goes through the launch plan of a frame whose camera
 * lies at the batch's largest |o| (form choice, cull slacks, the far-camera re-pad, the grid's
 * refusal beyond its pad radius) and runs the form's trace kernel with a ray per unit, and
 * rt_debug_launch_info reports it like any other launch. out_id[i]: the winning sphere of ray i,
 * 0xffffffff for none; out_t[i]: its t (unspecified on a miss). Synchronous. n = 0: RT_OK, nothing
 * written; RT_ERR_NO_SCENE before rt_set_scene. Leaves the images and the hand-out order of the
 * frames around it alone. A batch with an origin beyond the radius the tree's node boxes are padded
 * for re-pads them for it, as a frame with a far camera does, and ctx keeps the wider boxes (more
 * conservative culling, the same answers) until its next rt_set_scene. */
int rt_debug_closest_hits(rt_context* ctx, const float* rays6, uint32_t n, const rt_options* options,
                          uint32_t* out_id, float* out_t);
/* Diagnostic (tests): one bounce of n given hits in ctx's scene by the frames' own shading code (the
 * function every hit of a frame is shaded by), a lane per case. Case i: host ray rays6[6 i ..] = {ox,
 * oy, oz, vx, vy, vz}, traced along the kernels' d = normalize(v), hit sphere ids[i] at t[i] with the
 * LCG (random.glsl) in state seeds[i]. Outputs, host arrays: out_p[3 i ..] the hit point fma(t, d, o),
 * out_att the attenuation, out_sd the scatter direction as the shader leaves it, out_dnext the
 * direction the next segment of a frame would be traced along (normalize of it; zeros when the bounce
 * does not scatter), out_scatter[i] 1 / 0, out_seed[i] the LCG state after the bounce. form: where the
 * sphere's records come from, 0 the scene's global arrays (the tree, brute and L2 grid kernels'
 * load), 1 the static LDS record table staged as the REC grid kernels stage it (scenes of at most
 * 512 spheres). RT_ERR_INVALID_ARGUMENT: a NULL array, a ray value or t that is not finite, a
 * direction without a nonzero component, ids[i] >= the scene's spheres, n above 2^24, an unknown form
 * or form 1 on a larger scene. n = 0: RT_OK, nothing written; RT_ERR_NO_SCENE before rt_set_scene.
 * Synchronous. Goes through no launch plan: frames, the tile-cost record and the hand-out order of
 * the frames around it are left alone, and rt_debug_launch_info still describes the last frame. */
int rt_debug_scatter(rt_context* ctx, const float* rays6, const uint32_t* ids, const float* t, const uint32_t* seeds,
                     uint32_t n, uint32_t form, float* out_p, float* out_att, float* out_sd, float* out_dnext,
                     uint32_t* out_scatter, uint32_t* out_seed);

/*
 * The multi-device frame plan rt_multi_render (band_starts NULL: its first frame's row-exact strips,
 * rt_partition_strips) or rt_render (band i = rows [band_starts[i], band_starts[i+1]) on device
 * i % n_devices) executes for a width x height frame, with or without accumulation. Host only (no
 * device needed). Flat u32 form: {n_parts, n_steps}, per part {device, whole, n_rows, rows...},
 * per step {op, device, peer, part, flags, count low, count high}; ops 1 load rows (device 0:
 * caller accumulator -> part buffer), 2 RCCL group start, 3 send, 4 receive, 5 group end,
 * 6 render (flags bit 0: straight into the caller's buffers), 7 store rows (part buffer -> caller
 * accumulator), 8 resolve rgba8 (count texels); send / receive counts are floats. out NULL: size
 * query (*count = words).
 */
int rt_debug_multi_plan(uint32_t n_devices, uint32_t width, uint32_t height, const uint32_t* band_starts,
                        uint32_t n_bands, uint32_t accumulate, uint32_t* out, uint64_t capacity,
                        uint64_t* count);
/* The same plan for an explicit partition (rows / counts as rt_partition_strips writes them: every
 * row of [0, height) exactly once), e.g. one the balancer re-dealt. */
int rt_debug_multi_plan_rows(uint32_t n_devices, uint32_t width, uint32_t height, const uint32_t* rows,
                             const uint32_t* counts, uint32_t accumulate, uint32_t* out, uint64_t capacity,
                             uint64_t* count);
/* The plan of an adaptive frame (rt_multi_render_adaptive) over rt_partition_tile_rows' parts, same
 * flat form (a device without a tile row has no part). Ops: 9 adaptive render (flags bit 0:
 * straight into the caller's buffers; the parts' passes are interleaved), 2 / 5 the group, 3 / 4
 * send / receive of a part's accumulator rows (floats), 10 / 11 send / receive of its per-tile
 * sample counts (32-bit words), 12 the fused store of a part (accumulator, rgba8, counts; count =
 * floats). No op 8: there is no whole-image resolve. */
int rt_debug_multi_plan_adaptive(uint32_t n_devices, uint32_t width, uint32_t height, uint32_t* out,
                                 uint64_t capacity, uint64_t* count);
/* Tests on a one-GPU box: an rt_multi of n_devices LOGICAL devices, all on device 0 (one context
 * and one stream each), executing the same frame plans as rt_multi_create's, with every RCCL
 * send / receive pair of a group replaced by one device copy on the receiver's stream, ordered
 * after the sender's earlier work and before its later work (the group boundaries of the plan).
 * No communicator (rt_multi_info reports 0 ranks). */
int rt_debug_multi_create_logical(uint32_t n_devices, rt_multi** out);
/* The same logical devices with the transfers through RCCL itself: one communicator of one rank on
 * device 0 (ncclCommInitAll), every group's sends and receives issued as ncclSend / ncclRecv of
 * rank 0 to itself on logical device 0's stream (fenced by events against every logical device's
 * stream before and after the group), so the one-GPU pool runs rt_multi's RCCL branch: the
 * communicator, the grouped calls and their buffers (rt_multi_info reports 1 rank). */
int rt_debug_multi_create_logical_rccl(uint32_t n_devices, rt_multi** out);
/* The balancer of m's strip frames: "balance" (1 on, 0 off), "tolerance" (re-deal above
 * (1 + tolerance) x the mean device time, by exchanges that gain more than tolerance x the mean;
 * default 0.001), "blend" (weight in (0, 1] of a new measurement in the per-row estimates, above 1
 * taken as 1; default 0.5), "lag" (frames between the measured frame and the one it re-deals, 1 to
 * 8; default 2); -1 restores the default. Other values: RT_ERR_INVALID_ARGUMENT. */
int rt_debug_multi_tune(rt_multi* m, const char* key, double value);
/* Feeds n device times (ms) as if measured on the current partition: the next rt_multi_render
 * re-deals from them instead of its own measurement (tests: forced re-deals). */
int rt_debug_multi_feedback(rt_multi* m, const float* device_ms, uint32_t n);
/* {strip frames rendered since the partition was set up, re-deals, rows moved, predicted max / mean
 * device time after the last re-deal}. */
int rt_debug_multi_balance_info(const rt_multi* m, double* out4);
/* The kernel form of rt_denoise_device and of rt_denoise_variance_device, its prefilter passes
 * included (A/B and tests; the image does not depend on it): iterations of
 * step <= max_step stage their taps in LDS, the others read them from global memory. 0 (every
 * iteration from global memory), 1, 2 or 4 (the default); other values: RT_ERR_INVALID_ARGUMENT. */
int rt_debug_denoise_lds_steps(rt_context* ctx, uint32_t max_step);
/* Timing: the resolve of adaptive and feedback frames alone, one launch on `stream`, over the context's
 * fixed-point planes as they stand (zero between frames, and zero again afterwards) with `count` as
 * every tile's count. halves NULL: the plain resolve; else rt_half_outputs' rules and the resolve that
 * also hands the halves over. The outputs are band_width x band_height texels, sample_count optional.
 * Forgets the count table of the last adaptive frame. Refused while an adaptive frame is open. */
int rt_debug_adaptive_resolve(rt_context* ctx, uint32_t band_width, uint32_t band_height, uint32_t count,
                              float* accum_rgba32f, uint8_t* out_rgba8, uint32_t* sample_count,
                              const rt_half_outputs* halves, void* stream);

#ifdef __cplusplus
}  /* extern "C" */
#endif

#endif /* RT_MI355X_DEBUG_H */
