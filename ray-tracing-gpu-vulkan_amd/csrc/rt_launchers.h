// rt_launchers.h — the host-callable launchers of the device translation units, declared once: each
// .hip file that defines them includes this header (so a definition is checked against its
// declaration), and so does every host file that calls them. Declarations only: the parameter
// structs are named, not defined, here. rt_build.hip's launchers are in rt_build.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {
struct TraceParams; struct Counters; struct TabSize; struct ScatterProbeParams;   // rt_internal.h, rt_hand_out.h
struct AdaptiveState; struct AdaptiveErrorParams; struct FeedbackParams;   // rt_adaptive.h
namespace sample_map { struct DevicePlanParams; }                          // rt_sample_map_device.h

// rt_kernels.hip
hipError_t launch_trace(const TraceParams& P, uint32_t accel, bool count, int mode, int grid, size_t lds_bytes,
                        hipStream_t st);
hipError_t trace_occupancy(uint32_t accel, bool count, int mode, bool flat, size_t lds_bytes, int* blocks_per_cu);
bool flat_grid_form(const TraceParams& P, uint32_t accel, bool count);
hipError_t launch_trace_batch(const TraceParams& P, int grid, size_t lds_bytes, hipStream_t st);
hipError_t trace_batch_occupancy(size_t lds_bytes, int* blocks_per_cu, size_t* static_lds);
uint32_t block_size(uint32_t accel);
// rt_frame_kernels.hip
hipError_t launch_resolve_fixed(unsigned long long* fixed, uint64_t n_texels, uint32_t accumulate, uint32_t spp,
                                float* accum, uint8_t* out, hipStream_t st);
hipError_t launch_tonemap(const float* accum, uint64_t n_texels, uint32_t spp, uint8_t* out, hipStream_t st);
hipError_t launch_prep(const TraceParams& P, uint32_t work_head, float* tab, uint32_t n_cost, hipStream_t st);
hipError_t launch_tab_size(const uint32_t* n_blocks, uint64_t reserve, uint64_t grid_waves, TabSize* rec,
                           Counters* counters, hipStream_t st);
hipError_t launch_scatter_rows(const float* src_acc, const uint8_t* src_px, const uint32_t* rows,
                               uint32_t n_rows, uint32_t width, uint32_t dst_rows, float* dst_acc, uint8_t* dst_px,
                               hipStream_t st);
hipError_t launch_gather_rows(const float* src_acc, const uint32_t* rows, uint32_t n_rows, uint32_t width,
                              uint32_t src_rows, float* dst_acc, hipStream_t st);
// rt_debug_kernels.hip
hipError_t launch_debug_math(int op, const float* in, float* out, uint32_t n, hipStream_t st);
hipError_t launch_debug_exact(unsigned long long* bad, hipStream_t st);
hipError_t launch_debug_exact_normalize(unsigned long long* bad4, hipStream_t st);
hipError_t launch_scatter_probe(const ScatterProbeParams& K, bool rec, hipStream_t st);
// rt_adaptive.hip
hipError_t launch_adaptive_init(AdaptiveState* state, hipStream_t st);
hipError_t launch_adaptive_error(const AdaptiveErrorParams& K, hipStream_t st);
// (accum_a non-null: the resolve that also hands the two halves over; accum_b then too, half_count optional)
hipError_t launch_adaptive_resolve(unsigned long long* a, unsigned long long* b, uint64_t n_texels, uint32_t band_w,
                                   uint32_t tiles_x, const uint32_t* tile_n, float* accum, uint8_t* out,
                                   uint32_t* sample_count, float* accum_a, float* accum_b, uint32_t* half_count,
                                   hipStream_t st);
hipError_t launch_feedback_update(const FeedbackParams& K, hipStream_t st);
hipError_t launch_adaptive_store_tiles(const float* src, uint32_t n_rows, uint32_t width, const uint32_t* tile_n,
                                       const uint32_t* rows, uint32_t dst_rows, float* accum, uint8_t* out,
                                       uint32_t* sample_count, hipStream_t st);
// rt_sample_map_plan.hip
hipError_t device_plan_temp_bytes(uint32_t n_tiles, size_t* bytes);
hipError_t launch_device_plan(const sample_map::DevicePlanParams& K, hipStream_t st);
}  // namespace rt
