// rt_host.h — error plumbing and device selection shared by the host runtime files, and the narrow
// interface of rt_multi.cpp to a context (the context itself: rt_context.h). Not part of the public C-ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/rt_mi355x.h"

namespace rt {

// A host-built scene (tree, grid, records; rt_api.cpp), built once and uploadable to any context:
// rt_multi_set_scene builds it for the first device and uploads the same package to the others.
struct HostPackage;
struct HostPackageDeleter { void operator()(HostPackage* p) const; };
using HostPackagePtr = std::unique_ptr<HostPackage, HostPackageDeleter>;

// rt_set_scene in two halves, so that rt_multi_set_scene issues every device's build before it
// waits for any: begin builds a host scene (or takes *shared) and uploads it, or starts a device
// build on the context's build stream; end waits for the device build's summary and builds its
// grid. Every begin that succeeds must be followed by end on the same context.
int set_scene_begin(rt_context* ctx, const Sphere* spheres, uint32_t count, void* stream, HostPackagePtr* shared);
int set_scene_end(rt_context* ctx);

// Trace launches recorded on ctx so far, and the trace-kernel duration of launch `index` (0 = the
// context's first; only the last 64 are kept), waiting for that launch's end event only.
uint64_t launch_count(const rt_context* ctx);
int launch_ms_at(rt_context* ctx, uint64_t index, float* ms);
// Per band row of launch `index` (one of the last 4), its share of the launch's work as the
// tile-cost record estimates it (rt_launch_row_weights); waits for that launch's copy only.
// Launches keep the record copies only once asked for (keep_row_weights, or the first call).
int launch_row_weights(rt_context* ctx, uint64_t index, std::vector<double>& w);
void keep_row_weights(rt_context* ctx);

// The pass loop of an adaptive frame (rt_render_adaptive_device) as resumable
// steps on a context, so that one host thread interleaves the passes of several contexts
// (rt_multi_render_adaptive); rt_render_adaptive_device itself is a loop over them, beside their
// definitions in rt_adaptive_frame.cpp. (Here and not in rt_internal.h: that header is compiled
// into the trace kernels' object.)
//   adaptive_check  the argument checks alone, no device work: rt_render_adaptive_device's rules,
//                   `who` names the caller in messages. *empty: a band without texels.
//   adaptive_check_values  the part of them that needs no context (options, adaptive, the cap).
//   adaptive_begin  the checks, the buffers and the state reset, ordered on `stream`. *open = false
//                   and RT_OK: nothing to render. accum / out: the band buffers finish will write.
//   adaptive_active the frame is open and tiles are left for another pass.
//   adaptive_issue_pass  two trace launches, the error kernel, the readback of the next list's
//                   length and its event. No host wait.
//   adaptive_pass_done   has that readback landed? block = false: hipEventQuery (*done = false
//                   when not yet); block = true waits. Consumes it once landed: the next pass's list.
//   adaptive_finish the resolve into accum / out / sample_count (band layout; sample_count optional),
//                   fills info (optional) and closes the frame. halves (optional, checked by the
//                   caller): the same resolve also writes the two halves and the half counts.
//   adaptive_abort  after a failed step: clears the half-buffers (A and B are zero between calls,
//                   whatever happened) and closes the frame; returns rc (or the closing's own error).
//   adaptive_tile_counts  DEVICE pointer of the band's per-tile sample counts (ceil(W / 8) x
//                   ceil(rows / 8) words, row-major), written by the frame's passes on its stream;
//                   valid until the context's next adaptive call.
int adaptive_check_values(const RenderCallInfo* rci, const rt_options& o, const rt_adaptive* ad, const char* who);
int adaptive_check(const rt_context* ctx, const RenderCallInfo* rci, uint32_t band_width, uint32_t band_height,
                   const float* accum, const uint8_t* out, const rt_options* opt, const rt_adaptive* ad,
                   const char* who, rt_options* o_out, bool* empty);
int adaptive_begin(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows, uint32_t band_width,
                   uint32_t band_height, float* accum, uint8_t* out, const rt_options* opt, const rt_adaptive* ad,
                   void* stream, const char* who, bool* open);
bool adaptive_active(const rt_context* ctx);
int adaptive_issue_pass(rt_context* ctx);
int adaptive_pass_done(rt_context* ctx, bool block, bool* done);
int adaptive_finish(rt_context* ctx, float* accum, uint8_t* out, uint32_t* sample_count, rt_adaptive_info* info,
                    const rt_half_outputs* halves = nullptr);
// The host-only refusals of a halves frame (rt_half_outputs_check): a NULL struct or accumulator, a
// non-NULL reserved, accum_a == accum_b, either equal to `accum`.
int half_outputs_check(const rt_half_outputs* halves, const float* accum);
int adaptive_abort(rt_context* ctx, int rc);
const uint32_t* adaptive_tile_counts(const rt_context* ctx);
// The fused store of a multi-device adaptive frame on `device` (rt_adaptive.hip
// rt_adaptive_store_tiles_kernel): band rows of `src` with the part's count table into rows[i] of
// the image's accumulator, rgba8 and optional count map.
int adaptive_store_tiles(int device, const float* src, uint32_t n_rows, uint32_t width, const uint32_t* tile_n,
                         const uint32_t* rows, uint32_t dst_rows, float* accum, uint8_t* out, uint32_t* sample_count,
                         void* stream);

// Message of the calling thread's last failure (rt_last_error()).
extern thread_local std::string g_last_error;
int fail(int code, const std::string& msg);
// A failed HIP call of `who`: RT_ERR_OUT_OF_MEMORY or RT_ERR_DEVICE, message "who: <HIP's error string>".
int fail_hip(hipError_t e, const std::string& who);
// RT_ERR_INVALID_ARGUMENT for a scene whose sphere `index` has a NaN / inf centre or radius
// (the geometry contract; rt_grid.h first_nonfinite_geometry).
int refuse_nonfinite(uint32_t index);
int current_device_count(int* n);

// RAII device selection: restores the caller's current device.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

}  // namespace rt

#define RT_HIP(call)                                            \
    do {                                                        \
        hipError_t e_ = (call);                                 \
        if (e_ != hipSuccess) return ::rt::fail_hip(e_, #call); \
    } while (0)
