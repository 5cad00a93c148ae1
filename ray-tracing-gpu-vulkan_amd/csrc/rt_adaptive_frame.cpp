// rt_adaptive_frame.cpp — adaptive frames (rt_render_adaptive_device): the pass
// loop as steps on a context (rt_host.h; rt_multi.cpp interleaves them over several contexts) and
// the adaptive planes, which sample-map frames sum into as well (rt_sample_map_frame.cpp). The
// launches themselves are rt_api.cpp's (rt_context.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/rt_mi355x_debug.h"
#include "rt_context.h"
#include "rt_launchers.h"

namespace rt {

// The recovery of a frame on the adaptive planes that failed with `rc` after its first launch: the
// planes are zero between calls, whatever happened. Keeps the first error and its message.
int abort_on_planes(rt_context* ctx, hipStream_t st, int rc) {
    rt_context::Adaptive& a = ctx->adaptive;
    const std::string msg = rt::g_last_error;
    (void)hipMemsetAsync(a.planes, 0, a.cap * 6u * sizeof(unsigned long long), st);
    rt::g_last_error = msg;
    if (int rc2 = render_issued(ctx, st)) return rc ? rc : rc2;
    return rc;
}

// Buffers of an adaptive frame of `texels` texels in `n_tiles` tiles.
int adaptive_reserve(rt_context* ctx, uint64_t texels, uint64_t n_tiles, hipStream_t st) {
    rt_context::Adaptive& a = ctx->adaptive;
    if (a.cap < texels) {
        if (a.planes) ctx->host_waits++;
        if (int rc = grow_on_stream(a.planes, a.cap, texels, 6u * sizeof(unsigned long long), true, st)) return rc;
    }
    if (a.cap_tiles < n_tiles) {
        a.last_w = a.last_h = 0;   // the last frame's count table goes with the old buffer
        if (int rc = grow_on_stream(a.tiles, a.cap_tiles, n_tiles, 4u * sizeof(uint32_t), false, st)) return rc;
    }
    if (!a.state) RT_HIP(hipMalloc(reinterpret_cast<void**>(&a.state), sizeof(rt::AdaptiveState)));
    if (!a.host) RT_HIP(hipHostMalloc(reinterpret_cast<void**>(&a.host), sizeof(rt::AdaptiveState), hipHostMallocDefault));
    if (!a.ev) RT_HIP(hipEventCreateWithFlags(&a.ev, hipEventDisableTiming));
    return RT_OK;
}

namespace {
// The half-buffers and tile tables of the frame in flight.
struct AdaptiveBuffers {
    uint64_t texels, n_tiles;
    unsigned long long* half[2];
    uint32_t* tile_n;
    uint32_t* lists[2];
};
AdaptiveBuffers adaptive_buffers(rt_context* ctx) {
    rt_context::Adaptive& a = ctx->adaptive;
    const rt::TraceParams& P = a.frame.S.P;
    AdaptiveBuffers b;
    b.texels = uint64_t(P.band_w) * P.band_h;
    b.n_tiles = a.frame.S.n_tiles;
    b.half[0] = a.planes;
    b.half[1] = a.planes + 3u * b.texels;
    b.tile_n = a.tiles;
    b.lists[0] = a.tiles + b.n_tiles;
    b.lists[1] = a.tiles + 2u * b.n_tiles;
    return b;
}
}  // namespace

// The adaptive pass loop as steps on a context (rt_host.h).
int adaptive_check_values(const RenderCallInfo* rci, const rt_options& o, const rt_adaptive* ad, const char* who) {
    if (!ad) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive is NULL");
    const uint32_t max_spp = rci->samplesPerRenderCall;
    if (o.rng_mode != RT_RNG_SAMPLE_HASH)
        return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + " needs rng_mode RT_RNG_SAMPLE_HASH");
    if (o.accumulate) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": accumulate must be 0");
    if (ad->min_spp == 0 || (ad->min_spp & 1u)) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive min_spp must be even and >= 2");
    if (ad->step_spp == 0 || (ad->step_spp & 1u))
        return fail(RT_ERR_INVALID_ARGUMENT, "adaptive step_spp must be even and >= 2");
    if (max_spp == 0 || (max_spp & 1u))
        return fail(RT_ERR_INVALID_ARGUMENT, "adaptive max_spp (samplesPerRenderCall) must be even and >= 2");
    if (ad->min_spp > max_spp) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive min_spp exceeds max_spp (samplesPerRenderCall)");
    if (uint64_t(o.sample_base) + max_spp > 0xffffffffull)
        return fail(RT_ERR_INVALID_ARGUMENT, "sample_base + max_spp overflows 32 bits");
    if (!(std::isfinite(ad->threshold) && ad->threshold >= 0.0f && ad->threshold <= 16.0f))
        return fail(RT_ERR_INVALID_ARGUMENT, "adaptive threshold must be finite and within [0, 16]");
    if (ad->reserved != 0) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive reserved must be 0");
    return RT_OK;
}

int adaptive_check(const rt_context* ctx, const RenderCallInfo* rci, uint32_t band_width, uint32_t band_height,
                   const float* accum, const uint8_t* out, const rt_options* opt, const rt_adaptive* ad,
                   const char* who, rt_options* o_out, bool* empty) {
    rt_options o;
    if (int rc = check_render_args(ctx, rci, band_width, band_height, accum, out, opt, who, o, empty)) return rc;
    if (*empty) return RT_OK;
    if (int rc = adaptive_check_values(rci, o, ad, who)) return rc;
    if (o_out) *o_out = o;
    return RT_OK;
}

int adaptive_abort(rt_context* ctx, int rc) {
    rt_context::Adaptive& a = ctx->adaptive;
    if (!a.frame.open) return rc;
    DeviceGuard g(ctx->device);
    a.frame.open = a.frame.pending = false;
    return abort_on_planes(ctx, a.frame.st, rc);
}

int adaptive_begin(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows, uint32_t band_width,
                   uint32_t band_height, float* accum, uint8_t* out, const rt_options* opt, const rt_adaptive* ad,
                   void* stream, const char* who, bool* open) {
    *open = false;
    rt_options o;
    bool empty = false;
    if (int rc = adaptive_check(ctx, rci, band_width, band_height, accum, out, opt, ad, who, &o, &empty)) return rc;
    if (empty) return RT_OK;
    rt_context::Adaptive& a = ctx->adaptive;
    rt_context::Adaptive::Frame& f = a.frame;
    if (f.open) return fail(RT_ERR_INVALID_ARGUMENT, std::string(who) + ": an adaptive frame is in flight on this context");
    DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = order_on(ctx, st)) return rc;
    if (int rc = fill_trace(ctx, rci, rows, band_width, band_height, o, accum, out, st, f.S)) return rc;
    if (int rc = adaptive_reserve(ctx, uint64_t(band_width) * band_height, f.S.n_tiles, st)) return rc;
    rt::TraceParams& P = f.S.P;
    // the walk kernels record tile costs unconditionally (rt_trace_units.h record_tile_cost): a
    // scratch table of the whole tile grid, never read
    P.tile_cost = f.S.plan.accel != rt::ACCEL_BRUTE ? a.tiles + 3u * f.S.n_tiles : nullptr;
    P.accumulate = 0u;
    P.head_tiles = 0u;
    f.o = o;
    f.ad = *ad;
    f.st = st;
    f.max_spp = rci->samplesPerRenderCall;
    f.done = f.passes = f.cur = 0;
    f.active = f.S.n_tiles;
    f.list = nullptr;   // pass 0: every tile, row-major
    f.pending = false;
    f.open = true;      // from here on a failure leaves sums or state behind: adaptive_abort clears them
    a.last_w = a.last_h = 0;   // the passes overwrite the last frame's count table
    if (hipError_t e = rt::launch_adaptive_init(a.state, st); e != hipSuccess)
        return adaptive_abort(ctx, fail(RT_ERR_DEVICE, std::string("launch_adaptive_init: ") + hipGetErrorString(e)));
    *open = true;
    return RT_OK;
}

bool adaptive_active(const rt_context* ctx) { return ctx->adaptive.frame.open && ctx->adaptive.frame.active != 0; }

int adaptive_issue_pass(rt_context* ctx) {
    rt_context::Adaptive& a = ctx->adaptive;
    rt_context::Adaptive::Frame& f = a.frame;
    if (!f.open || f.pending || !f.active) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive pass out of order");
    DeviceGuard g(ctx->device);
    const AdaptiveBuffers b = adaptive_buffers(ctx);
    TraceSetup& S = f.S;
    rt::TraceParams& P = S.P;
    hipStream_t st = f.st;
    const uint32_t k = f.passes == 0 ? f.ad.min_spp : std::min(f.ad.step_spp, f.max_spp - f.done);
    for (uint32_t h = 0; h < 2; h++) {   // samples [done, done + k/2) into A, the next k/2 into B
        P.fixed = b.half[h];
        P.tile_order = f.list;
        if (int rc = launch_tile_prefix(ctx, S, k / 2u, f.o.sample_base + f.done + h * (k / 2u), f.active,
                                        f.list != nullptr, st))
            return rc;
    }
    f.done += k;
    rt::AdaptiveErrorParams K;
    std::memset(&K, 0, sizeof(K));
    K.a = b.half[0];
    K.b = b.half[1];
    K.texels = b.texels;
    K.band_w = P.band_w;
    K.band_h = P.band_h;
    K.tiles_x = P.tiles_x;
    K.list = f.list;
    K.n_list = uint32_t(f.active);
    K.n_done = f.done;
    K.max_spp = f.max_spp;
    K.thr_q16 = rt::adaptive_thr_q16(f.ad.threshold);
    K.cur = f.cur;
    K.tile_n = b.tile_n;
    K.next_list = b.lists[f.cur ^ 1u];
    K.state = a.state;
    RT_HIP(rt::launch_adaptive_error(K, st));
    // the one readback of the pass: the next list's length (and the running totals)
    RT_HIP(hipMemcpyAsync(a.host, a.state, sizeof(rt::AdaptiveState), hipMemcpyDeviceToHost, st));
    RT_HIP(hipEventRecord(a.ev, st));
    f.pending = true;
    return RT_OK;
}

int adaptive_pass_done(rt_context* ctx, bool block, bool* done) {
    rt_context::Adaptive& a = ctx->adaptive;
    rt_context::Adaptive::Frame& f = a.frame;
    if (done) *done = false;
    if (!f.open || !f.pending) return fail(RT_ERR_INVALID_ARGUMENT, "no adaptive pass in flight");
    DeviceGuard g(ctx->device);
    if (block) {
        RT_HIP(hipEventSynchronize(a.ev));
    } else {
        const hipError_t e = hipEventQuery(a.ev);
        if (e == hipErrorNotReady) {
            (void)hipGetLastError();   // not an error: nothing for a later launch check to pick up
            return RT_OK;
        }
        RT_HIP(e);
    }
    const AdaptiveBuffers b = adaptive_buffers(ctx);
    f.pending = false;
    f.passes++;
    f.cur ^= 1u;
    f.active = a.host->count[f.cur];
    f.list = b.lists[f.cur];
    if (f.active > b.n_tiles) return fail(RT_ERR_DEVICE, "adaptive tile list longer than the tile grid");
    if (done) *done = true;
    return RT_OK;
}

int half_outputs_check(const rt_half_outputs* halves, const float* accum) {
    if (!halves) return fail(RT_ERR_INVALID_ARGUMENT, "rt_half_outputs: halves is NULL");
    if (!halves->accum_a) return fail(RT_ERR_INVALID_ARGUMENT, "rt_half_outputs: accum_a is NULL");
    if (!halves->accum_b) return fail(RT_ERR_INVALID_ARGUMENT, "rt_half_outputs: accum_b is NULL");
    if (halves->reserved) return fail(RT_ERR_INVALID_ARGUMENT, "rt_half_outputs: reserved must be NULL");
    if (halves->accum_a == halves->accum_b)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_half_outputs: accum_a and accum_b are the same array");
    if (halves->accum_a == accum) return fail(RT_ERR_INVALID_ARGUMENT, "rt_half_outputs: accum_a is accum_rgba32f");
    if (halves->accum_b == accum) return fail(RT_ERR_INVALID_ARGUMENT, "rt_half_outputs: accum_b is accum_rgba32f");
    return RT_OK;
}

int adaptive_finish(rt_context* ctx, float* accum, uint8_t* out, uint32_t* sample_count, rt_adaptive_info* info,
                    const rt_half_outputs* halves) {
    rt_context::Adaptive& a = ctx->adaptive;
    rt_context::Adaptive::Frame& f = a.frame;
    if (!f.open || f.pending || f.active) return fail(RT_ERR_INVALID_ARGUMENT, "adaptive finish out of order");
    DeviceGuard g(ctx->device);
    const AdaptiveBuffers b = adaptive_buffers(ctx);
    const rt::TraceParams& P = f.S.P;
    if (hipError_t e = rt::launch_adaptive_resolve(b.half[0], b.half[1], b.texels, P.band_w, P.tiles_x, b.tile_n, accum,
                                                   out, sample_count, halves ? halves->accum_a : nullptr,
                                                   halves ? halves->accum_b : nullptr,
                                                   halves ? halves->half_count : nullptr, f.st);
        e != hipSuccess)
        return adaptive_abort(ctx, fail(RT_ERR_DEVICE, std::string("launch_adaptive_resolve: ") + hipGetErrorString(e)));
    if (info) {
        info->passes = f.passes;
        info->tiles = uint32_t(b.n_tiles);
        info->tiles_capped = a.host->capped;
        info->reserved = 0;
        info->samples = a.host->samples;
    }
    f.open = false;
    a.last_w = P.band_w;
    a.last_h = P.band_h;
    return render_issued(ctx, f.st);
}

const uint32_t* adaptive_tile_counts(const rt_context* ctx) { return ctx->adaptive.tiles; }

int adaptive_store_tiles(int device, const float* src, uint32_t n_rows, uint32_t width, const uint32_t* tile_n,
                         const uint32_t* rows, uint32_t dst_rows, float* accum, uint8_t* out, uint32_t* sample_count,
                         void* stream) {
    if (n_rows == 0 || width == 0) return RT_OK;
    if (!src || !tile_n || !rows || !accum || !out) return fail(RT_ERR_INVALID_ARGUMENT, "NULL argument");
    DeviceGuard g(device);
    RT_HIP(rt::launch_adaptive_store_tiles(src, n_rows, width, tile_n, rows, dst_rows, accum, out, sample_count,
                                           static_cast<hipStream_t>(stream)));
    return RT_OK;
}

}  // namespace rt

using rt::fail;

namespace {

// rt_render_adaptive_device (halves null) and rt_render_adaptive_halves_device (halves checked).
int render_adaptive(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows, uint32_t band_width,
                    uint32_t band_height, float* accum, uint8_t* out, uint32_t* sample_count, const rt_options* opt,
                    const rt_adaptive* ad, rt_adaptive_info* info, const rt_half_outputs* halves, void* stream,
                    const char* who) {
    // the state machine of rt_host.h, one context: each pass waits for its own readback
    bool open = false;
    if (int rc = rt::adaptive_begin(ctx, rci, rows, band_width, band_height, accum, out, opt, ad, stream, who, &open))
        return rc;
    if (!open) return RT_OK;   // a band without texels
    int rc = RT_OK;
    while (rc == RT_OK && rt::adaptive_active(ctx)) {
        rc = rt::adaptive_issue_pass(ctx);
        if (rc == RT_OK) rc = rt::adaptive_pass_done(ctx, true, nullptr);
    }
    if (rc != RT_OK) return rt::adaptive_abort(ctx, rc);
    return rt::adaptive_finish(ctx, accum, out, sample_count, info, halves);
}

}  // namespace

extern "C" {

int rt_render_adaptive_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows,
                              uint32_t band_width, uint32_t band_height, float* accum, uint8_t* out,
                              uint32_t* sample_count, const rt_options* opt, const rt_adaptive* ad,
                              rt_adaptive_info* info, void* stream) {
    if (info) std::memset(info, 0, sizeof(*info));
    return render_adaptive(ctx, rci, rows, band_width, band_height, accum, out, sample_count, opt, ad, info, nullptr,
                           stream, "rt_render_adaptive_device");
}

int rt_half_outputs_check(const rt_half_outputs* halves, const float* accum) {
    return rt::half_outputs_check(halves, accum);
}

int rt_render_adaptive_halves_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows,
                                     uint32_t band_width, uint32_t band_height, float* accum, uint8_t* out,
                                     uint32_t* sample_count, const rt_options* opt, const rt_adaptive* ad,
                                     rt_adaptive_info* info, const rt_half_outputs* halves, void* stream) {
    if (info) std::memset(info, 0, sizeof(*info));
    if (int rc = rt::half_outputs_check(halves, accum)) return rc;
    return render_adaptive(ctx, rci, rows, band_width, band_height, accum, out, sample_count, opt, ad, info, halves,
                           stream, "rt_render_adaptive_halves_device");
}

int rt_debug_adaptive_resolve(rt_context* ctx, uint32_t band_width, uint32_t band_height, uint32_t count, float* accum,
                              uint8_t* out, uint32_t* sample_count, const rt_half_outputs* halves, void* stream) {
    if (!ctx || !accum || !out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_adaptive_resolve: ctx, accum or out is NULL");
    if (band_width == 0 || band_height == 0 || band_width > 65535u || band_height > 65535u)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_adaptive_resolve: band width and height must be within 1 .. 65535");
    if (halves)
        if (int rc = rt::half_outputs_check(halves, accum)) return rc;
    rt_context::Adaptive& a = ctx->adaptive;
    if (a.frame.open) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_adaptive_resolve: an adaptive frame is open on this context");
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = rt::order_on(ctx, st)) return rc;
    const uint64_t texels = uint64_t(band_width) * band_height;
    const uint32_t tiles_x = (band_width + 7u) / 8u;
    const uint64_t n_tiles = uint64_t(tiles_x) * ((band_height + 7u) / 8u);
    if (int rc = rt::adaptive_reserve(ctx, texels, n_tiles, st)) return rc;
    a.last_w = a.last_h = 0;   // the count table below replaces the last frame's
    RT_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.tiles), int(count), n_tiles, st));
    RT_HIP(rt::launch_adaptive_resolve(a.planes, a.planes + 3u * texels, texels, band_width, tiles_x, a.tiles, accum, out,
                                       sample_count, halves ? halves->accum_a : nullptr,
                                       halves ? halves->accum_b : nullptr, halves ? halves->half_count : nullptr, st));
    return rt::mark_issued(ctx, st);
}

int rt_adaptive_tile_converged(uint64_t E, uint64_t S, uint32_t n, uint32_t m, uint32_t thr_q16, int* converged) {
    if (!converged) return fail(RT_ERR_INVALID_ARGUMENT, "converged is NULL");
    if (E >= rt::kAdaptiveMaxSum || S >= rt::kAdaptiveMaxSum)
        return fail(RT_ERR_INVALID_ARGUMENT, "E and S must be below 2^56");
    if (n > rt::kAdaptiveMaxSpp) return fail(RT_ERR_INVALID_ARGUMENT, "n above 2^19");
    if (m == 0 || m > 64u) return fail(RT_ERR_INVALID_ARGUMENT, "m must be within 1 .. 64");
    *converged = rt::adaptive_tile_converged(E, S, n, m, thr_q16) ? 1 : 0;
    return RT_OK;
}

}  // extern "C"
