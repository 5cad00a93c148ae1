// rt_probe.cpp — rt_debug_closest_hits (include/rt_mi355x_debug.h): the closest hit of a batch of
// given rays by the production walks. The batch is a band of kProbeBandW texels per row, one ray per
// texel, planned and launched as a one-sample STREAM frame of that band through rt_api.cpp's own
// steps (fill_trace, split_units, launch_units); TraceParams::probe_rays makes launch_trace pick the
// kernels' MODE_PROBE instantiation, which loads a unit's ray where a frame computes the camera's
// and stores (winner, t) where a frame shades (rt_trace_shade.h start_sample, shade_rec). The host half
// (argument checks of the rays, the batch as a band) is rt_probe_batch.cpp, without HIP.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt_mi355x_debug.h"
#include "rt_context.h"
#include "rt_launchers.h"
#include "rt_probe_batch.h"

using rt::fail;

extern "C" int rt_debug_closest_hits(rt_context* ctx, const float* rays6, uint32_t n, const rt_options* options,
                                     uint32_t* out_id, float* out_t) {
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (ctx->pending) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_closest_hits between the halves of a scene build");
    if (!ctx->scene_set) return fail(RT_ERR_NO_SCENE, "rt_debug_closest_hits before rt_set_scene");
    if (n == 0) return RT_OK;
    if (!rays6 || !out_id || !out_t) return fail(RT_ERR_INVALID_ARGUMENT, "rays6, out_id or out_t is NULL");
    if (n > rt::probe::kProbeMaxRays) return fail(RT_ERR_INVALID_ARGUMENT, "more than 2^24 rays");
    rt_options o;
    std::memset(&o, 0, sizeof(o));
    if (options) {
        o.accel = options->accel;
        o.reserved[0] = options->reserved[0] & 2u;   // force_regate; never the instrumented kernels
        o.reserved[1] = options->reserved[1];
    }
    if (o.accel > RT_ACCEL_LBVH) return fail(RT_ERR_INVALID_ARGUMENT, "unknown accel");
    std::vector<float> rays;
    uint32_t band_h = 0;
    float cam_r = 0.0f;
    if (const uint32_t bad = rt::probe::stage_batch(rays6, n, rays, &band_h, &cam_r))
        return fail(RT_ERR_INVALID_ARGUMENT, "ray " + std::to_string(bad - 1u) +
                                                 ": not finite, or a direction without a nonzero component");
    const uint32_t band_w = rt::probe::kProbeBandW;
    const uint64_t texels = uint64_t(band_w) * band_h;

    // a one-sample frame of the band; its camera is never traced (the plan gets the batch's distance
    // and the pinhole fact directly, fill_trace_at), the reference's only keeps the launch's fields finite
    RenderCallInfo rci;
    if (int rc = rt_canonical_render_call_info(1u, band_w, band_h, &rci)) return rc;

    rt::DeviceGuard g(ctx->device);
    hipStream_t st = nullptr;
    if (int rc = rt::order_on(ctx, st)) return rc;
    // the batch and its answers on the device, for this call only
    struct Buffers {
        float* rays = nullptr;
        uint32_t* out = nullptr;
        ~Buffers() {
            (void)hipFree(rays);
            (void)hipFree(out);
        }
    } buf;
    RT_HIP(hipMalloc(reinterpret_cast<void**>(&buf.rays), rays.size() * sizeof(float)));
    RT_HIP(hipMalloc(reinterpret_cast<void**>(&buf.out), size_t(texels) * 2u * sizeof(uint32_t)));
    RT_HIP(hipMemcpyAsync(buf.rays, rays.data(), rays.size() * sizeof(float), hipMemcpyHostToDevice, st));

    TraceSetup S;
    // pinhole_lf = 1: a probe has no camera origin to perturb, so the one-layer L2 grid kernel runs in
    // the form production frames run it in (flat_grid_form)
    if (int rc = rt::fill_trace_at(ctx, &rci, nullptr, band_w, band_h, o, nullptr, nullptr, st, cam_r, 1, S)) return rc;
    rt::TraceParams& P = S.P;
    // no tile order and no cost record: the context's LPT schedule belongs to the frames
    const char* err = "";
    if (int rc = rt::launch::split_units(S.in, S.plan, 1u, texels, S.n_tiles, false, true, &err)) return fail(rc, err);
    P.chunks = S.plan.chunks;
    P.head_tiles = S.plan.head_tiles;
    P.head_chunks = S.plan.head_chunks;
    P.n_units = S.plan.n_units;
    P.probe_rays = buf.rays;
    P.probe_out = buf.out;
    if (int rc = rt::launch_units(ctx, S, st)) return rc;
    if (int rc = rt::render_issued(ctx, st)) return rc;
    std::vector<uint32_t> out(size_t(texels) * 2u);
    RT_HIP(hipMemcpyAsync(out.data(), buf.out, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    for (uint32_t i = 0; i < n; i++) {
        out_id[i] = out[2u * size_t(i)];
        std::memcpy(&out_t[i], &out[2u * size_t(i) + 1u], sizeof(float));
    }
    return RT_OK;
}
