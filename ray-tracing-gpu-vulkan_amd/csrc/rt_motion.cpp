// rt_motion.cpp — the motion pass (include/rt_mi355x.h): rt_motion_create and its
// kin, and rt_render_motion_device. The pass is three launches on the caller's stream: the rays
// through the band's texel centres (rt_motion_kernels.hip), their closest hits by the production walks, planned
// and launched as the closest-hit probe is (rt_probe.cpp: a one-sample STREAM frame of the band through
// fill_trace, split_units and launch_units, TraceParams::probe_rays picking the kernels' MODE_PROBE
// instantiation) but on the object's device planes and at the band's own width and offset, and the
// motion plane from the answers (rt_motion_kernels.hip). The checks, the camera and the kernel's constants are
// the HIP-free host half's (rt_motion_host.cpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>

#include "rt_context.h"
#include "rt_motion.h"
#include "rt_motion_host.h"

using rt::fail;

extern "C" int rt_motion_check(uint32_t band_width, uint32_t band_height, const RenderCallInfo* rci,
                               const RenderCallInfo* prev_rci) {
    const char* err = "";
    if (int rc = rt::motion::check(band_width, band_height, rci, prev_rci, &err)) return fail(rc, err);
    return RT_OK;
}

extern "C" int rt_motion_create(rt_context* ctx, uint32_t band_width, uint32_t band_height, rt_motion** out) {
    if (!ctx || !out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_motion_create: ctx or out is NULL");
    *out = nullptr;
    const char* err = "";
    if (int rc = rt::motion::check_band(band_width, band_height, &err)) return fail(rc, err);
    rt::DeviceGuard g(ctx->device);
    rt_motion* m = new (std::nothrow) rt_motion;
    if (!m) return fail(RT_ERR_OUT_OF_MEMORY, "rt_motion_create: out of host memory");
    m->ctx = ctx;
    m->band_w = band_width;
    m->band_h = band_height;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->rays), size_t(rt::motion::ray_bytes(band_width, band_height)));
    if (e == hipSuccess)
        e = hipMalloc(reinterpret_cast<void**>(&m->hits), size_t(rt::motion::hit_bytes(band_width, band_height)));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&m->stage_ev, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipFree(m->rays);
        (void)hipFree(m->hits);
        delete m;
        return rt::fail_hip(e, "rt_motion_create");
    }
    *out = m;
    return RT_OK;
}

extern "C" int rt_motion_destroy(rt_motion* motion) {
    if (!motion) return RT_OK;
    rt::DeviceGuard g(motion->ctx->device);
    (void)hipFree(motion->rays);   // waits for the queued calls that still use the planes
    (void)hipFree(motion->hits);
    (void)hipFree(motion->prev_geom);
    if (motion->stage) (void)hipHostFree(motion->stage);
    if (motion->stage_ev) (void)hipEventDestroy(motion->stage_ev);
    delete motion;
    return RT_OK;
}

namespace {

// Room for n previous centres on the device; queued work may still read the old buffer.
int reserve_prev(rt_context* ctx, rt_motion* m, uint32_t n, hipStream_t st) {
    if (m->prev_cap >= n) return RT_OK;
    if (m->prev_geom) ctx->host_waits++;
    return rt::grow_on_stream(m->prev_geom, m->prev_cap, uint64_t(n), 4u * sizeof(float), false, st);
}

}  // namespace

extern "C" int rt_motion_set_previous(rt_motion* motion, const Sphere* spheres, uint32_t count,
                                      const RenderCallInfo* prev_rci, void* stream) {
    if (!motion) return fail(RT_ERR_INVALID_ARGUMENT, "rt_motion_set_previous: motion is NULL");
    if (!prev_rci) return fail(RT_ERR_INVALID_ARGUMENT, "rt_motion_set_previous: prev_rci is NULL");
    if (count && !spheres) return fail(RT_ERR_INVALID_ARGUMENT, "rt_motion_set_previous: spheres is NULL");
    rt_context* ctx = motion->ctx;
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = rt::order_on(ctx, st)) return rc;
    if (count) {
        if (motion->stage_used) RT_HIP(hipEventSynchronize(motion->stage_ev));   // the last copy out of the staging
        if (motion->stage_cap < count) {
            if (motion->stage) RT_HIP(hipHostFree(motion->stage));
            motion->stage = nullptr;
            motion->stage_cap = 0;
            RT_HIP(hipHostMalloc(reinterpret_cast<void**>(&motion->stage), size_t(count) * 4u * sizeof(float), 0));
            motion->stage_cap = count;
        }
        for (uint32_t i = 0; i < count; i++) std::memcpy(motion->stage + 4u * size_t(i), &spheres[i].geometry, 4u * sizeof(float));
        if (int rc = reserve_prev(ctx, motion, count, st)) return rc;
        RT_HIP(hipMemcpyAsync(motion->prev_geom, motion->stage, size_t(count) * 4u * sizeof(float), hipMemcpyHostToDevice, st));
        RT_HIP(hipEventRecord(motion->stage_ev, st));
        motion->stage_used = true;
    }
    motion->prev_n = count;
    motion->prev_rci = *prev_rci;
    motion->has_prev = true;
    return rt::mark_issued(ctx, st);
}

extern "C" int rt_motion_keep_current(rt_context* ctx, rt_motion* motion, const RenderCallInfo* rci, void* stream) {
    if (!ctx || !motion || !rci) return fail(RT_ERR_INVALID_ARGUMENT, "rt_motion_keep_current: ctx, motion or rci is NULL");
    if (motion->ctx != ctx) return fail(RT_ERR_INVALID_ARGUMENT, "rt_motion_keep_current: motion belongs to another context");
    if (ctx->pending) return fail(RT_ERR_INVALID_ARGUMENT, "rt_motion_keep_current between the halves of a scene build");
    if (!ctx->scene_set) return fail(RT_ERR_NO_SCENE, "rt_motion_keep_current before rt_set_scene");
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = rt::order_on(ctx, st)) return rc;   // behind the scene's upload or device build
    const uint32_t n = ctx->scene.n_spheres;
    if (n) {
        if (int rc = reserve_prev(ctx, motion, n, st)) return rc;
        RT_HIP(hipMemcpyAsync(motion->prev_geom, ctx->scene.geom, size_t(n) * 4u * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    motion->prev_n = n;
    motion->prev_rci = *rci;
    motion->has_prev = true;
    return rt::render_issued(ctx, st);   // the copy reads the scene's arena
}

extern "C" int rt_render_motion_device(rt_context* ctx, rt_motion* motion, const RenderCallInfo* rci, float* motion_out,
                                       const rt_options* opt, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_motion_device: ctx is NULL");
    if (!motion) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_motion_device: motion is NULL");
    if (motion->ctx != ctx) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_motion_device: motion belongs to another context");
    const uint32_t band_w = motion->band_w, band_h = motion->band_h;
    const char* err = "";
    if (int rc = rt::motion::check(band_w, band_h, rci, motion->has_prev ? &motion->prev_rci : nullptr, &err))
        return fail(rc, err);
    if (!motion_out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_motion_device: motion_out is NULL");
    // the walk as a frame's options select it; never the instrumented kernels
    rt_options plan_opt;
    std::memset(&plan_opt, 0, sizeof(plan_opt));
    if (opt) {
        plan_opt.accel = opt->accel;
        plan_opt.reserved[0] = opt->reserved[0] & 2u;
        plan_opt.reserved[1] = opt->reserved[1];
    }
    RenderCallInfo frame = *rci;
    frame.samplesPerRenderCall = 1u;
    rt_options o;
    bool empty = false;
    if (int rc = rt::check_render_args(ctx, &frame, band_w, band_h, motion_out, reinterpret_cast<const uint8_t*>(motion_out),
                                       &plan_opt, "rt_render_motion_device", o, &empty))
        return rc;
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = rt::order_on(ctx, st)) return rc;

    // the rays through the texel centres
    rt::motion::Camera cam;
    rt::motion::camera(*rci, &cam);
    rt::MotionRayParams RK;
    std::memset(&RK, 0, sizeof(RK));
    RK.band_w = band_w;
    RK.band_h = band_h;
    RK.off_x = rci->offset.x;
    RK.off_y = rci->offset.y;
    std::memcpy(RK.lf, cam.lf, sizeof(RK.lf));
    std::memcpy(RK.hor, cam.hor, sizeof(RK.hor));
    std::memcpy(RK.ver, cam.ver, sizeof(RK.ver));
    std::memcpy(RK.ulc, cam.ulc, sizeof(RK.ulc));
    RK.inv_size_x = cam.inv_size_x;
    RK.inv_size_y = cam.inv_size_y;
    RK.rays = motion->rays;

    // their closest hits
    TraceSetup S;
    if (int rc = rt::fill_trace(ctx, &frame, nullptr, band_w, band_h, o, nullptr, nullptr, st, S)) return rc;
    rt::TraceParams& P = S.P;
    // the rays start at the camera the frame's plan was made for
    if (std::memcmp(P.lf, cam.lf, sizeof(cam.lf)) || std::memcmp(P.hor, cam.hor, sizeof(cam.hor)) ||
        std::memcmp(P.ver, cam.ver, sizeof(cam.ver)) || std::memcmp(P.ulc, cam.ulc, sizeof(cam.ulc)))
        return fail(RT_ERR_DEVICE, "rt_render_motion_device: the motion pass's camera is not the frame's");
    RT_HIP(rt::launch_motion_rays(RK, st));
    // no tile order and no cost record: the context's LPT schedule belongs to the frames
    if (int rc = rt::launch::split_units(S.in, S.plan, 1u, uint64_t(band_w) * band_h, S.n_tiles, false, true, &err))
        return fail(rc, err);
    P.chunks = S.plan.chunks;
    P.head_tiles = S.plan.head_tiles;
    P.head_chunks = S.plan.head_chunks;
    P.n_units = S.plan.n_units;
    P.probe_rays = motion->rays;
    P.probe_out = motion->hits;
    if (int rc = rt::launch_units(ctx, S, st)) return rc;

    // the motion plane
    const RenderCallInfo& prev_rci = motion->has_prev ? motion->prev_rci : *rci;
    rt::motion::Camera prev_cam;
    rt::motion::camera(prev_rci, &prev_cam);
    rt::motion::Projection pr;
    rt::motion::projection(prev_cam, &pr);
    const uint32_t n = ctx->scene.n_spheres;
    rt::MotionParams K;
    std::memset(&K, 0, sizeof(K));
    K.band_w = band_w;
    K.band_h = band_h;
    K.n_spheres = n;
    K.same_count = (!motion->has_prev || motion->prev_n == n) && n != 0u ? 1u : 0u;
    K.size_x = cam.size_x;
    K.size_y = cam.size_y;
    K.off_x = float(rci->offset.x);
    K.off_y = float(rci->offset.y);
    std::memcpy(K.lf, pr.lf, sizeof(K.lf));
    std::memcpy(K.hor, pr.hor, sizeof(K.hor));
    std::memcpy(K.ver, pr.ver, sizeof(K.ver));
    std::memcpy(K.u, pr.u, sizeof(K.u));
    std::memcpy(K.wn, pr.wn, sizeof(K.wn));
    K.k = pr.k;
    K.ihh = pr.ihh;
    K.ivv = pr.ivv;
    K.rays = motion->rays;
    K.hits = motion->hits;
    K.geom_now = reinterpret_cast<const float4*>(ctx->scene.geom);
    K.geom_prev = motion->has_prev ? reinterpret_cast<const float4*>(motion->prev_geom) : K.geom_now;
    K.motion = motion_out;
    RT_HIP(rt::launch_motion(K, st));
    return rt::render_issued(ctx, st);
}
