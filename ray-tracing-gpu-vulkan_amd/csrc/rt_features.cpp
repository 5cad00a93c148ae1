// rt_features.cpp — rt_render_features_device and rt_denoise_device (include/rt_mi355x.h, DESIGN.md
// §3.1.3). The feature pass is planned and launched as the one-chunk STREAM frame of its band with
// samplesPerRenderCall = feature_samples, through rt_api.cpp's own steps (fill_trace, split_units,
// launch_units), as the closest-hit probe is (rt_probe.cpp): one unit per pixel, so that one lane
// sums a pixel's samples in ascending order. TraceParams::feat0 makes launch_trace pick the kernels'
// MODE_FEATURES instantiation, which takes HASH's camera rays and ends each at its closest hit
// (rt_trace_shade.h shade_rec). The denoise is one kernel per iteration (rt_denoise.hip) by the launch
// list of its HIP-free host half (rt_denoise_host.cpp); the variance-guided denoise likewise
// (rt_denoise_var.hip, rt_denoise_var_host.cpp), on the same band planes of the context. The temporal
// stage in front of them is a state object of its own and one kernel per call (rt_temporal.hip: in
// place, or reprojected along the motion plane of rt_motion.cpp) by the checks of its host half
// (rt_temporal_host.cpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <string>

#include "../../include/rt_mi355x_debug.h"
#include "rt_context.h"
#include "rt_denoise.h"
#include "rt_denoise_host.h"
#include "rt_denoise_var.h"
#include "rt_denoise_var_host.h"
#include "rt_launchers.h"
#include "rt_temporal.h"
#include "rt_temporal_host.h"

using rt::fail;

extern "C" int rt_render_features_device(rt_context* ctx, const RenderCallInfo* rci, const uint32_t* rows,
                                         uint32_t band_width, uint32_t band_height, float* feat0, float* feat1,
                                         uint32_t feature_samples, const rt_options* opt, void* stream) {
    if (!ctx || !rci) return fail(RT_ERR_INVALID_ARGUMENT, "ctx or rci is NULL");
    if (!opt || opt->rng_mode != RT_RNG_SAMPLE_HASH)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_features_device: rng_mode must be RT_RNG_SAMPLE_HASH");
    if (opt->accumulate) return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_features_device: accumulate must be 0");
    if (feature_samples < 1u || feature_samples > RT_FEATURE_MAX_SAMPLES)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_features_device: feature_samples must be 1..256");
    if (opt->sample_base > 0xffffffffu - feature_samples)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_render_features_device: sample_base + feature_samples exceeds 32 bits");
    // the launch's plan is the STREAM frame's of feature_samples samples (one chunk per pixel); never
    // the instrumented kernels
    rt_options plan_opt = *opt;
    plan_opt.rng_mode = RT_RNG_PIXEL_STREAM;
    plan_opt.reserved[0] = opt->reserved[0] & 2u;
    RenderCallInfo frame = *rci;
    frame.samplesPerRenderCall = feature_samples;
    rt_options o;
    bool empty = false;
    if (band_width && band_height && (!feat0 || !feat1)) return fail(RT_ERR_INVALID_ARGUMENT, "feat0 or feat1 is NULL");
    if (int rc = rt::check_render_args(ctx, &frame, band_width, band_height, feat0, reinterpret_cast<const uint8_t*>(feat1),
                                       &plan_opt, "rt_render_features_device", o, &empty))
        return rc;
    if (empty) return RT_OK;
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = rt::order_on(ctx, st)) return rc;
    TraceSetup S;
    if (int rc = rt::fill_trace(ctx, &frame, rows, band_width, band_height, o, nullptr, nullptr, st, S)) return rc;
    rt::TraceParams& P = S.P;
    // no tile order and no cost record: the context's LPT schedule belongs to the frames
    const char* err = "";
    if (int rc = rt::launch::split_units(S.in, S.plan, feature_samples, uint64_t(band_width) * band_height, S.n_tiles,
                                         false, true, &err))
        return fail(rc, err);
    if (S.plan.chunks != 1u) return fail(RT_ERR_DEVICE, "rt_render_features_device: the plan split a pixel's samples");
    P.chunks = S.plan.chunks;
    P.head_tiles = S.plan.head_tiles;
    P.head_chunks = S.plan.head_chunks;
    P.n_units = S.plan.n_units;
    P.feat0 = feat0;
    P.feat1 = feat1;
    if (int rc = rt::launch_units(ctx, S, st)) return rc;
    return rt::render_issued(ctx, st);
}

extern "C" int rt_denoise_check(const rt_denoise* params, uint32_t band_width, uint32_t band_height,
                                uint32_t feature_samples) {
    rt_denoise p;
    const char* err = "";
    if (int rc = rt::denoise::check(params, band_width, band_height, feature_samples, &p, &err)) return fail(rc, err);
    return RT_OK;
}

extern "C" int rt_debug_denoise_lds_steps(rt_context* ctx, uint32_t max_step) {
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (max_step != 0u && max_step != 1u && max_step != 2u && max_step != 4u)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_denoise_lds_steps: 0, 1, 2 or 4");
    ctx->denoise.lds_max_step = max_step;
    return RT_OK;
}

extern "C" int rt_denoise_device(rt_context* ctx, const float* accum, const uint32_t* sample_count, uint32_t spp,
                                 const float* feat0, const float* feat1, uint32_t feature_samples, uint32_t band_width,
                                 uint32_t band_height, const rt_denoise* params, float* out_mean, uint8_t* out_rgba8,
                                 void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    rt_denoise p;
    const char* err = "";
    if (int rc = rt::denoise::check(params, band_width, band_height, feature_samples, &p, &err)) return fail(rc, err);
    if (band_width == 0 || band_height == 0) return RT_OK;
    if (!accum || !feat0 || !feat1 || !out_rgba8)
        return fail(RT_ERR_INVALID_ARGUMENT, "rt_denoise_device: accum, feat0, feat1 or out_rgba8 is NULL");
    const uint64_t texels = uint64_t(band_width) * band_height;
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = rt::order_on(ctx, st)) return rc;
    rt_context::Denoise& dn = ctx->denoise;
    if (p.iterations > 1u && dn.cap < texels) {
        if (dn.planes) ctx->host_waits++;   // queued denoises still read the old planes: the stream drains
        if (int rc = rt::grow_on_stream(dn.planes, dn.cap, texels, 3u * 4u * sizeof(float), false, st)) return rc;
    }
    float* plane[3] = {nullptr, nullptr, nullptr};   // BUF_PING, BUF_PONG, the guide
    if (dn.planes)
        for (int k = 0; k < 3; k++) plane[k] = dn.planes + size_t(k) * dn.cap * 4u;
    rt::denoise::Launch list[rt::denoise::kMaxIterations];
    const uint32_t n = rt::denoise::plan(p, dn.lds_max_step, list);
    for (uint32_t i = 0; i < n; i++) {
        const rt::denoise::Launch& L = list[i];
        rt::DenoiseParams K;
        std::memset(&K, 0, sizeof(K));
        K.band_w = band_width;
        K.band_h = band_height;
        K.step = L.step;
        K.spp = spp;
        K.feature_samples = float(feature_samples);
        K.k_normal = p.k_normal;
        K.k_depth = p.k_depth;
        K.k_color = L.k_color;
        K.accum = accum;
        K.sample_count = sample_count;
        K.feat0 = feat0;
        K.feat1 = feat1;
        const bool first = L.src == rt::denoise::BUF_CALLER, last = L.dst == rt::denoise::BUF_CALLER;
        if (!first) {
            K.src = plane[L.src - 1u];
            K.guide = plane[2];
        }
        if (!last) {
            K.dst = plane[L.dst - 1u];
            K.guide_out = plane[2];
        } else {
            K.out_mean = out_mean;
            K.out_rgba8 = reinterpret_cast<uint32_t*>(out_rgba8);
        }
        RT_HIP(rt::launch_denoise(K, first, last, L.lds_step, st));
    }
    return rt::mark_issued(ctx, st);
}

extern "C" int rt_denoise_variance_check(const rt_denoise_variance* params, uint32_t band_width, uint32_t band_height,
                                         uint32_t feature_samples) {
    rt_denoise_variance p;
    const char* err = "";
    if (int rc = rt::denoise::check_variance(params, band_width, band_height, feature_samples, &p, &err))
        return fail(rc, err);
    return RT_OK;
}

extern "C" int rt_denoise_variance_device(rt_context* ctx, const float* accum_a, const float* accum_b,
                                          const uint32_t* half_count, uint32_t half_spp, const float* feat0,
                                          const float* feat1, uint32_t feature_samples, uint32_t band_width,
                                          uint32_t band_height, const rt_denoise_variance* params, float* out_mean,
                                          uint8_t* out_rgba8, void* stream) {
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    rt_denoise_variance p;
    const char* err = "";
    if (int rc = rt::denoise::check_variance(params, band_width, band_height, feature_samples, &p, &err))
        return fail(rc, err);
    if (band_width == 0 || band_height == 0) return RT_OK;
    if (!accum_a || !accum_b || !feat0 || !feat1 || !out_rgba8)
        return fail(RT_ERR_INVALID_ARGUMENT,
                    "rt_denoise_variance_device: accum_a, accum_b, feat0, feat1 or out_rgba8 is NULL");
    const uint64_t texels = uint64_t(band_width) * band_height;
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = rt::order_on(ctx, st)) return rc;
    rt_context::Denoise& dn = ctx->denoise;
    if (p.prefilter + p.iterations > 1u && dn.cap < texels) {
        if (dn.planes) ctx->host_waits++;   // queued denoises still read the old planes: the stream drains
        if (int rc = rt::grow_on_stream(dn.planes, dn.cap, texels, 3u * 4u * sizeof(float), false, st)) return rc;
    }
    float* plane[3] = {nullptr, nullptr, nullptr};   // BUF_PING, BUF_PONG, the guide
    if (dn.planes)
        for (int k = 0; k < 3; k++) plane[k] = dn.planes + size_t(k) * dn.cap * 4u;
    rt::denoise::VarLaunch list[rt::denoise::kMaxVarLaunches];
    const uint32_t n = rt::denoise::plan_variance(p, dn.lds_max_step, list);
    for (uint32_t i = 0; i < n; i++) {
        const rt::denoise::VarLaunch& L = list[i];
        rt::DenoiseVarParams K;
        std::memset(&K, 0, sizeof(K));
        K.band_w = band_width;
        K.band_h = band_height;
        K.step = L.step;
        K.half_spp = half_spp;
        K.feature_samples = float(feature_samples);
        K.k_normal = p.k_normal;
        K.k_depth = p.k_depth;
        K.k_color = p.k_color;
        K.accum_a = accum_a;
        K.accum_b = accum_b;
        K.half_count = half_count;
        K.feat0 = feat0;
        K.feat1 = feat1;
        const bool first = L.src == rt::denoise::BUF_CALLER, last = L.dst == rt::denoise::BUF_CALLER;
        if (!first) {
            K.src = plane[L.src - 1u];
            K.guide = plane[2];
        }
        if (!last) {
            K.dst = plane[L.dst - 1u];
            K.guide_out = plane[2];
        } else {
            K.out_mean = out_mean;
            K.out_rgba8 = reinterpret_cast<uint32_t*>(out_rgba8);
        }
        RT_HIP(rt::launch_denoise_var(K, L.prefilter != 0u, first, last, L.lds_step, st));
    }
    return rt::mark_issued(ctx, st);
}

extern "C" int rt_temporal_check(const rt_temporal_params* params, uint32_t band_width, uint32_t band_height,
                                 uint32_t feature_samples) {
    rt_temporal_params p;
    const char* err = "";
    if (int rc = rt::temporal::check(params, band_width, band_height, feature_samples, &p, &err)) return fail(rc, err);
    return RT_OK;
}

extern "C" int rt_temporal_create(rt_context* ctx, uint32_t band_width, uint32_t band_height, rt_temporal** out) {
    if (!ctx || !out) return fail(RT_ERR_INVALID_ARGUMENT, "rt_temporal_create: ctx or out is NULL");
    *out = nullptr;
    const char* err = "";
    if (int rc = rt::temporal::check_band(band_width, band_height, &err)) return fail(rc, err);
    rt::DeviceGuard g(ctx->device);
    rt_temporal* t = new (std::nothrow) rt_temporal;
    if (!t) return fail(RT_ERR_OUT_OF_MEMORY, "rt_temporal_create: out of host memory");
    t->ctx = ctx;
    t->band_w = band_width;
    t->band_h = band_height;
    const size_t bytes = size_t(rt::temporal::state_bytes(band_width, band_height));
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&t->planes), bytes);
    // n = 0 everywhere before the call returns: the first accumulate may come on any stream
    if (e == hipSuccess) e = hipMemsetAsync(t->planes, 0, bytes, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        (void)hipFree(t->planes);
        delete t;
        return rt::fail_hip(e, "rt_temporal_create");
    }
    *out = t;
    return RT_OK;
}

extern "C" int rt_temporal_destroy(rt_temporal* temporal) {
    if (!temporal) return RT_OK;
    rt::DeviceGuard g(temporal->ctx->device);
    (void)hipFree(temporal->planes);   // waits for the queued calls that still use the planes
    (void)hipFree(temporal->planes2);
    delete temporal;
    return RT_OK;
}

extern "C" int rt_temporal_reset(rt_temporal* temporal, void* stream) {
    if (!temporal) return fail(RT_ERR_INVALID_ARGUMENT, "rt_temporal_reset: temporal is NULL");
    rt_context* ctx = temporal->ctx;
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = rt::order_on(ctx, st)) return rc;
    RT_HIP(hipMemsetAsync(temporal->set(temporal->cur), 0,
                          size_t(rt::temporal::state_bytes(temporal->band_w, temporal->band_h)), st));
    return rt::mark_issued(ctx, st);
}

namespace {

// The checks the two temporal calls share, before anything is queued, and their launch parameters
// but for the state's planes.
int temporal_setup(const std::string& who, rt_context* ctx, rt_temporal* temporal, const float* accum_a,
                   const float* accum_b, const uint32_t* sample_count, uint32_t spp, const float* feat0,
                   const float* feat1, uint32_t feature_samples, const rt_temporal_params* params, float* out_a,
                   float* out_b, uint8_t* out_rgba8, uint32_t* history_len, rt::TemporalParams& K) {
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, who + ": ctx is NULL");
    if (!temporal) return fail(RT_ERR_INVALID_ARGUMENT, who + ": temporal is NULL");
    if (temporal->ctx != ctx) return fail(RT_ERR_INVALID_ARGUMENT, who + ": temporal belongs to another context");
    rt_temporal_params p;
    const char* err = "";
    if (int rc = rt::temporal::check(params, temporal->band_w, temporal->band_h, feature_samples, &p, &err))
        return fail(rc, err);
    if (!accum_a || !feat0 || !feat1 || !out_a)
        return fail(RT_ERR_INVALID_ARGUMENT, who + ": accum_a, feat0, feat1 or out_a is NULL");
    if (accum_b && !out_b) return fail(RT_ERR_INVALID_ARGUMENT, who + ": accum_b is given and out_b is NULL");
    if (out_b && !accum_b) return fail(RT_ERR_INVALID_ARGUMENT, who + ": out_b is given and accum_b is NULL");
    std::memset(&K, 0, sizeof(K));
    K.band_w = temporal->band_w;
    K.band_h = temporal->band_h;
    K.spp = spp;
    K.feature_samples = float(feature_samples);
    K.k_normal = p.k_normal;
    K.k_depth = p.k_depth;
    K.max_history = float(p.max_history);
    K.accum_a = accum_a;
    K.accum_b = accum_b;
    K.sample_count = sample_count;
    K.feat0 = feat0;
    K.feat1 = feat1;
    K.out_a = out_a;
    K.out_b = out_b;
    K.out_rgba8 = reinterpret_cast<uint32_t*>(out_rgba8);
    K.history_len = history_len;
    return RT_OK;
}

}  // namespace

extern "C" int rt_temporal_accumulate_device(rt_context* ctx, rt_temporal* temporal, const float* accum_a,
                                             const float* accum_b, const uint32_t* sample_count, uint32_t spp,
                                             const float* feat0, const float* feat1, uint32_t feature_samples,
                                             const rt_temporal_params* params, float* out_a, float* out_b,
                                             uint8_t* out_rgba8, uint32_t* history_len, void* stream) {
    rt::TemporalParams K;
    if (int rc = temporal_setup("rt_temporal_accumulate_device", ctx, temporal, accum_a, accum_b, sample_count, spp, feat0,
                                feat1, feature_samples, params, out_a, out_b, out_rgba8, history_len, K))
        return rc;
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = rt::order_on(ctx, st)) return rc;
    const uint64_t plane = rt::temporal::plane_floats(temporal->band_w, temporal->band_h);
    float* cur = temporal->set(temporal->cur);
    K.ha = cur;
    K.hb = cur + plane;
    K.hg = cur + 2u * plane;
    RT_HIP(rt::launch_temporal(K, st));
    return rt::mark_issued(ctx, st);
}

extern "C" int rt_temporal_reproject_device(rt_context* ctx, rt_temporal* temporal, const float* accum_a,
                                            const float* accum_b, const uint32_t* sample_count, uint32_t spp,
                                            const float* feat0, const float* feat1, uint32_t feature_samples,
                                            const float* motion, const rt_temporal_params* params, float* out_a,
                                            float* out_b, uint8_t* out_rgba8, uint32_t* history_len, void* stream) {
    rt::TemporalReprojectParams R;
    std::memset(&R, 0, sizeof(R));
    if (int rc = temporal_setup("rt_temporal_reproject_device", ctx, temporal, accum_a, accum_b, sample_count, spp, feat0,
                                feat1, feature_samples, params, out_a, out_b, out_rgba8, history_len, R.T))
        return rc;
    if (!motion) return fail(RT_ERR_INVALID_ARGUMENT, "rt_temporal_reproject_device: motion is NULL");
    rt::DeviceGuard g(ctx->device);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = rt::order_on(ctx, st)) return rc;
    if (!temporal->planes2) {   // the first reprojected call of the state: the one that may wait
        const size_t bytes = size_t(rt::temporal::state_bytes(temporal->band_w, temporal->band_h));
        ctx->host_waits++;
        RT_HIP(hipMalloc(reinterpret_cast<void**>(&temporal->planes2), bytes));
        RT_HIP(hipMemsetAsync(temporal->planes2, 0, bytes, st));
    }
    const uint64_t plane = rt::temporal::plane_floats(temporal->band_w, temporal->band_h);
    const float* src = temporal->set(temporal->cur);
    float* dst = temporal->set(temporal->cur ^ 1);
    R.motion = motion;
    R.ha_src = src;
    R.hb_src = src + plane;
    R.hg_src = src + 2u * plane;
    R.T.ha = dst;
    R.T.hb = dst + plane;
    R.T.hg = dst + 2u * plane;
    RT_HIP(rt::launch_temporal_reproject(R, st));
    temporal->cur ^= 1;
    return rt::mark_issued(ctx, st);
}
