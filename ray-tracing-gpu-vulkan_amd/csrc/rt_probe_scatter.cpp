// rt_probe_scatter.cpp — rt_debug_scatter (include/rt_mi355x_debug.h): one bounce of a batch of given
// hits by the frames' own shading (rt_trace_shade.h shade_rec, instantiated as MODE_SCATTER: the STREAM
// path's code for a hit, storing the bounce), a lane per case, with the sphere's records read the two ways the trace kernels read them:
// from the scene's global arrays (load_hit) or from the static LDS table of the REC grid kernels
// (load_hit_rec). No launch plan, no hand-out, no tile costs: the kernel is its own
// (rt_scatter_probe_kernel) and a context's frames do not see it. The host half (argument checks)
// is rt_probe_batch.cpp, without HIP.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/rt_mi355x_debug.h"
#include "rt_context.h"
#include "rt_launchers.h"
#include "rt_probe_batch.h"

using rt::fail;

extern "C" int rt_debug_scatter(rt_context* ctx, const float* rays6, const uint32_t* ids, const float* t,
                                const uint32_t* seeds, uint32_t n, uint32_t form, float* out_p, float* out_att,
                                float* out_sd, float* out_dnext, uint32_t* out_scatter, uint32_t* out_seed) {
    if (!ctx) return fail(RT_ERR_INVALID_ARGUMENT, "ctx is NULL");
    if (ctx->pending) return fail(RT_ERR_INVALID_ARGUMENT, "rt_debug_scatter between the halves of a scene build");
    if (!ctx->scene_set) return fail(RT_ERR_NO_SCENE, "rt_debug_scatter before rt_set_scene");
    if (!rt::probe::scatter_form_ok(form, ctx->scene.n_spheres, rt::kRecStatic))
        return fail(RT_ERR_INVALID_ARGUMENT,
                    form > rt::probe::kScatterFormRec ? "unknown form"
                                                      : "form 1 (records in LDS) holds at most 512 spheres");
    if (n == 0) return RT_OK;
    if (!rays6 || !ids || !t || !seeds || !out_p || !out_att || !out_sd || !out_dnext || !out_scatter || !out_seed)
        return fail(RT_ERR_INVALID_ARGUMENT, "an input or output array is NULL");
    if (n > rt::probe::kProbeMaxRays) return fail(RT_ERR_INVALID_ARGUMENT, "more than 2^24 cases");
    if (const uint32_t bad = rt::probe::check_scatter_batch(rays6, ids, t, n, ctx->scene.n_spheres))
        return fail(RT_ERR_INVALID_ARGUMENT,
                    "case " + std::to_string(bad - 1u) +
                        ": a ray or t that is not finite, a direction without a nonzero component, or a sphere "
                        "index beyond the scene");

    rt::DeviceGuard g(ctx->device);
    hipStream_t st = nullptr;
    if (int rc = rt::order_on(ctx, st)) return rc;
    // the batch and its answers on the device, for this call only: rays, then ids, t and seeds
    struct Buffers {
        uint32_t* in = nullptr;
        uint32_t* out = nullptr;
        ~Buffers() {
            (void)hipFree(in);
            (void)hipFree(out);
        }
    } buf;
    const size_t sn = n;
    RT_HIP(hipMalloc(reinterpret_cast<void**>(&buf.in), sn * 9u * sizeof(uint32_t)));
    RT_HIP(hipMalloc(reinterpret_cast<void**>(&buf.out), sn * 14u * sizeof(uint32_t)));
    RT_HIP(hipMemcpyAsync(buf.in, rays6, sn * 6u * sizeof(float), hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(buf.in + 6u * sn, ids, sn * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(buf.in + 7u * sn, t, sn * sizeof(float), hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(buf.in + 8u * sn, seeds, sn * sizeof(uint32_t), hipMemcpyHostToDevice, st));

    rt::ScatterProbeParams K;
    std::memset(&K, 0, sizeof(K));
    K.n_spheres = ctx->scene.n_spheres;
    K.geom = ctx->scene.geom;
    K.radius = ctx->scene.radius;
    K.mat = ctx->scene.mat;
    K.n = n;
    K.rays = reinterpret_cast<const float*>(buf.in);
    K.ids = buf.in + 6u * sn;
    K.t = reinterpret_cast<const float*>(buf.in + 7u * sn);
    K.seeds = buf.in + 8u * sn;
    K.out = buf.out;
    RT_HIP(rt::launch_scatter_probe(K, form == rt::probe::kScatterFormRec, st));
    if (int rc = rt::render_issued(ctx, st)) return rc;
    std::vector<uint32_t> out(sn * 14u);
    RT_HIP(hipMemcpyAsync(out.data(), buf.out, out.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    float* const fouts[4] = {out_p, out_att, out_sd, out_dnext};
    for (size_t i = 0; i < sn; i++) {
        const uint32_t* w = &out[14u * i];
        for (int k = 0; k < 4; k++) std::memcpy(fouts[k] + 3u * i, w + 3 * k, 3u * sizeof(float));
        out_scatter[i] = w[12];
        out_seed[i] = w[13];
    }
    return RT_OK;
}
