// rt_denoise_var_host.cpp — rt_denoise_var_host.h.
#include "rt_denoise_var_host.h"

namespace rt {
namespace denoise {

int check_variance(const rt_denoise_variance* params, uint32_t band_w, uint32_t band_h, uint32_t feature_samples,
                   rt_denoise_variance* p, const char** err) {
    const rt_denoise_variance def = {3u, 2u, 4.0f, 16.0f, 0.25f};
    *p = params ? *params : def;
    // everything but the prefilter count is rt_denoise_check's
    const rt_denoise plain = {p->iterations, p->k_normal, p->k_depth, p->k_color};
    rt_denoise unused;
    if (int rc = check(&plain, band_w, band_h, feature_samples, &unused, err)) return rc;
    if (p->prefilter > kMaxPrefilter) {
        *err = "rt_denoise_variance: prefilter must be 0..3";
        return RT_ERR_INVALID_ARGUMENT;
    }
    return RT_OK;
}

uint32_t plan_variance(const rt_denoise_variance& p, uint32_t lds_max_step, VarLaunch out[kMaxVarLaunches]) {
    const uint32_t pre = p.prefilter < kMaxPrefilter ? p.prefilter : kMaxPrefilter;
    const uint32_t it = p.iterations < kMaxIterations ? p.iterations : kMaxIterations;
    const uint32_t n = pre + it;
    for (uint32_t k = 0; k < n; k++) {
        VarLaunch& L = out[k];
        L.prefilter = k < pre ? 1u : 0u;
        L.index = k < pre ? k : k - pre;
        L.step = 1u << L.index;
        L.lds_step = L.step <= lds_max_step ? L.step : 0u;
        L.src = k == 0 ? BUF_CALLER : (k & 1u) ? BUF_PING : BUF_PONG;
        L.dst = k + 1u == n ? BUF_CALLER : (k & 1u) ? BUF_PONG : BUF_PING;
    }
    return n;
}

}  // namespace denoise
}  // namespace rt
