// rt_denoise_host.cpp — rt_denoise_host.h.
#include "rt_denoise_host.h"

#include <cmath>

namespace rt {
namespace denoise {

int check(const rt_denoise* params, uint32_t band_w, uint32_t band_h, uint32_t feature_samples, rt_denoise* p,
          const char** err) {
    const rt_denoise def = {3u, 4.0f, 16.0f, 1.0f};
    *p = params ? *params : def;
    *err = "";
    if (p->iterations < 1u || p->iterations > kMaxIterations) {
        *err = "rt_denoise: iterations must be 1..6";
        return RT_ERR_INVALID_ARGUMENT;
    }
    const float k[3] = {p->k_normal, p->k_depth, p->k_color};
    for (float v : k)
        if (!std::isfinite(v) || v < 0.0f) {
            *err = "rt_denoise: k_normal, k_depth and k_color must be finite and >= 0";
            return RT_ERR_INVALID_ARGUMENT;
        }
    if (feature_samples < 1u || feature_samples > kMaxFeatureSamples) {
        *err = "feature_samples must be 1..256";
        return RT_ERR_INVALID_ARGUMENT;
    }
    if (band_w > 65535u || band_h > 65535u) {
        *err = "band width and height must be below 65536";
        return RT_ERR_INVALID_ARGUMENT;
    }
    return RT_OK;
}

uint32_t plan(const rt_denoise& p, uint32_t lds_max_step, Launch out[kMaxIterations]) {
    const uint32_t n = p.iterations < kMaxIterations ? p.iterations : kMaxIterations;
    float kc = p.k_color;
    for (uint32_t i = 0; i < n; i++) {
        Launch& L = out[i];
        L.iteration = i;
        L.step = 1u << i;
        L.k_color = kc;
        L.lds_step = L.step <= lds_max_step ? L.step : 0u;
        L.src = i == 0 ? BUF_CALLER : (i & 1u) ? BUF_PING : BUF_PONG;
        L.dst = i + 1u == n ? BUF_CALLER : (i & 1u) ? BUF_PONG : BUF_PING;
        kc = kc * 4.0f;   // exact (a power of two) until it overflows to inf
    }
    return n;
}

}  // namespace denoise
}  // namespace rt
