// rt_temporal_host.cpp — rt_temporal_host.h.
#include "rt_temporal_host.h"

#include <cmath>

namespace rt {
namespace temporal {

int check(const rt_temporal_params* params, uint32_t band_w, uint32_t band_h, uint32_t feature_samples,
          rt_temporal_params* p, const char** err) {
    *p = params ? *params : kDefaults;
    // the band and the feature samples are rt_denoise_check's
    rt_denoise unused;
    if (int rc = denoise::check(nullptr, band_w, band_h, feature_samples, &unused, err)) return rc;
    if (p->max_history < kMinHistory || p->max_history > kMaxHistory) {
        *err = "rt_temporal_params: max_history must be 2..65535";
        return RT_ERR_INVALID_ARGUMENT;
    }
    if (!std::isfinite(p->k_normal) || p->k_normal < 0.0f) {
        *err = "rt_temporal_params: k_normal must be finite and >= 0";
        return RT_ERR_INVALID_ARGUMENT;
    }
    if (!std::isfinite(p->k_depth) || p->k_depth < 0.0f) {
        *err = "rt_temporal_params: k_depth must be finite and >= 0";
        return RT_ERR_INVALID_ARGUMENT;
    }
    if (p->reserved != 0u) {
        *err = "rt_temporal_params: reserved must be 0";
        return RT_ERR_INVALID_ARGUMENT;
    }
    return RT_OK;
}

int check_band(uint32_t band_w, uint32_t band_h, const char** err) {
    *err = "";
    if (band_w == 0u || band_h == 0u || band_w > 65535u || band_h > 65535u) {
        *err = "rt_temporal_create: band width and height must be within 1 .. 65535";
        return RT_ERR_INVALID_ARGUMENT;
    }
    return RT_OK;
}

uint64_t plane_texels(uint32_t band_w, uint32_t band_h) { return uint64_t(band_w) * band_h; }

uint64_t plane_floats(uint32_t band_w, uint32_t band_h) { return plane_texels(band_w, band_h) * 4u; }

uint64_t state_bytes(uint32_t band_w, uint32_t band_h) {
    return plane_floats(band_w, band_h) * kPlanes * sizeof(float);
}

}  // namespace temporal
}  // namespace rt
