// rt_probe_batch.cpp — rt_probe_batch.h.
#include "rt_probe_batch.h"

#include <cmath>
#include <cstring>

namespace rt {
namespace probe {

uint32_t stage_batch(const float* rays6, uint32_t n, std::vector<float>& rays, uint32_t* band_h, float* cam_r) {
    const uint32_t rows = (n + kProbeBandW - 1u) / kProbeBandW;
    float far_r = 0.0f;
    for (uint32_t i = 0; i < n; i++) {
        const float* q = rays6 + 6u * size_t(i);
        for (int k = 0; k < 6; k++)
            if (!std::isfinite(q[k])) return i + 1u;
        if (q[3] == 0.0f && q[4] == 0.0f && q[5] == 0.0f) return i + 1u;
        const float r = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
        if (!std::isfinite(r)) return i + 1u;
        if (r > far_r) far_r = r;
    }
    const size_t texels = size_t(rows) * kProbeBandW;
    rays.resize(texels * 6u);
    std::memcpy(rays.data(), rays6, size_t(n) * 6u * sizeof(float));
    for (size_t i = n; i < texels; i++) std::memcpy(&rays[6u * i], rays6, 6u * sizeof(float));
    *band_h = rows;
    *cam_r = far_r;
    return 0;
}

uint32_t check_scatter_batch(const float* rays6, const uint32_t* ids, const float* t, uint32_t n, uint32_t n_spheres) {
    for (uint32_t i = 0; i < n; i++) {
        const float* q = rays6 + 6u * size_t(i);
        for (int k = 0; k < 6; k++)
            if (!std::isfinite(q[k])) return i + 1u;
        if (q[3] == 0.0f && q[4] == 0.0f && q[5] == 0.0f) return i + 1u;
        if (!std::isfinite(t[i])) return i + 1u;
        if (ids[i] >= n_spheres) return i + 1u;
    }
    return 0;
}

bool scatter_form_ok(uint32_t form, uint32_t n_spheres, uint32_t rec_capacity) {
    if (form == kScatterFormGlobal) return true;
    return form == kScatterFormRec && n_spheres <= rec_capacity;
}

}  // namespace probe
}  // namespace rt
