// temporal_host_main.cpp — the host half of the temporal stage (csrc/rt_temporal_host.cpp: the
// parameter check, the defaults and the plane sizes) as a stand-alone program for the sanitizer build
// of tests/test_temporal_host.py: the accept and refusal cases of rt_temporal_check, each refusal's
// message naming its field, the band check of rt_temporal_create and the sizes of a state up to the
// largest band. Exits 0 and prints the number of checks when all hold.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_temporal_host.h"

namespace tp = rt::temporal;

static int g_checks = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static int check(const rt_temporal_params* p, uint32_t w, uint32_t h, uint32_t f, const char* names = nullptr) {
    rt_temporal_params out;
    const char* err = nullptr;
    const int rc = tp::check(p, w, h, f, &out, &err);
    CHECK(err != nullptr);
    CHECK((rc == RT_OK) == (err[0] == '\0'));
    if (names) CHECK(rc == RT_ERR_INVALID_ARGUMENT && std::strstr(err, names) != nullptr);
    return rc;
}

int main() {
    // the defaults
    rt_temporal_params out;
    const char* err = nullptr;
    CHECK(tp::check(nullptr, 1920, 1080, 16, &out, &err) == RT_OK);
    CHECK(out.max_history == 8 && out.k_normal == 4.0f && out.k_depth == 16.0f && out.reserved == 0);
    const rt_temporal_params p = {8, 4.0f, 16.0f, 0};
    CHECK(check(&p, 64, 36, 16) == RT_OK);
    // max_history 2 .. 65535
    for (uint32_t n : {0u, 1u, 65536u, 0xffffffffu}) {
        rt_temporal_params q = p;
        q.max_history = n;
        check(&q, 64, 36, 16, "max_history");
    }
    for (uint32_t n : {2u, 3u, 8u, 32u, 65535u}) {
        rt_temporal_params q = p;
        q.max_history = n;
        CHECK(check(&q, 64, 36, 16) == RT_OK);
    }
    // k finite and >= 0
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    for (float bad : {-1.0f, -0x1p-149f, inf, -inf, nan}) {
        rt_temporal_params q = p;
        q.k_normal = bad;
        check(&q, 64, 36, 16, "k_normal");
        q = p;
        q.k_depth = bad;
        check(&q, 64, 36, 16, "k_depth");
    }
    const rt_temporal_params zero = {2, 0.0f, 0.0f, 0};
    CHECK(check(&zero, 64, 36, 1) == RT_OK);
    // reserved
    for (uint32_t r : {1u, 0x80000000u}) {
        rt_temporal_params q = p;
        q.reserved = r;
        check(&q, 64, 36, 16, "reserved");
    }
    // rt_denoise_check's size and feature-sample limits
    check(&p, 64, 36, 0, "feature_samples");
    check(&p, 64, 36, 257, "feature_samples");
    check(nullptr, 64, 36, 257, "feature_samples");
    CHECK(check(&p, 64, 36, 256) == RT_OK);
    check(&p, 65536, 36, 16, "width");
    check(&p, 64, 65536, 16, "height");
    CHECK(check(&p, 65535, 65535, 16) == RT_OK);
    // the band of a state
    CHECK(tp::check_band(1, 1, &err) == RT_OK && err[0] == '\0');
    CHECK(tp::check_band(65535, 65535, &err) == RT_OK);
    for (uint32_t bad : {0u, 65536u, 0xffffffffu}) {
        CHECK(tp::check_band(bad, 36, &err) == RT_ERR_INVALID_ARGUMENT && err[0] != '\0');
        CHECK(tp::check_band(64, bad, &err) == RT_ERR_INVALID_ARGUMENT && err[0] != '\0');
    }
    // the sizes: three float4 planes, no overflow at the largest band
    CHECK(tp::kPlanes == 3);
    CHECK(tp::plane_texels(1, 1) == 1 && tp::plane_floats(1, 1) == 4 && tp::state_bytes(1, 1) == 48);
    CHECK(tp::plane_texels(1920, 1080) == 2073600ull && tp::state_bytes(1920, 1080) == 2073600ull * 48ull);
    CHECK(tp::plane_texels(65535, 65535) == 4294836225ull);
    CHECK(tp::plane_floats(65535, 65535) == 4294836225ull * 4ull);
    CHECK(tp::state_bytes(65535, 65535) == 4294836225ull * 48ull);
    std::printf("%d checks passed (ASan + UBSan)\n", g_checks);
    return 0;
}
