// denoise_var_host_main.cpp — the host half of rt_denoise_variance_device
// (csrc/rt_denoise_var_host.cpp: parameter checks and the launch list) as a stand-alone program for
// the sanitizer build of tests/test_denoise_var_host.py: the refusal cases of
// rt_denoise_variance_check and the plan of every (prefilter, iterations) pair at every LDS limit.
// Every launch is also printed, one line each, for the test to check against its own expectation:
//   launch <lds_max> <prefilter> <iterations> <k> <is_prefilter> <index> <step> <lds_step> <src> <dst>
// Exits 0 and prints the number of checks when all hold.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../ray-tracing-gpu-vulkan_amd/csrc/rt_denoise_var_host.h"

namespace dn = rt::denoise;

static int g_checks = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);  \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static int check(const rt_denoise_variance* p, uint32_t w, uint32_t h, uint32_t f) {
    rt_denoise_variance out;
    const char* err = nullptr;
    const int rc = dn::check_variance(p, w, h, f, &out, &err);
    CHECK(err != nullptr);
    CHECK((rc == RT_OK) == (err[0] == '\0'));
    return rc;
}

int main() {
    // the defaults
    rt_denoise_variance out;
    const char* err = nullptr;
    CHECK(dn::check_variance(nullptr, 1920, 1080, 16, &out, &err) == RT_OK);
    CHECK(out.iterations == 3 && out.prefilter == 2 && out.k_normal == 4.0f && out.k_depth == 16.0f &&
          out.k_color == 0.25f);
    // refusals: rt_denoise_check's, and prefilter > 3
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    rt_denoise_variance p = {3, 2, 4.0f, 16.0f, 0.25f};
    CHECK(check(&p, 64, 36, 16) == RT_OK);
    for (uint32_t it : {0u, 7u, 0xffffffffu}) {
        rt_denoise_variance q = p;
        q.iterations = it;
        CHECK(check(&q, 64, 36, 16) == RT_ERR_INVALID_ARGUMENT);
    }
    for (uint32_t pre : {4u, 5u, 0xffffffffu}) {
        rt_denoise_variance q = p;
        q.prefilter = pre;
        CHECK(check(&q, 64, 36, 16) == RT_ERR_INVALID_ARGUMENT);
    }
    for (uint32_t pre = 0; pre <= dn::kMaxPrefilter; pre++)
        for (uint32_t it = 1; it <= dn::kMaxIterations; it++) {
            rt_denoise_variance q = p;
            q.prefilter = pre;
            q.iterations = it;
            CHECK(check(&q, 64, 36, 16) == RT_OK);
        }
    for (float bad : {-1.0f, -0x1p-149f, inf, -inf, nan})
        for (int k = 0; k < 3; k++) {
            rt_denoise_variance q = p;
            (k == 0 ? q.k_normal : k == 1 ? q.k_depth : q.k_color) = bad;
            CHECK(check(&q, 64, 36, 16) == RT_ERR_INVALID_ARGUMENT);
        }
    rt_denoise_variance zero = {1, 0, 0.0f, 0.0f, 0.0f};
    CHECK(check(&zero, 64, 36, 1) == RT_OK);
    CHECK(check(&p, 64, 36, 0) == RT_ERR_INVALID_ARGUMENT);
    CHECK(check(&p, 64, 36, 257) == RT_ERR_INVALID_ARGUMENT);
    CHECK(check(&p, 64, 36, 256) == RT_OK);
    CHECK(check(&p, 65536, 36, 16) == RT_ERR_INVALID_ARGUMENT);
    CHECK(check(&p, 64, 65536, 16) == RT_ERR_INVALID_ARGUMENT);
    CHECK(check(&p, 65535, 65535, 16) == RT_OK);
    CHECK(check(&p, 0, 0, 16) == RT_OK);
    // the launch list: the prefilter passes at steps 1, 2, 4, then the iterations at steps 1, 2, ...;
    // the caller's buffers at both ends, the context's two buffers alternating in between, never
    // read and written by one launch; the last launch is an iteration
    for (uint32_t lds_max : {0u, 1u, 2u, 4u})
        for (uint32_t pre = 0; pre <= dn::kMaxPrefilter; pre++)
            for (uint32_t it = 1; it <= dn::kMaxIterations; it++) {
                rt_denoise_variance q = {it, pre, 4.0f, 16.0f, 0.25f};
                std::vector<dn::VarLaunch> list(dn::kMaxVarLaunches);
                const uint32_t n = dn::plan_variance(q, lds_max, list.data());
                CHECK(n == pre + it);
                for (uint32_t k = 0; k < n; k++) {
                    const dn::VarLaunch& L = list[k];
                    CHECK(L.prefilter == (k < pre ? 1u : 0u));
                    CHECK(L.index == (k < pre ? k : k - pre) && L.step == (1u << L.index));
                    CHECK(L.lds_step == (L.step <= lds_max ? L.step : 0u));
                    CHECK((L.src == dn::BUF_CALLER) == (k == 0));
                    CHECK((L.dst == dn::BUF_CALLER) == (k + 1 == n));
                    CHECK(L.src != L.dst || n == 1);
                    if (k) CHECK(L.src == list[k - 1].dst);
                    std::printf("launch %u %u %u %u %u %u %u %u %u %u\n", lds_max, pre, it, k, L.prefilter, L.index, L.step,
                                L.lds_step, L.src, L.dst);
                }
                CHECK(list[n - 1].prefilter == 0u);
            }
    std::printf("%d checks passed (ASan + UBSan)\n", g_checks);
    return 0;
}
