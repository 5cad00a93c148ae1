// rt_denoise_var_host.h — the host half of rt_denoise_variance_device (rt_features.cpp) without HIP:
// the checks of the call's parameters and the list of kernel launches of a variance-guided denoise,
// `prefilter` feature-only passes over the variance and then `iterations` a-trous iterations. Plain
// C++, so the sanitizer build (tests/test_denoise_var_host.py) runs exactly this code. The kernels
// are rt_denoise_var.hip; the contract is include/rt_mi355x.h and DESIGN.md §3.1.3.
#pragma once

#include <cstdint>

#include "rt_denoise_host.h"

namespace rt {
namespace denoise {

constexpr uint32_t kMaxPrefilter = 3;
constexpr uint32_t kMaxVarLaunches = kMaxPrefilter + kMaxIterations;

struct VarLaunch {
    uint32_t prefilter;   // 1: a prefilter pass (v alone), 0: an iteration (e and v)
    uint32_t index;       // j of the prefilter passes, i of the iterations
    uint32_t step;        // 1 << index
    uint32_t lds_step;    // step when the launch stages its taps in LDS, else 0
    uint32_t src, dst;    // BUF_*: src BUF_CALLER = the prologue, dst BUF_CALLER = the epilogue
};

// rt_denoise_variance_check. *p: the parameters in force (the defaults for params == nullptr).
// Returns RT_OK or RT_ERR_INVALID_ARGUMENT with *err a static message.
int check_variance(const rt_denoise_variance* params, uint32_t band_w, uint32_t band_h, uint32_t feature_samples,
                   rt_denoise_variance* p, const char** err);

// The launches of a denoise with checked parameters p, in order: the prefilter passes, then the
// iterations, each reading what the one before wrote; lds_max_step as for plan(). Returns their
// count (p.prefilter + p.iterations).
uint32_t plan_variance(const rt_denoise_variance& p, uint32_t lds_max_step, VarLaunch out[kMaxVarLaunches]);

}  // namespace denoise
}  // namespace rt
