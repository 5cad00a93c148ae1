// rt_denoise_host.h — the host half of rt_denoise_device (rt_features.cpp) without HIP: the checks of
// the call's parameters and the list of kernel launches of a denoise, one per a-trous iteration.
// Plain C++, so the sanitizer build (tests/test_denoise_host.py) runs exactly this code. The kernels
// are rt_denoise.hip; the contract is include/rt_mi355x.h and DESIGN.md §3.1.3.
#pragma once

#include <cstdint>

#include "../../include/rt_mi355x.h"

namespace rt {
namespace denoise {

constexpr uint32_t kMaxIterations = 6;
constexpr uint32_t kMaxFeatureSamples = RT_FEATURE_MAX_SAMPLES;
// The kernels' thread block: kTileW x kTileH texels, one thread each (four waves, a wave two rows
// of 32 texels: a tap's loads are two 512-byte row segments).
constexpr uint32_t kTileW = 32, kTileH = 8;
// Iterations of step <= kLdsMaxStep stage their tile and its halo of 2 step texels in LDS
// ((kTileW + 4 step) x (kTileH + 4 step) texels of 32 B: 13.5, 20 and 36 KiB at steps 1, 2 and 4);
// larger steps read their taps from global memory (the halo outgrows the tile).
constexpr uint32_t kLdsMaxStep = 4;

// Where an iteration reads the filtered colour e from and writes it to: the caller's buffers
// (prologue / epilogue folded into the kernel) or one of the context's two band buffers.
enum : uint32_t { BUF_CALLER = 0, BUF_PING = 1, BUF_PONG = 2 };

struct Launch {
    uint32_t iteration;   // i
    uint32_t step;        // 1 << i
    float k_color;        // k_color * 4^i, the binary32 product
    uint32_t lds_step;    // step when the iteration stages its taps in LDS, else 0
    uint32_t src, dst;    // BUF_*: src BUF_CALLER = the prologue, dst BUF_CALLER = the epilogue
};

// rt_denoise_check. *p: the parameters in force (the defaults for params == nullptr). Returns
// RT_OK or RT_ERR_INVALID_ARGUMENT with *err a static message.
int check(const rt_denoise* params, uint32_t band_w, uint32_t band_h, uint32_t feature_samples, rt_denoise* p,
          const char** err);

// The launches of a denoise with checked parameters p, in order; lds_max_step: the largest step
// staged in LDS (kLdsMaxStep; 0: every iteration reads global memory). Returns their count
// (p.iterations).
uint32_t plan(const rt_denoise& p, uint32_t lds_max_step, Launch out[kMaxIterations]);

}  // namespace denoise
}  // namespace rt
