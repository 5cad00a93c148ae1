// rt_debug_kernels.hip — diagnostic kernels that evaluate pieces of the trace kernels on their own:
// the contract primitives (rt_debug_math_kernel), the exhaustive checks of rcp_cr / sqrt_cr and the
// camera division (rt_debug_exact_kernel) and of normalize's sqrt_rcp_cr (rt_debug_exact_normalize_kernel), and one bounce of given hits by the frames' own shade_rec
// (rt_scatter_probe_kernel: shader.rchit:38-133); with their launchers. It includes the unit and
// shading headers and none of the walks.
#include <hip/hip_runtime.h>

#include "rt_device_math.h"
#include "rt_internal.h"
#include "rt_launchers.h"
#include "rt_trace_diag.h"
#include "rt_trace_units.h"
#include "rt_trace_shade.h"

using namespace rtd;

namespace {

// Diagnostic: device evaluation of contract primitives (tests/test_gpu_parity.py).
__global__ void rt_debug_math_kernel(int op, const float* __restrict__ in, float* __restrict__ out,
                                     uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = in[2 * i], y = in[2 * i + 1];
    float r = 0.0f;
    switch (op) {
        case 0: r = __builtin_sqrtf(x); break;
        case 1: r = x / y; break;
        case 2: r = sinf_det(x); break;
        case 3: r = __builtin_fmaf(x, y, 1.0f); break;
        case 4: { V3 v = normalize(v3(x, y, 0.5f)); r = v.x; break; }
        case 5: r = pow5(x); break;
        case 6: r = __uint_as_float(sample_seed_hash(__float_as_uint(x), __float_as_uint(y))); break;
        case 7: r = __uint_as_float(sample_fixed(x)); break;
        case 8: r = 0.0f; break;   // high word of the (32-bit) per-sample value
        case 9: r = checker_positive(x, y, 0.5f * (x - y)) ? 1.0f : 0.0f; break;
        case 10: { V3 v = normalize(v3(x, y, 0.5f)); r = v.y; break; }
        case 11: { V3 v = normalize_sqrt_rcp(v3(x, y, 0.5f)); r = v.y; break; }
        default: r = 0.0f;
    }
    out[i] = r;
}

// Diagnostic (rt_debug_scatter, rt_probe_scatter.cpp): one bounce of K.n given hits, a lane per
// case, by the frames' own shade_rec in its MODE_SCATTER instantiation: the STREAM path's shading of
// a hit, which stores the bounce where a frame goes on to the next segment. Case i is ray i traced
// along normalize(v), which hit sphere ids[i] at t[i] with the LCG in state seeds[i]. REC: the
// sphere's records come from the static LDS table, staged as rt_trace_grid_kernel stages it
// (load_hit_rec); otherwise from the scene's global arrays (load_hit). The host checked ids[i] <
// n_spheres, and n_spheres <= kRecStatic for REC.
template <bool REC>
__global__ __launch_bounds__(256) void rt_scatter_probe_kernel(const rt::ScatterProbeParams K) {
    const float4* mat4 = reinterpret_cast<const float4*>(K.mat);
    if (REC) {
        const uint32_t n = min(K.n_spheres, rt::kRecStatic);
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
            const rt::GeomRec g = K.geom[i];
            s_rec[3 * i] = make_float4(g.cx, g.cy, g.cz, K.radius[i]);
            s_rec[3 * i + 1] = mat4[2 * i];
            s_rec[3 * i + 2] = mat4[2 * i + 1];
        }
        __syncthreads();
    }
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= K.n) return;
    const float* q = K.rays + 6u * size_t(i);
    V3 o = v3(q[0], q[1], q[2]);
    V3 d = normalize(v3(q[3], q[4], q[5]));
    const uint32_t bi = K.ids[i];
    const HitRec hr = REC ? load_hit_rec(bi) : load_hit(reinterpret_cast<const float4*>(K.geom), mat4, bi);
    // of the launch parameters MODE_SCATTER reads probe_out alone, and no camera (shade_rec says so at
    // its MODE_SCATTER branch): the zeroed structs only fill its signature and compile away
    rt::TraceParams P{};
    P.probe_out = K.out;
    const Camera cam{};
    Path ps{};
    ps.px = i;
    ps.seed = K.seeds[i];
    ps.thr = v3(1.0f, 1.0f, 1.0f);
    bool fresh = false;
    shade_rec<rt::MODE_SCATTER, false>(P, cam, hr, ps, bi, K.t[i], o, d, fresh);
}

// Diagnostic: rcp_cr / sqrt_cr against hipcc's correctly rounded 1.0f / x and sqrtf over all 2^32
// inputs (base .. base + grid * 256); mismatches counted in bad[0] / bad[1] (NaN equals NaN). With
// div_b != 0: the camera's float(double(x) * (1 / double(div_b))) against x / div_b for every
// x in [0, 65536) (the camera's numerators), mismatches in bad[2].
__global__ __launch_bounds__(256) void rt_debug_exact_kernel(uint64_t base, float div_b, unsigned long long* bad) {
    const uint32_t bits = uint32_t(base + uint64_t(blockIdx.x) * blockDim.x + threadIdx.x);
    const float x = __uint_as_float(bits);
    if (div_b != 0.0f) {
        if (bits >= 0x47800000u) return;   // x >= 65536
        const float q0 = float(double(x) * (1.0 / double(div_b))), q1 = x / div_b;
        const unsigned long long mq = __ballot(__float_as_uint(q0) != __float_as_uint(q1));
        if (lane_id() == 0 && mq) atomicAdd(&bad[2], (unsigned long long)__popcll(mq));
        return;
    }
    const float r0 = rcp_cr(x), r1 = 1.0f / x, s0 = sqrt_cr(x), s1 = __builtin_sqrtf(x);
    const bool rb = __float_as_uint(r0) != __float_as_uint(r1) && !(r0 != r0 && r1 != r1);
    const bool sb = __float_as_uint(s0) != __float_as_uint(s1) && !(s0 != s0 && s1 != s1);
    const unsigned long long mr = __ballot(rb), ms = __ballot(sb);
    if (lane_id() == 0 && (mr | ms)) {
        atomicAdd(&bad[0], (unsigned long long)__popcll(mr));
        atomicAdd(&bad[1], (unsigned long long)__popcll(ms));
    }
}

// Diagnostic: sqrt_rcp_cr (normalize's length and reciprocal from one v_rsq_f32) and sqrt_rsq against
// hipcc's correctly rounded sqrtf(x) and 1.0f / sqrtf(x) over all 2^32 inputs (base .. base + grid *
// 256), NaN equals NaN: mismatches of the length in bad[0], of the reciprocal in bad[1], of sqrt_rsq
// in bad[2]; bad[3] counts the x in [2^-100, 2^100] that took sqrt_rcp_cr's rare branch.
__global__ __launch_bounds__(256) void rt_debug_exact_normalize_kernel(uint64_t base, unsigned long long* bad) {
    const uint32_t bits = uint32_t(base + uint64_t(blockIdx.x) * blockDim.x + threadIdx.x);
    const float x = __uint_as_float(bits);
    float len, inv;
    bool rare;
    sqrt_rcp_cr(x, len, inv, &rare);
    const float s2 = sqrt_rsq(x), s1 = __builtin_sqrtf(x), r1 = 1.0f / s1;
    const bool lb = __float_as_uint(len) != __float_as_uint(s1) && !(len != len && s1 != s1);
    const bool rb = __float_as_uint(inv) != __float_as_uint(r1) && !(inv != inv && r1 != r1);
    const bool sb = __float_as_uint(s2) != __float_as_uint(s1) && !(s2 != s2 && s1 != s1);
    const bool in_range = !(bits - 0x0d800000u > 0x71800000u - 0x0d800000u);
    const unsigned long long ml = __ballot(lb), mr = __ballot(rb), ms = __ballot(sb), mo = __ballot(rare && in_range);
    if (lane_id() == 0 && (ml | mr | ms | mo)) {
        atomicAdd(&bad[0], (unsigned long long)__popcll(ml));
        atomicAdd(&bad[1], (unsigned long long)__popcll(mr));
        atomicAdd(&bad[2], (unsigned long long)__popcll(ms));
        atomicAdd(&bad[3], (unsigned long long)__popcll(mo));
    }
}

}  // namespace

// ---- host-callable launchers (rt_launchers.h) -----------------------------------------------
namespace rt {

hipError_t launch_debug_exact(unsigned long long* bad, hipStream_t st) {
    const uint32_t grid = 1u << 22;   // 2^30 inputs per launch, 4 launches
    for (uint64_t base = 0; base < (1ull << 32); base += uint64_t(grid) * 256u)
        hipLaunchKernelGGL(rt_debug_exact_kernel, dim3(grid), dim3(256), 0, st, base, 0.0f, bad);
    // camera divisors: the BASELINE sizes, small and odd ones, the largest band extent
    const float divs[] = {1920.0f, 1080.0f, 3840.0f, 2160.0f, 64.0f, 36.0f, 1.0f, 3.0f, 7.0f, 1000.0f, 65535.0f};
    for (float b : divs)
        for (uint64_t base = 0; base < 0x47800000ull; base += uint64_t(grid) * 256u)
            hipLaunchKernelGGL(rt_debug_exact_kernel, dim3(grid), dim3(256), 0, st, base, b, bad);
    return hipGetLastError();
}

hipError_t launch_debug_exact_normalize(unsigned long long* bad, hipStream_t st) {
    const uint32_t grid = 1u << 22;   // 2^30 inputs per launch, 4 launches
    for (uint64_t base = 0; base < (1ull << 32); base += uint64_t(grid) * 256u)
        hipLaunchKernelGGL(rt_debug_exact_normalize_kernel, dim3(grid), dim3(256), 0, st, base, bad);
    return hipGetLastError();
}

hipError_t launch_debug_math(int op, const float* in, float* out, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(rt_debug_math_kernel, dim3((n + 255) / 256), dim3(256), 0, st, op, in, out, n);
    return hipGetLastError();
}

hipError_t launch_scatter_probe(const ScatterProbeParams& K, bool rec, hipStream_t st) {
    if (K.n == 0) return hipSuccess;
    const dim3 grid((K.n + 255u) / 256u), block(256);
    if (rec) hipLaunchKernelGGL(rt_scatter_probe_kernel<true>, grid, block, 0, st, K);
    else hipLaunchKernelGGL(rt_scatter_probe_kernel<false>, grid, block, 0, st, K);
    return hipGetLastError();
}

}  // namespace rt
