// The rsq chain of rt_device_math.h's sqrt_rcp_cr on the hardware, written out with one and two Newton
// steps side by side: every binary32 x in [2^-100, 2^100] against hipcc's correctly rounded sqrtf(x)
// and 1.0f / sqrtf(x), the seed (v_rsq_f32) against RN(1 / sqrt(x)), and the bits of the first misses
// (profiles/normalize_rsq_exhaustive.txt). The shipped helper's own check is
// rt_debug_exact_normalize_exhaustive.
//   hipcc -O3 -std=c++17 -ffp-contract=off -fno-fast-math --offload-arch=gfx950 scripts/rsq_chain_exhaustive.hip -o rsq_chain_exhaustive
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#define NC 16
#define NEX 64

__device__ __forceinline__ bool differs(float a, float b) {
    return __float_as_uint(a) != __float_as_uint(b) && !(a != a && b != b);
}

__device__ __forceinline__ void cnt(unsigned long long* c, int k, bool p) {
    const unsigned long long m = __ballot(p);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&c[k], (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(256) void probe(uint64_t base, unsigned long long* c, uint32_t* ex1, uint32_t* ex2, uint32_t* exs) {
    const uint32_t ux = uint32_t(base + uint64_t(blockIdx.x) * blockDim.x + threadIdx.x);
    const float x = __uint_as_float(ux);
    const bool inr = !(ux - 0x0d800000u > 0x71800000u - 0x0d800000u);
    const float R = __builtin_amdgcn_rsqf(x);
    float S = x * R, H = 0.5f * R;
    const float E = __builtin_fmaf(-H, S, 0.5f);
    H = __builtin_fmaf(H, E, H);
    S = __builtin_fmaf(S, E, S);
    const float D = __builtin_fmaf(-S, S, x);
    S = __builtin_fmaf(D, H, S);
    const float r0 = H + H;
    float e = __builtin_fmaf(-S, r0, 1.0f);
    const float q1 = __builtin_fmaf(e, r0, r0);
    e = __builtin_fmaf(-S, q1, 1.0f);
    const float q2 = __builtin_fmaf(e, q1, q1);
    const float sref = __builtin_sqrtf(x);
    const float qref = 1.0f / sref;
    const bool ones = ((__float_as_uint(sref) + 1u) & 0x7fffffu) == 0u;
    // seed error against RN(1/sqrt(x)) in ulps (double reference)
    const float rn = float(1.0 / __builtin_sqrt(double(x)));
    const int du = int(__float_as_uint(R)) - int(__float_as_uint(rn));
    cnt(c, 0, inr);
    if (inr && differs(S, sref)) { atomicAdd(&c[1], 1ull); uint32_t k = atomicAdd(&exs[0], 1u); if (k < NEX) exs[1 + k] = ux; }
    if (inr && differs(q1, qref)) {
        atomicAdd(&c[2], 1ull);
        if (!ones) { atomicAdd(&c[3], 1ull); uint32_t k = atomicAdd(&ex1[0], 1u); if (k < NEX) ex1[1 + k] = ux; }
    }
    if (inr && differs(q2, qref)) {
        atomicAdd(&c[4], 1ull);
        if (!ones) { atomicAdd(&c[5], 1ull); uint32_t k = atomicAdd(&ex2[0], 1u); if (k < NEX) ex2[1 + k] = ux; }
    }
    cnt(c, 6, inr && ones);
    cnt(c, 7, inr && du == 0);
    cnt(c, 8, inr && (du == 1 || du == -1));
    cnt(c, 9, inr && (du > 1 || du < -1));
    // q1 misses within [1, 4) alone (comparable with the model table)
    if (ux >= 0x3f800000u && ux < 0x40800000u) {
        if (differs(q1, qref)) atomicAdd(&c[10], 1ull);
        if (differs(q2, qref)) atomicAdd(&c[11], 1ull);
    }
    cnt(c, 12, ux >= 0x3f800000u && ux < 0x40800000u && du != 0);
}

#define CK(e) do { hipError_t _r = (e); if (_r != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(_r), __LINE__); return 1; } } while (0)

int main() {
    unsigned long long* c; uint32_t *ex1, *ex2, *exs;
    CK(hipMalloc(&c, NC * 8)); CK(hipMemset(c, 0, NC * 8));
    CK(hipMalloc(&ex1, (NEX + 1) * 4)); CK(hipMemset(ex1, 0, (NEX + 1) * 4));
    CK(hipMalloc(&ex2, (NEX + 1) * 4)); CK(hipMemset(ex2, 0, (NEX + 1) * 4));
    CK(hipMalloc(&exs, (NEX + 1) * 4)); CK(hipMemset(exs, 0, (NEX + 1) * 4));
    const uint32_t grid = 1u << 22;
    for (uint64_t base = 0; base < (1ull << 32); base += uint64_t(grid) * 256u)
        hipLaunchKernelGGL(probe, dim3(grid), dim3(256), 0, 0, base, c, ex1, ex2, exs);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    unsigned long long h[NC]; uint32_t h1[NEX + 1], h2[NEX + 1], hs[NEX + 1];
    CK(hipMemcpy(h, c, sizeof(h), hipMemcpyDeviceToHost));
    CK(hipMemcpy(h1, ex1, sizeof(h1), hipMemcpyDeviceToHost));
    CK(hipMemcpy(h2, ex2, sizeof(h2), hipMemcpyDeviceToHost));
    CK(hipMemcpy(hs, exs, sizeof(hs), hipMemcpyDeviceToHost));
    printf("in range %llu\nS miss %llu\nq1 miss %llu (not all-ones len: %llu)\nq2 miss %llu (not all-ones len: %llu)\n"
           "all-ones len %llu\nseed exact %llu, 1 ulp off %llu, further %llu\n[1,4): q1 miss %llu q2 miss %llu seed inexact %llu\n",
           h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9], h[10], h[11], h[12]);
    auto dump = [](const char* n, uint32_t* e) {
        printf("%s examples (%u):", n, e[0]);
        for (uint32_t i = 0; i < e[0] && i < NEX; i++) printf(" %08x", e[1 + i]);
        printf("\n");
    };
    dump("S", hs); dump("q1 (not all-ones)", h1); dump("q2 (not all-ones)", h2);
    return 0;
}
