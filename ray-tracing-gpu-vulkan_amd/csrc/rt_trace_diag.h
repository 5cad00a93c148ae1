// rt_trace_diag.h — the trace kernels' diagnostic builds (device only): the lane id, and the macros
// that -DRT_STAMPS (wave-level phase stamps), -DRT_ASM_MARKS (phase marks in an ISA listing),
// -DRT_UTIL (lane utilisation per code point) and -DRT_PLACEMENT (where the waves land) turn on, with
// the LDS words they count into. The shipped build compiles every one of them to nothing. They
// restate no reference shader line: the reference has no counterpart.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

// Diagnostic build only (-DRT_STAMPS): wave-level s_memtime phase stamps, summed per wave and
// added to Counters::stamp[] at exit (cdna_hip_programming.md §7, In-kernel stamps). The shipped
// build compiles every STAMP() to nothing.
struct Stamps { unsigned long long acc[8], t; uint32_t cur; };
#ifdef RT_STAMPS
#define STAMP(k)                                                                               \
    do {                                                                                       \
        __builtin_amdgcn_sched_barrier(0);                                                     \
        unsigned long long t_;                                                                 \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");           \
        __builtin_amdgcn_sched_barrier(0);                                                     \
        stamps.acc[stamps.cur] += t_ - stamps.t;                                               \
        stamps.t = t_;                                                                         \
        stamps.cur = (k);                                                                      \
    } while (0)
#define STAMP_DECL                                                                             \
    Stamps stamps = {{0, 0, 0, 0, 0, 0, 0, 0}, 0, 7};                                          \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamps.t)::"memory")
#define STAMP_FLUSH                                                                            \
    do {                                                                                       \
        STAMP(7);                                                                              \
        if (lane_id() == 0)                                                                    \
            for (int k_ = 0; k_ < 8; ++k_) atomicAdd(&P.counters->stamp[k_], stamps.acc[k_]);  \
    } while (0)
#elif defined(RT_ASM_MARKS)   // ISA listing only: phase boundaries as comments (scripts/isa_phases.py)
#define STAMP(k) asm volatile("; RT_PHASE " #k)
#define STAMP_DECL [[maybe_unused]] Stamps stamps
#define STAMP_FLUSH do {} while (0)
#else
#define STAMP(k) do {} while (0)
#define STAMP_DECL [[maybe_unused]] Stamps stamps
#define STAMP_FLUSH do {} while (0)
#endif

// Diagnostic build only (-DRT_UTIL): lane utilisation per code point. UTIL(k, pred) counts one
// wave pass through the point and the lanes executing it with `pred` true (block totals in LDS,
// added to Counters::util at exit; rt_debug_util). Points: 0 node visit, 1 leaf test, 2 sphere
// candidate (test4 loop), 3 shade, 4 diffuse, 5 metal, 6 dielectric, 7 sample start, 8 segment
// (tracing lanes of 64), 9 unit vector draw, 10 shade of a hit, 11 node visit from L2, 12 / 13 / 14
// node visits (LDS) of passes with at most 8 / 16 / 32 active lanes.
#ifdef RT_UTIL
__shared__ unsigned long long s_util[32];
#define UTIL(k, pred)                                                                          \
    do {                                                                                       \
        const unsigned long long b_ = __ballot(pred), a_ = __ballot(true);                     \
        if (lane_id() == uint32_t(__ffsll(a_) - 1)) {                                          \
            atomicAdd(&s_util[2 * (k)], 1ull);                                                 \
            atomicAdd(&s_util[2 * (k) + 1], (unsigned long long)__popcll(b_));               \
        }                                                                                      \
    } while (0)
#define UTIL_INIT do { if (threadIdx.x < 32) s_util[threadIdx.x] = 0ull; } while (0)
#define UTIL_FLUSH                                                                             \
    do {                                                                                       \
        __syncthreads();                                                                       \
        if (threadIdx.x < 32) atomicAdd(&P.counters->util[threadIdx.x], s_util[threadIdx.x]);  \
    } while (0)
#else
#define UTIL(k, pred) do {} while (0)
#define UTIL_INIT do {} while (0)
#define UTIL_FLUSH do {} while (0)
#endif

// Diagnostic build only (-DRT_PLACEMENT): where the trace kernel's waves land. Counters::util[k]
// (k = 0..3) = waves on SIMD k over the chip; util[8 + m] = blocks whose busiest SIMD holds m of
// their waves (from the HW_ID register).
#ifdef RT_PLACEMENT
__shared__ uint32_t s_simd[4];
#define PLACEMENT_RECORD(P)                                                                    \
    do {                                                                                       \
        if (threadIdx.x < 4) s_simd[threadIdx.x] = 0u;                                         \
        __syncthreads();                                                                       \
        const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);                         \
        const uint32_t simd = (hw >> 4) & 3u;                                                  \
        if (lane_id() == 0) {                                                                  \
            atomicAdd(&s_simd[simd], 1u);                                                      \
            atomicAdd(&(P).counters->util[simd], 1ull);                                        \
        }                                                                                      \
        __syncthreads();                                                                       \
        if (threadIdx.x == 0) {                                                                \
            const uint32_t m = max(max(s_simd[0], s_simd[1]), max(s_simd[2], s_simd[3]));      \
            atomicAdd(&(P).counters->util[8 + min(m, 23u)], 1ull);                             \
        }                                                                                      \
    } while (0)
#else
#define PLACEMENT_RECORD(P) do {} while (0)
#endif

}  // namespace
