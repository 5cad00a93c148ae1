"""CPU model of the two halves an adaptive or feedback frame hands over (rt_half_outputs, DESIGN.md
§3.1.2), on adaptive_sim.cube, the per-sample 8.24 integers of the unchanged oracle: the integer
planes (A, B) per texel and their resolve np.float32(A.astype(np.float64) * 2.0**-24). The product
is exact (A < 2^53), so there is one rounding, as in the kernel. Helper module of test_gpu_halves.py,
test_gpu_halves_chain.py and test_cli_feedback_denoise.py (no tests here)."""
import numpy as np

import adaptive_sim as sim


def cube_of(oracle, scene, rci, W, H, base, n):
    """adaptive_sim.cube for a frame loop, where every frame has its own camera and sample range: the
    8.24 integers Q[s, y, x, c] of samples base .. base + n - 1 under the RenderCallInfo `rci` (its
    samplesPerRenderCall is ignored)."""
    one = np.array(rci, np.uint32, copy=True)
    one[1] = 1
    q = np.zeros((n, H, W, 3), np.int64)
    for s in range(n):
        acc, _, _ = oracle.render(scene, one, W, H, opts=oracle.options(rng_mode=sim.HASH, sample_base=base + s))
        v = acc[..., :3].astype(np.float64) * 2.0 ** 24   # one sample: <= 2^24, exact in binary32
        assert np.array_equal(v, np.floor(v))
        q[s] = v.astype(np.int64)
    return q


def resolve(q):
    """Integer planes [H, W, 3] -> the float4 accumulator [H, W, 4] the resolve stores: (sum, 1)."""
    assert q.dtype == np.int64 and int(q.max(initial=0)) < (1 << 53)
    acc = np.ones(q.shape[:2] + (4,), np.float32)
    acc[..., :3] = (q.astype(np.float64) * 2.0 ** -24).astype(np.float32)
    return acc


def even_table(table):
    """The counts a feedback frame renders: every count rounded up to even."""
    return [(int(n) + 1) & ~1 for n in table]


def feedback_planes(Q, table):
    """The planes of a feedback frame of `table` (even counts, row-major tiles) on the cube Q, whose
    sample 0 is the frame's sample_base: per tile of count n = 2 h, A = the sum of Q[:h], B = of
    Q[h:n]. Returns (A, B, half) with A, B int64 [H, W, 3] and half uint32 [H, W]."""
    _, H, W, _ = Q.shape
    tx = (W + 7) // 8
    A = np.zeros((H, W, 3), np.int64)
    B = np.zeros((H, W, 3), np.int64)
    half = np.zeros((H, W), np.uint32)
    for t, n in enumerate(table):
        assert n % 2 == 0 and n <= Q.shape[0], (t, n)
        ys, xs = slice((t // tx) * 8, (t // tx) * 8 + 8), slice((t % tx) * 8, (t % tx) * 8 + 8)
        h = n // 2
        A[ys, xs] = Q[:h, ys, xs].sum(axis=0)
        B[ys, xs] = Q[h:n, ys, xs].sum(axis=0)
        half[ys, xs] = h
    return A, B, half


def feedback_halves(Q, table):
    """(accum_a, accum_b, half_count) of a feedback halves frame."""
    A, B, half = feedback_planes(Q, table)
    return resolve(A), resolve(B), half


def adaptive_planes(Q, min_spp, step_spp, max_spp, thr_q16):
    """adaptive_sim.simulate's pass loop, restated to return the planes: (A, B, counts) with A, B
    int64 [H, W, 3] and counts uint32 [H, W] (n per texel; the half count is n / 2)."""
    _, H, W, _ = Q.shape
    A = np.zeros((H, W, 3), np.int64)
    B = np.zeros((H, W, 3), np.int64)
    counts = np.zeros((H, W), np.uint32)
    for ty in range(0, H, 8):
        for tx in range(0, W, 8):
            q = Q[:, ty:ty + 8, tx:tx + 8, :]
            m = q.shape[1] * q.shape[2]
            a = np.zeros(q.shape[1:], np.int64)
            b = np.zeros(q.shape[1:], np.int64)
            n = p = 0
            while True:
                k = min_spp if p == 0 else min(step_spp, max_spp - n)
                a += q[n:n + k // 2].sum(axis=0)
                b += q[n + k // 2:n + k].sum(axis=0)
                n += k
                p += 1
                if sim.converged(np.abs(a - b).sum(), (a + b).sum(), n, m, thr_q16) or n >= max_spp:
                    break
            A[ty:ty + 8, tx:tx + 8] = a
            B[ty:ty + 8, tx:tx + 8] = b
            counts[ty:ty + 8, tx:tx + 8] = n
    return A, B, counts


def adaptive_halves(Q, min_spp, step_spp, max_spp, thr_q16):
    """(accum_a, accum_b, half_count, counts) of an adaptive halves frame."""
    A, B, counts = adaptive_planes(Q, min_spp, step_spp, max_spp, thr_q16)
    return resolve(A), resolve(B), counts // 2, counts
