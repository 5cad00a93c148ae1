"""CPU restatement of the variance-guided denoise (rt_denoise_variance_device; include/rt_mi355x.h,
DESIGN.md §3.1.3) in binary32 numpy: one float32 numpy operation per contract operation, taps in
the contract's order, taps outside the band skipped. The kernel, the features, the random inputs
and the PSNR are denoise_sim's. Helper module of test_denoise_var_host.py,
test_denoise_var_quality.py, test_gpu_denoise_var.py and test_cli_denoise_var.py (no tests here)."""
import numpy as np

from denoise_sim import KERNEL, features, psnr, random_inputs  # noqa: F401  (re-exported)

f32 = np.float32
DEFAULTS = (3, 2, 4.0, 16.0, 0.25)    # iterations, prefilter, k_normal, k_depth, k_color
V_FLOOR = 2.0 ** -20


def random_halves(seed, H, W, F):
    """(accum_a, accum_b, feat0, feat1): denoise_sim.random_inputs for A and the features, and a
    second seeded draw of the colour sums for B."""
    accum_a, feat0, feat1 = random_inputs(seed, H, W, F)
    accum_b = np.ones((H, W, 4), f32)
    accum_b[..., :3] = np.random.default_rng(seed + 7919).uniform(0.0, 8.0, (H, W, 3))
    return accum_a, accum_b, feat0, feat1


def prologue(accum_a, accum_b, feat0, feat1, F, half_spp=None, half_count=None):
    """(e_0 [H, W, 3], v_0 [H, W], a [H, W, 3], nrm [H, W, 3], z [H, W])."""
    A, B, feat0, feat1 = (np.asarray(v, f32) for v in (accum_a, accum_b, feat0, feat1))
    H, W = A.shape[:2]
    h = np.full((H, W), half_spp, np.uint32) if half_count is None else np.asarray(half_count, np.uint32)
    hf = h.astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ma = np.where((h > 0)[..., None], A[..., 0:3] / hf[..., None], f32(0.0)).astype(f32)
        mb = np.where((h > 0)[..., None], B[..., 0:3] / hf[..., None], f32(0.0)).astype(f32)
    a = feat0[..., 0:3] / f32(F) + f32(2.0 ** -6)
    nrm = feat1[..., 0:3] / f32(F)
    z = feat1[..., 3] / f32(F)
    e = ((ma + mb) * f32(0.5)) / a
    d = (ma - mb) / a
    v = f32(0.25) * ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    return e, v, a, nrm, z


def _taps(H, W, step):
    """(kk, P, Q) per tap in the contract's order, P the texels whose tap Q lies in the band."""
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * step, dx * step
            y0, y1, x0, x1 = max(0, -oy), min(H, H - oy), max(0, -ox), min(W, W - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            yield (f32(KERNEL[abs(dy)]) * f32(KERNEL[abs(dx)]), (slice(y0, y1), slice(x0, x1)),
                   (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox)))


def _feature_stop(nrm, z, P, Q, k_normal, k_depth):
    one = f32(1.0)
    dn = nrm[P] - nrm[Q]
    dn2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
    dz = (z[P] - z[Q]) / (z[P] + one)
    return (one + k_normal * dn2) * (one + k_depth * (dz * dz))


def denoise(accum_a, accum_b, feat0, feat1, F, half_spp=None, half_count=None, params=DEFAULTS, track=True,
            return_variance=False):
    """mean [H, W, 4] float32 = (e_I a, 1). track=False holds the prefiltered variance fixed through
    the iterations (not the contract: the measurement of what carrying it is worth)."""
    iterations, prefilter, k_normal, k_depth, k_color = params
    k_normal, k_depth, k_color = f32(k_normal), f32(k_depth), f32(k_color)
    one = f32(1.0)
    e, v, a, nrm, z = prologue(accum_a, accum_b, feat0, feat1, F, half_spp, half_count)
    H, W = z.shape
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for j in range(prefilter):
            nv = np.zeros((H, W), f32)
            den = np.zeros((H, W), f32)
            for kk, P, Q in _taps(H, W, 1 << j):
                f = _feature_stop(nrm, z, P, Q, k_normal, k_depth)
                w = kk / (f * f)
                nv[P] = nv[P] + w * v[Q]
                den[P] = den[P] + w
            v = nv / den
        for i in range(iterations):
            num = np.zeros((H, W, 3), f32)
            den = np.zeros((H, W), f32)
            nv = np.zeros((H, W), f32)
            vp = v + f32(V_FLOOR)
            for kk, P, Q in _taps(H, W, 1 << i):
                f = _feature_stop(nrm, z, P, Q, k_normal, k_depth)
                de = e[P] - e[Q]
                de2 = (de[..., 0] * de[..., 0] + de[..., 1] * de[..., 1]) + de[..., 2] * de[..., 2]
                x = f * (one + k_color * (de2 / vp[P]))
                w = kk / (x * x)
                num[P] = num[P] + w[..., None] * e[Q]
                den[P] = den[P] + w
                nv[P] = nv[P] + (w * w) * v[Q]
            e = num / den[..., None]
            if track:
                v = nv / (den * den)
    mean = np.ones((H, W, 4), f32)
    mean[..., 0:3] = e * a
    assert mean.dtype == f32 and e.dtype == f32 and v.dtype == f32
    return (mean, v) if return_variance else mean
