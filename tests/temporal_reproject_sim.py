"""CPU restatement of the reprojected temporal call (rt_temporal_reproject_device; include/rt_mi355x.h,
DESIGN.md §3.1.3) in binary32 numpy: one float32 numpy operation per contract operation, in the
contract's order. The state extends temporal_sim.State with the second plane set the call writes;
temporal_sim.accumulate works in place on the current set, as the library's in-place call does. Helper
module of test_temporal_reproject_sim.py, test_gpu_temporal_reproject.py, test_cli_reproject.py and
test_temporal_reproject_quality.py (no tests here)."""
import numpy as np

import temporal_sim as ts
from denoise_sim import prologue

f32 = np.float32
DEFAULTS = ts.DEFAULTS
SNAP = f32(2.0 ** -6)


class State(ts.State):
    """ha, hb, hg are the current set (temporal_sim.accumulate and reset work on it); `other` is the
    set the next reprojected call writes, zero when the library allocates it."""

    def __init__(self, H, W):
        super().__init__(H, W)
        self.other = [np.zeros((H, W, 4), f32) for _ in range(3)]

    def copy(self):
        s = State(self.H, self.W)
        s.ha, s.hb, s.hg = self.ha.copy(), self.hb.copy(), self.hg.copy()
        s.other = [p.copy() for p in self.other]
        return s


def taps(motion):
    """The four taps of every texel: [(tx, ty, w)], float32 [H, W] each; a snapped texel's first tap is
    its one tap and its other three weigh 0."""
    half, one = f32(0.5), f32(1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        bx, by = motion[..., 0] - half, motion[..., 1] - half
        jx, jy = np.floor(bx + half), np.floor(by + half)
        snap = (np.abs(bx - jx) <= SNAP) & (np.abs(by - jy) <= SNAP)
        ix, iy = np.floor(bx), np.floor(by)
        fx, fy = bx - ix, by - iy
        gx, gy = one - fx, one - fy
        zero = np.zeros_like(bx)
        out = [(np.where(snap, jx, ix), np.where(snap, jy, iy), np.where(snap, one, gx * gy)),
               (ix + one, iy, np.where(snap, zero, fx * gy)),
               (ix, iy + one, np.where(snap, zero, gx * fy)),
               (ix + one, iy + one, np.where(snap, zero, fx * fy))]
    assert all(v.dtype == f32 for t in out for v in t)
    return out, snap


def history(state, nrm, z, motion, params, two):
    """(valid, HA [H, W, 4], HB.rgb [H, W, 3] or None, Wt): the reprojected history of every texel."""
    _, k_normal, k_depth = params
    k_normal, k_depth, one = f32(k_normal), f32(k_depth), f32(1.0)
    H, W = state.H, state.W
    tap_list, _ = taps(motion)
    ok = motion[..., 3] > 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ze = z + motion[..., 2]
        Wt = np.zeros((H, W), f32)
        S = np.zeros((H, W, 4), f32)
        SB = np.zeros((H, W, 3), f32)
        for tx, ty, w in tap_list:
            inside = ok & (w > 0) & (tx >= 0) & (tx < f32(W)) & (ty >= 0) & (ty < f32(H))
            qx = np.where(inside, tx, f32(0.0)).astype(np.int64)
            qy = np.where(inside, ty, f32(0.0)).astype(np.int64)
            HA, HG, HB = state.ha[qy, qx], state.hg[qy, qx], state.hb[qy, qx]
            dn = nrm - HG[..., 0:3]
            dn2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
            dz = (ze - HG[..., 3]) / (ze + one)
            x = (one + k_normal * dn2) * (one + k_depth * (dz * dz))
            counts = inside & (HA[..., 3] > 0) & (x < f32(2.0))
            Wt = Wt + np.where(counts, w, f32(0.0))
            S = S + np.where(counts[..., None], w[..., None] * HA, f32(0.0))
            if two:
                SB = SB + np.where(counts[..., None], w[..., None] * HB[..., 0:3], f32(0.0))
        valid = Wt > 0
        HA = S / Wt[..., None]
        HB = SB / Wt[..., None] if two else None
    assert Wt.dtype == f32 and S.dtype == f32 and SB.dtype == f32 and HA.dtype == f32
    return valid, HA, HB, Wt


def reproject(state, accum_a, feat0, feat1, F, motion, accum_b=None, spp=None, sample_count=None, params=DEFAULTS):
    """One reprojected call on `state`: reads the current set, writes the other and makes it current.
    Returns temporal_sim.accumulate's tuple (out_a, out_b or None, mean, history_len)."""
    max_history = params[0]
    nmax, one = f32(max_history), f32(1.0)
    H, W = state.H, state.W
    motion = np.asarray(motion, f32)
    two = accum_b is not None
    h = np.full((H, W), spp, np.uint32) if sample_count is None else np.asarray(sample_count, np.uint32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ea, a, nrm, z = prologue(accum_a, feat0, feat1, F, spp, sample_count)
        valid, HA, HB, _ = history(state, nrm, z, motion, params, two)
        n0 = HA[..., 3]
        measured = h > 0
        n = np.where(measured, np.where(valid, np.minimum(n0 + one, nmax), one), np.where(valid, n0, f32(0.0))).astype(f32)
        alpha = one / n

        def integrate(e, hist):
            blended = hist + alpha[..., None] * (e - hist)
            with_h = np.where(valid[..., None], blended, e)
            without = np.where(valid[..., None], hist, f32(0.0))
            out = np.where(measured[..., None], with_h, without).astype(f32)
            assert out.dtype == f32 and blended.dtype == f32
            return out

        new_a = integrate(ea, HA[..., 0:3])
        out_a = np.ones((H, W, 4), f32)
        out_a[..., 0:3] = new_a * a
        mean = out_a.copy()
        out_b = None
        dst_ha, dst_hb, dst_hg = state.other
        if two:
            eb, _, _, _ = prologue(accum_b, feat0, feat1, F, spp, sample_count)
            new_b = integrate(eb, HB)
            out_b = np.ones((H, W, 4), f32)
            out_b[..., 0:3] = new_b * a
            mean[..., 0:3] = ((new_a + new_b) * f32(0.5)) * a
            dst_hb = np.concatenate([new_b, n[..., None]], axis=-1).astype(f32)   # (one accumulator: left as it was)
    dst_ha = np.concatenate([new_a, n[..., None]], axis=-1).astype(f32)
    dst_hg = np.concatenate([nrm, z[..., None]], axis=-1).astype(f32)
    state.other = [state.ha, state.hb, state.hg]
    state.ha, state.hb, state.hg = dst_ha, dst_hb, dst_hg
    return out_a, out_b, mean, n.astype(np.uint32)


def identity_motion(H, W, ok=1.0):
    """The motion plane of a frame nothing moved in: every texel's own centre."""
    m = np.zeros((H, W, 4), f32)
    m[..., 0] = np.arange(W, dtype=f32)[None, :] + f32(0.5)
    m[..., 1] = np.arange(H, dtype=f32)[:, None] + f32(0.5)
    m[..., 3] = ok
    return m
