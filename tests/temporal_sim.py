"""CPU restatement of the temporal stage (rt_temporal_accumulate_device; include/rt_mi355x.h,
DESIGN.md §3.1.3) in binary32 numpy: one float32 numpy operation per contract operation, in the
contract's order. The demodulation and the guide are denoise_sim.prologue's expressions; the state is
the small class below, three [H, W, 4] float32 planes as the library holds them. Helper module of
test_temporal_host.py, test_temporal_quality.py, test_gpu_temporal.py and test_cli_temporal.py (no
tests here)."""
import numpy as np

from denoise_sim import prologue, psnr, random_inputs  # noqa: F401  (re-exported)

f32 = np.float32
DEFAULTS = (8, 4.0, 16.0)    # max_history, k_normal, k_depth


class State:
    """HA = (eA.rgb, n), HB = (eB.rgb, n), HG = (nrm.xyz, z) of a band; n = 0 after create and reset."""

    def __init__(self, H, W):
        self.H, self.W = H, W
        self.reset()

    def reset(self):
        self.ha = np.zeros((self.H, self.W, 4), f32)
        self.hb = np.zeros((self.H, self.W, 4), f32)
        self.hg = np.zeros((self.H, self.W, 4), f32)

    def copy(self):
        s = State(self.H, self.W)
        s.ha, s.hb, s.hg = self.ha.copy(), self.hb.copy(), self.hg.copy()
        return s


def accumulate(state, accum_a, feat0, feat1, F, accum_b=None, spp=None, sample_count=None, params=DEFAULTS):
    """One call on `state`, updated in place. Returns (out_a, out_b or None, mean [H, W, 4],
    history_len uint32 [H, W]); rgba8 is oracle.resolve(mean, 1)."""
    max_history, k_normal, k_depth = params
    k_normal, k_depth, nmax, one = f32(k_normal), f32(k_depth), f32(max_history), f32(1.0)
    H, W = state.H, state.W
    h = np.full((H, W), spp, np.uint32) if sample_count is None else np.asarray(sample_count, np.uint32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        # e = c / a with c = h ? A.rgb / float(h) : 0, a = feat0.rgb / F + 2^-6, nrm, z
        ea, a, nrm, z = prologue(accum_a, feat0, feat1, F, spp, sample_count)
        dn = nrm - state.hg[..., 0:3]
        dn2 = (dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2]
        dz = (z - state.hg[..., 3]) / (z + one)
        x = (one + k_normal * dn2) * (one + k_depth * (dz * dz))
        n0 = state.ha[..., 3]
        valid = (n0 > 0) & (x < f32(2.0))
        measured = h > 0
        n = np.where(measured, np.where(valid, np.minimum(n0 + one, nmax), one), np.where(valid, n0, f32(0.0))).astype(f32)
        alpha = one / n

        def integrate(e, hist):
            blended = hist[..., 0:3] + alpha[..., None] * (e - hist[..., 0:3])
            with_h = np.where(valid[..., None], blended, e)
            without = np.where(valid[..., None], hist[..., 0:3], f32(0.0))
            out = np.where(measured[..., None], with_h, without).astype(f32)
            assert out.dtype == f32 and blended.dtype == f32
            return out

        new_a = integrate(ea, state.ha)
        out_a = np.ones((H, W, 4), f32)
        out_a[..., 0:3] = new_a * a
        mean = out_a.copy()
        out_b = None
        if accum_b is not None:
            eb, _, _, _ = prologue(accum_b, feat0, feat1, F, spp, sample_count)
            new_b = integrate(eb, state.hb)
            out_b = np.ones((H, W, 4), f32)
            out_b[..., 0:3] = new_b * a
            mean[..., 0:3] = ((new_a + new_b) * f32(0.5)) * a
            state.hb = np.concatenate([new_b, n[..., None]], axis=-1).astype(f32)
    state.ha = np.concatenate([new_a, n[..., None]], axis=-1).astype(f32)
    state.hg = np.concatenate([nrm, z[..., None]], axis=-1).astype(f32)
    return out_a, out_b, mean, n.astype(np.uint32)
