"""Quality of the temporal stage on the CPU: the oracle's frames of the canonical
scene in the counter-based stream at 96x54 and 4 spp, frame k at scene time k dt rendered as two
halves at sample_base 4 k and 4 k + 2, 16 feature samples at sample_base 0, the default k, through
the numpy restatements (tests/temporal_sim.py, then denoise_sim.py or denoise_var_sim.py), against
the oracle's 1024-spp frame of the same scene time at sample_base 1 << 20. PSNR on sqrt(clip(mean)).
The whole table is printed; only the orderings that held in the prototype with more than 1.3 dB to
spare are asserted:
  static, N 32, frame 5   temporal alone above the plain filter's single frame;
                          temporal + variance above the variance filter's single frame
  dt 0.05, N 8, frame 9   temporal + variance above the variance filter's single frame
  dt 0.2, N 8, frame 7    temporal + variance above the variance filter's single frame;
                          temporal alone above the noisy frame"""
import numpy as np
import pytest

import denoise_sim as ds
import denoise_var_sim as dv
import temporal_sim as ts

W, H, F, SPP, REF_SPP, REF_BASE = 96, 54, 16, 4, 1024, 1 << 20
f32 = np.float32
ROWS = {"static": (0.0, 32, 5), "dt 0.05": (0.05, 8, 9), "dt 0.2": (0.2, 8, 7)}    # dt, N, the frame measured
COLUMNS = ("noisy", "plain", "variance", "temporal", "temporal + plain", "temporal + variance")


@pytest.fixture(scope="module")
def table(oracle):
    rays = ds.camera_rays(oracle, oracle.render_call_info(SPP, W, H), W, H, F)       # the camera stands still
    half_rci = oracle.render_call_info(SPP // 2, W, H)
    done = {}

    def row(name):
        if name in done:
            return done[name]
        dt, N, last = ROWS[name]
        two, one = ts.State(H, W), ts.State(H, W)
        params = (N,) + ts.DEFAULTS[1:]
        for k in range(last + 1):
            sc = oracle.generate_scene(float(f32(k * dt)))
            A, _, _ = oracle.render(sc, half_rci, W, H, opts=oracle.options(rng_mode=ds.HASH, sample_base=SPP * k))
            B, _, _ = oracle.render(sc, half_rci, W, H, opts=oracle.options(rng_mode=ds.HASH, sample_base=SPP * k + SPP // 2))
            feat0, feat1 = ds.sum_samples(ds.sample_values(oracle, sc, rays))
            out_a, out_b, mean, n = ts.accumulate(two, A, feat0, feat1, F, accum_b=B, spp=SPP // 2, params=params)
            sum_a, _, _, _ = ts.accumulate(one, A + B, feat0, feat1, F, spp=SPP, params=params)
        ref, _, _ = oracle.render(sc, oracle.render_call_info(REF_SPP, W, H), W, H,
                                  opts=oracle.options(rng_mode=ds.HASH, sample_base=REF_BASE))
        ref_mean = ref[..., :3] / f32(REF_SPP)
        got = {
            "noisy": ds.psnr((A + B)[..., :3] / f32(SPP), ref_mean),
            "plain": ds.psnr(ds.denoise(A + B, feat0, feat1, F, spp=SPP), ref_mean),
            "variance": ds.psnr(dv.denoise(A, B, feat0, feat1, F, half_spp=SPP // 2), ref_mean),
            "temporal": ds.psnr(mean, ref_mean),
            "temporal + plain": ds.psnr(ds.denoise(sum_a, feat0, feat1, F, spp=1), ref_mean),
            "temporal + variance": ds.psnr(dv.denoise(out_a, out_b, feat0, feat1, F, half_spp=1), ref_mean),
        }
        print(f"{W}x{H} {SPP} spp, {name}, N {N}, frame {last} (history valid on {100.0 * np.mean(n > 1):.1f} % of the texels): "
              + ", ".join(f"{c} {got[c]:.2f} dB" for c in COLUMNS))
        done[name] = got
        return got
    return row


def test_static_scene(table):
    r = table("static")
    assert r["temporal"] > r["plain"]
    assert r["temporal + variance"] > r["variance"]


def test_slow_motion(table):
    r = table("dt 0.05")
    assert r["temporal + variance"] > r["variance"]


def test_fast_motion(table):
    r = table("dt 0.2")
    assert r["temporal + variance"] > r["variance"]
    assert r["temporal"] > r["noisy"]
