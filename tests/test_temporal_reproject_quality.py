"""Quality of the reprojected temporal stage on the CPU, in test_temporal_quality.py's
setup: the oracle's frames of the canonical scene in the counter-based stream at 96x54 and 4 spp in two
halves, 16 feature samples at sample_base 0, the default k, through the binary32 restatements
(motion_sim.py, temporal_reproject_sim.py and temporal_sim.py, then denoise_var_sim.py), against the
oracle's 1024-spp frame of the same frame. Frame k's camera stands at (13 + s k, 11, -3 + 2 s k) and
looks at the origin; scene time is k dt. PSNR on sqrt(clip(mean)). The whole table is printed; only the
orderings that held in the float64 prototype with more than 1.3 dB to spare are asserted:
  camera s = 0.05          reprojected above in place; reprojected + variance above the variance filter
  camera s = 0.2           reprojected above in place; reprojected + variance above temporal + variance
                           and above the variance filter
  objects dt 0.2           reprojected + variance above the variance filter
and the static row's reprojected columns equal its in-place columns exactly."""
import numpy as np
import pytest

import denoise_sim as ds
import denoise_var_sim as dv
import motion_sim as ms
import temporal_reproject_sim as tr
import temporal_sim as ts
from test_motion_host import moved_camera

W, H, F, SPP, REF_SPP, REF_BASE = 96, 54, 16, 4, 1024, 1 << 20
f32 = np.float32
# s, dt, N, the frame measured
ROWS = {"static": (0.0, 0.0, 32, 5), "objects dt 0.2": (0.0, 0.2, 8, 7), "camera s 0.05": (0.05, 0.0, 8, 7),
        "camera s 0.2": (0.2, 0.0, 8, 7), "camera s 0.2, objects dt 0.2": (0.2, 0.2, 8, 7)}
COLUMNS = ("noisy", "variance", "temporal", "temporal + variance", "reprojected", "reprojected + variance")


@pytest.fixture(scope="module")
def table(oracle):
    done = {}

    def row(name):
        if name in done:
            return done[name]
        s, dt, N, last = ROWS[name]
        here, moved = ts.State(H, W), tr.State(H, W)
        params = (N,) + ts.DEFAULTS[1:]
        prev = (None, None)
        for k in range(last + 1):
            sc = oracle.generate_scene(float(f32(k * dt)))
            rci = moved_camera(oracle, SPP, W, H, s, k)
            half_rci = moved_camera(oracle, SPP // 2, W, H, s, k)
            A, _, _ = oracle.render(sc, half_rci, W, H, opts=oracle.options(rng_mode=ds.HASH, sample_base=SPP * k))
            B, _, _ = oracle.render(sc, half_rci, W, H, opts=oracle.options(rng_mode=ds.HASH, sample_base=SPP * k + SPP // 2))
            feat0, feat1 = ds.features(oracle, sc, rci, W, H, F)
            motion = ms.motion(oracle, sc, rci, W, H, *prev)
            prev = (sc, rci)
            t_a, t_b, t_mean, _ = ts.accumulate(here, A, feat0, feat1, F, accum_b=B, spp=SPP // 2, params=params)
            r_a, r_b, r_mean, n = tr.reproject(moved, A, feat0, feat1, F, motion, accum_b=B, spp=SPP // 2, params=params)
        ref, _, _ = oracle.render(sc, moved_camera(oracle, REF_SPP, W, H, s, last), W, H,
                                  opts=oracle.options(rng_mode=ds.HASH, sample_base=REF_BASE))
        ref_mean = ref[..., :3] / f32(REF_SPP)
        got = {
            "noisy": ds.psnr((A + B)[..., :3] / f32(SPP), ref_mean),
            "variance": ds.psnr(dv.denoise(A, B, feat0, feat1, F, half_spp=SPP // 2), ref_mean),
            "temporal": ds.psnr(t_mean, ref_mean),
            "temporal + variance": ds.psnr(dv.denoise(t_a, t_b, feat0, feat1, F, half_spp=1), ref_mean),
            "reprojected": ds.psnr(r_mean, ref_mean),
            "reprojected + variance": ds.psnr(dv.denoise(r_a, r_b, feat0, feat1, F, half_spp=1), ref_mean),
        }
        print(f"{W}x{H} {SPP} spp, {name}, N {N}, frame {last} (reprojected history valid on {100.0 * np.mean(n > 1):.1f} % "
              f"of the texels): " + ", ".join(f"{c} {got[c]:.2f} dB" for c in COLUMNS))
        got["same"] = all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in ((t_a, r_a), (t_b, r_b), (t_mean, r_mean)))
        done[name] = got
        return got
    return row


def test_static_scene_equals_the_in_place_stage(table):
    r = table("static")
    assert r["same"]
    assert r["reprojected"] == r["temporal"] and r["reprojected + variance"] == r["temporal + variance"]


def test_moving_objects(table):
    r = table("objects dt 0.2")
    assert r["reprojected + variance"] > r["variance"]


def test_slow_camera(table):
    r = table("camera s 0.05")
    assert r["reprojected"] > r["temporal"]
    assert r["reprojected + variance"] > r["variance"]


def test_fast_camera(table):
    r = table("camera s 0.2")
    assert r["reprojected"] > r["temporal"]
    assert r["reprojected + variance"] > r["temporal + variance"]
    assert r["reprojected + variance"] > r["variance"]


def test_fast_camera_and_moving_objects_is_measured(table):
    """No ordering of this row had 1.3 dB to spare in the prototype: it is printed with the others."""
    r = table("camera s 0.2, objects dt 0.2")
    assert all(np.isfinite(r[c]) for c in COLUMNS)
