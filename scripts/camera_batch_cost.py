#!/usr/bin/env python3
"""What a full wave of camera segments costs against a lane slot of the mixed segment loop
(step 0 of the camera-batch form), canonical scene, 1920x1080, hash stream.

  features  launches of F = 16 ... 256 feature samples (every lane always on a camera segment: the
            hash stream's camera ray, the walk, the gate, first-hit shading, the next sample), each
            the median of --launches launches between two stream events after three warm-up
            launches (scripts/denoise_quality.py's method); the least-squares slope is ms per
            sample of the frame, the intercept the launch's fixed cost.
  frame     the plain frame at 16 ... 256 spp the same way, with the unit loop (rt_debug_tune
            camera_batches = 0) unless --batches: its slope / segments per sample is the cost of
            one segment slot of that loop.

Prints one JSON line per measurement and the two fits.
  python scripts/camera_batch_cost.py [--launches 15] [--batches]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ray-tracing-gpu-vulkan_amd")]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=15)
    ap.add_argument("--batches", action="store_true", help="time the frames with the camera-batch form")
    args = ap.parse_args()

    import torch
    import rtvk

    if not torch.cuda.is_available():
        print("camera_batch_cost.py needs a GPU", file=sys.stderr)
        return 1

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(max(3, args.launches)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms), max(ms)

    W, H = 1920, 1080
    opt = rtvk.make_options(rng_mode=rtvk.HASH)
    z = lambda dt=torch.float32: torch.zeros((H, W, 4), dtype=dt, device="cuda")   # noqa: E731
    acc, f0, f1, out = z(), z(), z(), z(torch.uint8)
    with rtvk.Renderer(0) as r:
        r.set_scene(rtvk.generateRandomScene(0.0))
        xs, ys = [], []
        for F in (16, 32, 64, 128, 192, 256):
            rci = rtvk.canonical_render_call_info(F, W, H)
            med, lo, hi = timed(lambda: r.render_features(rci, f0, f1, samples=F, options=opt))
            print(json.dumps({"what": "features", "F": F, "median_ms": round(med, 4), "min_ms": round(lo, 4),
                              "max_ms": round(hi, 4)}), flush=True)
            xs.append(F)
            ys.append(med)
        k, c = np.polyfit(xs, ys, 1)
        print(json.dumps({"what": "features_fit", "slope_ms_per_sample": round(float(k), 6), "intercept_ms": round(float(c), 4)}),
              flush=True)
        if not args.batches:
            r.tune(camera_batches=0)
        xs, ys, sps = [], [], 1.0
        for spp in (16, 64, 128, 256):
            rci = rtvk.canonical_render_call_info(spp, W, H)
            med, lo, hi = timed(lambda: r.render_device(rci, acc, out, options=opt))
            torch.cuda.synchronize()
            st = r.stats()
            sps = st.segments / max(1, st.samples)
            print(json.dumps({"what": "frame", "spp": spp, "median_ms": round(med, 4), "min_ms": round(lo, 4),
                              "max_ms": round(hi, 4), "segments_per_sample": round(sps, 4),
                              "camera_batches": r.launch_info()["camera_batches"]}), flush=True)
            xs.append(spp)
            ys.append(med)
        k2, c2 = np.polyfit(xs, ys, 1)
        print(json.dumps({"what": "frame_fit", "slope_ms_per_sample": round(float(k2), 6), "intercept_ms": round(float(c2), 4),
                          "per_segment_slot_ms": round(float(k2) / sps, 6),
                          "features_slope_over_slot": round(float(k) / (float(k2) / sps), 4)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
