#!/usr/bin/env python3
"""Adaptive frames at BASELINE config 3's geometry (1920x1080, canonical scene, cap 10 000 spp):

  1. pass overhead: the adaptive frame at threshold 0 (every tile runs every pass: the same samples
     as the uniform frame) against rt_render_device at the cap from the same library, with the
     per-half-pass trace-kernel times (rt_launch_ms);
  2. what adaptivity buys: frame time, mean spp, capped tiles and PSNR of the rgba8 frame against
     the uniform frame at the cap, for a few thresholds.

Prints one JSON line per measurement. Not a bench leg (bench.py measures the headline).
  python scripts/adaptive_probe.py [--spp 10000] [--min 512] [--step 512] [--thresholds 0.01,0.02,0.04,0.08]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ray-tracing-gpu-vulkan_amd")]


def psnr(a, b) -> float:
    mse = float(np.mean((a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)) ** 2))
    return float("inf") if mse == 0 else round(10.0 * np.log10(255.0 ** 2 / mse), 2)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=10000, help="the cap (max_spp)")
    ap.add_argument("--min", type=int, default=512)
    ap.add_argument("--step", type=int, default=512)
    ap.add_argument("--thresholds", default="0.01,0.02,0.04,0.08")
    ap.add_argument("--repeat", type=int, default=2, help="timed frames per measurement (the best is reported too)")
    args = ap.parse_args()

    import torch
    import rtvk
    from rtvk import abi

    W, H, cap = args.width, args.height, args.spp
    lib_sha = abi.build_info().get("sources_sha256")
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    opt = rtvk.make_options(rng_mode=rtvk.HASH)
    rci = rtvk.canonical_render_call_info(cap, W, H)

    def timed(fn):
        ms = []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return r, ms

    with rtvk.Renderer(0) as r:
        r.set_scene(rtvk.generateRandomScene(0.0, 11))
        for _ in range(2):   # warm-up: kernels loaded, the uniform launch has its tile order
            r.render_device(rci, acc, out, options=opt)
        torch.cuda.synchronize()
        _, uni_ms = timed(lambda: r.render_device(rci, acc, out, options=opt))
        uni_kernel = r.launch_ms(0)
        ref = out.cpu().numpy()
        ref_acc = acc.cpu().numpy()
        print(json.dumps({"what": "uniform", "lib": lib_sha, "spp": cap, "frame_ms": [round(m, 2) for m in uni_ms],
                          "trace_kernel_ms": round(uni_kernel, 2)}), flush=True)

        def adaptive(thr):
            return r.render_adaptive(rci, acc, out, sample_count=cnt, options=opt,
                                     adaptive=rtvk.make_adaptive(thr, args.min, args.step))

        adaptive(16.0)   # warm-up of the adaptive kernels and buffers
        info, ms = timed(lambda: adaptive(0.0))
        halves = [round(r.launch_ms(b), 3) for b in range(min(64, 2 * info.passes) - 1, -1, -1)]
        same = bool(np.array_equal(out.cpu().numpy(), ref) and np.array_equal(acc.cpu().numpy(), ref_acc))
        print(json.dumps({"what": "threshold 0", "lib": lib_sha, "min": args.min, "step": args.step,
                          "passes": info.passes, "frame_ms": [round(m, 2) for m in ms],
                          "ratio_to_uniform": round(min(ms) / min(uni_ms), 4),
                          "half_pass_trace_kernel_ms": halves, "sum_half_pass_ms": round(sum(halves), 2),
                          # the launch times are the last frame's
                          "frame_minus_trace_kernels_ms": round(ms[-1] - sum(halves), 2),
                          "equals_uniform_frame": same}), flush=True)
        for thr in [float(t) for t in args.thresholds.split(",") if t]:
            info, ms = timed(lambda: adaptive(thr))
            print(json.dumps({"what": "adaptive", "lib": lib_sha, "threshold": thr, "min": args.min,
                              "step": args.step, "cap": cap, "passes": info.passes,
                              "frame_ms": [round(m, 2) for m in ms],
                              "speedup_vs_uniform": round(min(uni_ms) / min(ms), 3),
                              "mean_spp": round(info.samples / (W * H), 1), "tiles": info.tiles,
                              "tiles_capped": info.tiles_capped,
                              "psnr_db_vs_uniform_cap": psnr(out.cpu().numpy(), ref)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
