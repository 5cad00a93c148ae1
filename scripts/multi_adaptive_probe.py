#!/usr/bin/env python3
"""Adaptive frames through rt_multi at BASELINE config 3's geometry (1920x1080, canonical scene,
cap 10 000 spp, min = step = 512: scripts/adaptive_probe.py's setup). One measurement per process,
so that runs of several libraries can alternate on one machine:

  --mode device    rt_render_adaptive_device on one context (--lib: another build of the library,
                   e.g. the commit before rt_multi_render_adaptive, which has this mode only)
  --mode multi     rt_multi_render_adaptive over --devices logical devices on GPU 0 (1: the direct path)
  --mode deal      one threshold-0.04 frame over --devices logical devices: each device's sample
                   count, the imbalance the static tile-row deal leaves

Prints one JSON line per threshold: frame times of --repeat frames (the best is the figure), passes,
mean spp. Not a bench leg (bench.py measures the headline).
  python scripts/multi_adaptive_probe.py --mode multi --devices 2 [--thresholds 0.04,0]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ray-tracing-gpu-vulkan_amd")]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["device", "multi", "deal"], required=True)
    ap.add_argument("--devices", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=10000, help="the cap (max_spp)")
    ap.add_argument("--min", type=int, default=512)
    ap.add_argument("--step", type=int, default=512)
    ap.add_argument("--thresholds", default="0.04,0")
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--label", default="")
    ap.add_argument("--lib", default=None, help="another build of librt_mi355x.so to measure (--mode device)")
    args = ap.parse_args()

    import torch
    import rtvk
    from rtvk import abi

    if args.lib:   # an older build of the same ABI (it may predate the multi-device entry points)
        abi._lib = abi.load_library(args.lib)
    W, H, cap = args.width, args.height, args.spp
    lib_sha = abi.build_info().get("sources_sha256")
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
    opt = rtvk.make_options(rng_mode=rtvk.HASH)
    rci = rtvk.canonical_render_call_info(cap, W, H)
    scene = rtvk.generateRandomScene(0.0, 11)

    if args.mode == "device":
        r = rtvk.Renderer(0)
        r.set_scene(scene)
    else:
        r = rtvk.MultiRenderer(args.devices, logical=args.devices > 1)
        r.set_scene(scene)

    def frame(thr):
        return r.render_adaptive(rci, acc, out, sample_count=cnt, options=opt,
                                 adaptive=rtvk.make_adaptive(thr, args.min, args.step))

    frame(16.0)   # warm-up: kernels loaded, buffers allocated
    torch.cuda.synchronize()
    if args.mode == "deal":
        info = frame(0.04)
        torch.cuda.synchronize()
        devs = [r.adaptive_device_info(d) for d in range(args.devices)]
        samples = [int(d.samples) for d in devs]
        print(json.dumps({"what": "deal", "lib": lib_sha, "devices": args.devices, "threshold": 0.04,
                          "samples": samples, "passes": [int(d.passes) for d in devs],
                          "tiles": [int(d.tiles) for d in devs], "total": int(info.samples),
                          "max_over_mean": round(max(samples) * len(samples) / max(1, sum(samples)), 4)}), flush=True)
        r.close()
        return 0
    for thr in [float(t) for t in args.thresholds.split(",") if t]:
        ms = []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = frame(thr)
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        print(json.dumps({"what": args.label or args.mode, "lib": lib_sha, "mode": args.mode, "devices": args.devices,
                          "threshold": thr, "frame_ms": ms, "best_ms": min(ms), "passes": int(info.passes),
                          "mean_spp": round(info.samples / (W * H), 1)}), flush=True)
    r.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
