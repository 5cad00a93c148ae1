#!/usr/bin/env python3
"""Feedback frames at BASELINE config 3's geometry (1920x1080, canonical scene, cap
10 000 spp, min = step = 512), per threshold: an adaptive frame, its counts set as the map, then

  replay_one   the one-launch replay of that map (the frame a feedback frame is compared with);
  feedback     --frames feedback frames queued back to back, one host wait at the end: ms per frame,
               and per frame (from a second, synchronised pass over the same start) the two trace
               launches' kernel times, the mean spp it rendered and the tiles its update raised and
               lowered.

--lib PATH loads another build of the library (the replay only, for a build without feedback frames).
Prints one JSON line per measurement.
  python scripts/feedback_probe.py [--thresholds 0.04] [--frames 12] [--animate] [--lib PATH]
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
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=10000, help="the cap (max_spp)")
    ap.add_argument("--min", type=int, default=512)
    ap.add_argument("--step", type=int, default=512)
    ap.add_argument("--thresholds", default="0.04")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--animate", action="store_true", help="scene time advances 0.1 s per frame")
    ap.add_argument("--lib", default=None, help="another build of librt_mi355x.so")
    args = ap.parse_args()

    import torch
    import rtvk
    from rtvk import abi

    if args.lib:
        abi._lib = abi.load_library(args.lib)
    has_feedback = hasattr(abi.load_library(), "rt_render_sample_map_feedback_device")
    W, H, cap = args.width, args.height, args.spp
    lib_sha = abi.build_info().get("sources_sha256")
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    opt = rtvk.make_options(rng_mode=rtvk.HASH)
    rci = rtvk.canonical_render_call_info(cap, W, H)
    scenes = [rtvk.generateRandomScene(0.1 * i if args.animate else 0.0, 11) for i in range(args.frames)]

    with rtvk.Renderer(0) as r:
        r.set_scene(scenes[0])
        r.render_adaptive(rci, acc, out, options=opt, adaptive=rtvk.make_adaptive(16.0, args.min, args.step))   # warm-up
        for thr in [float(t) for t in args.thresholds.split(",") if t]:
            base = {"lib": lib_sha, "threshold": thr, "min": args.min, "cap": cap, "animate": args.animate}
            ad = rtvk.make_adaptive(thr, args.min, args.step)
            with r.sample_map(W, H) as smap:
                smap.schedule(abi.SAMPLE_MAP_ONE_LAUNCH)

                def start():
                    r.set_scene(scenes[0])
                    r.render_adaptive(rci, acc, out, options=opt, adaptive=ad)
                    return smap.set_from_adaptive(0)

                mi = start()
                r.render_sample_map(rci, acc, out, smap, options=opt)   # warm-up
                ms = []
                for _ in range(2):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r.render_sample_map(rci, acc, out, smap, options=opt)
                    torch.cuda.synchronize()
                    ms.append(round((time.perf_counter() - t0) * 1e3, 2))
                print(json.dumps({"what": "replay_one", **base, "frame_ms": ms, "trace_kernel_ms": round(r.launch_ms(0), 3),
                                  "mean_spp": round(mi.samples / (W * H), 1)}), flush=True)
                if not has_feedback:
                    continue
                fb = rtvk.make_feedback(thr, args.min, cap)
                r.render_sample_map_feedback(rci, acc, out, smap, fb, options=opt)   # warm-up: the planner's buffers
                start()
                waits = r.host_waits()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(args.frames):
                    if args.animate:
                        r.set_scene(scenes[i])
                    r.render_sample_map_feedback(rci, acc, out, smap, fb, options=opt)
                queued = time.perf_counter() - t0
                torch.cuda.synchronize()
                total = time.perf_counter() - t0
                print(json.dumps({"what": "feedback_loop", **base, "frames": args.frames,
                                  "ms_per_frame": round(total * 1e3 / args.frames, 2),
                                  "host_ms_to_queue_all": round(queued * 1e3, 2),
                                  "host_waits": r.host_waits() - waits}), flush=True)
                # the same frames again, one at a time, for what each did
                mi = start()
                spp = mi.samples / (W * H)
                moved = smap.debug_feedback()   # (the counters run over the map's life)
                up, down = moved["raised"], moved["lowered"]
                for i in range(args.frames):
                    if args.animate:
                        r.set_scene(scenes[i])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    r.render_sample_map_feedback(rci, acc, out, smap, fb, options=opt)
                    torch.cuda.synchronize()
                    frame_ms = (time.perf_counter() - t0) * 1e3
                    moved = smap.debug_feedback()
                    info = smap.info
                    print(json.dumps({"what": "feedback_frame", **base, "frame": i, "frame_ms": round(frame_ms, 2),
                                      "trace_kernel_ms": [round(r.launch_ms(1), 3), round(r.launch_ms(0), 3)],
                                      "rendered_mean_spp": round(spp, 1), "raised": moved["raised"] - up,
                                      "lowered": moved["lowered"] - down, **smap.schedule_info()}), flush=True)
                    up, down = moved["raised"], moved["lowered"]
                    spp = info.samples / (W * H)
    return 0


if __name__ == "__main__":
    sys.exit(main())
