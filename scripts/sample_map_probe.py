#!/usr/bin/env python3
"""Sample-map frames at BASELINE config 3's geometry (1920x1080, canonical scene,
cap 10 000 spp, min = step = 512), per threshold:

  adaptive     rt_render_adaptive_device (the pass loop);
  replay       rt_render_sample_map_device replaying that frame's counts (set_from_adaptive, quantum 0),
               with the per-level trace-kernel times (rt_launch_ms);
  replay_q     the same at --quantum (fewer levels, more samples);
  replay_one   the replay under the one-launch schedule (RT_SAMPLE_MAP_ONE_LAUNCH), once per unit
               length of --units (0: automatic), with the launch's kernel time and its t_dry / t_last
               tail; asserted to be the level replay's image bit for bit;
  uniform      rt_render_device at the adaptive frame's mean spp, rounded up to even: the frame of the
               same cost;
  and the PSNR of each rgba8 frame against the uniform frame at the cap (skipped with --no-psnr).

--lib PATH loads another build of the library (e.g. the parent commit's, for the adaptive leg's A/B);
a build without the sample-map entry points measures the adaptive leg only. Prints one JSON line per
measurement; every time is the list of --repeat frames, host clock around a synchronised frame.
  python scripts/sample_map_probe.py [--thresholds 0.04,0.02] [--quantum 2048] [--units 0,32,64,128,256]
                                     [--lib PATH] [--no-psnr]
"""
import argparse
import ctypes
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
    ap.add_argument("--thresholds", default="0.04,0.02")
    ap.add_argument("--quantum", type=int, default=2048)
    ap.add_argument("--units", default="0,32,64,128,256", help="unit lengths of the one-launch replay (0: automatic)")
    ap.add_argument("--repeat", type=int, default=2, help="timed frames per measurement")
    ap.add_argument("--lib", default=None, help="another build of librt_mi355x.so")
    ap.add_argument("--no-psnr", action="store_true", help="skip the uniform frame at the cap and the PSNRs")
    args = ap.parse_args()

    import torch
    import rtvk
    from rtvk import abi

    if args.lib:
        abi._lib = abi.load_library(args.lib)
    has_maps = hasattr(abi.load_library(), "rt_render_sample_map_device")
    has_one = hasattr(abi.load_library(), "rt_sample_map_set_schedule")
    W, H, cap = args.width, args.height, args.spp
    lib_sha = abi.build_info().get("sources_sha256")
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    opt = rtvk.make_options(rng_mode=rtvk.HASH)
    rci = rtvk.canonical_render_call_info(cap, W, H)

    def timed(fn):
        ms = []
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
        return r, ms

    with rtvk.Renderer(0) as r:
        r.set_scene(rtvk.generateRandomScene(0.0, 11))
        ref = None
        if not args.no_psnr:
            r.render_device(rci, acc, out, options=opt)
            torch.cuda.synchronize()
            ref = out.cpu().numpy()
        r.render_adaptive(rci, acc, out, options=opt, adaptive=rtvk.make_adaptive(16.0, args.min, args.step))   # warm-up
        smap = r.sample_map(W, H) if has_maps else None
        for thr in [float(t) for t in args.thresholds.split(",") if t]:
            base = {"lib": lib_sha, "threshold": thr, "min": args.min, "step": args.step, "cap": cap}
            ad = rtvk.make_adaptive(thr, args.min, args.step)
            info, ms = timed(lambda: r.render_adaptive(rci, acc, out, options=opt, adaptive=ad))
            mean_spp = info.samples / (W * H)
            print(json.dumps({"what": "adaptive", **base, "frame_ms": ms, "passes": info.passes,
                              "trace_launches": 2 * info.passes, "mean_spp": round(mean_spp, 1),
                              "tiles_capped": info.tiles_capped,
                              "psnr_db": None if ref is None else psnr(out.cpu().numpy(), ref)}), flush=True)
            if smap is None:
                continue
            for name, quantum in (("replay", 0), ("replay_q", args.quantum)):
                mi = smap.set_from_adaptive(quantum)
                # the frame's cap covers the map: a quantum may round the adaptive cap up
                rci_m = rtvk.canonical_render_call_info(max(cap, mi.max_count), W, H)
                r.render_sample_map(rci_m, acc, out, smap, options=opt)   # warm-up of this map's launch sizes
                _, ms = timed(lambda: r.render_sample_map(rci_m, acc, out, smap, options=opt))
                levels = [round(r.launch_ms(b), 3) for b in range(mi.levels - 1, -1, -1)]
                plan = smap.debug_plan()
                print(json.dumps({"what": name, **base, "quantum": quantum, "frame_ms": ms, "levels": mi.levels,
                                  "mean_spp": round(mi.samples / (W * H), 1), "tile_launches": mi.tile_launches,
                                  "level_counts": plan["levels"].tolist(), "level_tiles": plan["level_tiles"].tolist(),
                                  "level_trace_kernel_ms": levels, "sum_level_ms": round(sum(levels), 2),
                                  "frame_minus_trace_kernels_ms": round(ms[-1] - sum(levels), 2),
                                  "psnr_db": None if ref is None else psnr(out.cpu().numpy(), ref)}), flush=True)
                if name == "replay":
                    level_acc, level_out = acc.clone(), out.clone()
            for unit in [int(u) for u in args.units.split(",") if u] if has_one else []:
                smap.schedule(abi.SAMPLE_MAP_ONE_LAUNCH, unit)
                mi = smap.set_from_adaptive(0)
                sched = smap.schedule_info()
                r.render_sample_map(rci, acc, out, smap, options=opt)   # warm-up
                _, ms = timed(lambda: r.render_sample_map(rci, acc, out, smap, options=opt))
                assert torch.equal(acc, level_acc) and torch.equal(out, level_out), "one-launch replay differs from the level replay"
                h = (ctypes.c_uint64 * 68)()   # the last launch's realtime stamps, 100 MHz (scripts/tail_ab.py)
                abi.check(abi.load_library().rt_debug_lane_hist(r._ctx, h))
                kt = {"queue_dry_ms": round((h[66] - h[65]) / 1e5, 2), "tail_ms": round((h[67] - h[66]) / 1e5, 2)}
                print(json.dumps({"what": "replay_one", **base, "unit_samples": unit, "unit_samples_used": sched["unit_samples"],
                                  "n_blocks": sched["n_blocks"], "frame_ms": ms, "levels": mi.levels,
                                  "mean_spp": round(mi.samples / (W * H), 1), "tiles": mi.tile_launches,
                                  "trace_kernel_ms": round(r.launch_ms(0), 3), **kt,
                                  "same_image_as_replay": True}), flush=True)
            if has_one:
                smap.schedule(abi.SAMPLE_MAP_LEVELS)
            even = int(np.ceil(mean_spp / 2.0)) * 2
            rci_u = rtvk.canonical_render_call_info(even, W, H)
            r.render_device(rci_u, acc, out, options=opt)   # warm-up: the tile order of this launch
            _, ms = timed(lambda: r.render_device(rci_u, acc, out, options=opt))
            print(json.dumps({"what": "uniform", **base, "spp": even, "frame_ms": ms,
                              "trace_kernel_ms": round(r.launch_ms(0), 2),
                              "psnr_db": None if ref is None else psnr(out.cpu().numpy(), ref)}), flush=True)
        if smap is not None:
            smap.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
