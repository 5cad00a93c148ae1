#!/usr/bin/env python3
"""Cost and quality of the hand-over of the two halves (adaptive and feedback frames
feeding the variance-guided filter and the temporal stage), canonical scene, after
scripts/temporal_quality.py.

  timing   at 1920x1080, in this one process:
           resolve   the resolve alone (Renderer.adaptive_resolve) without and with the halves and a
                     device-to-device copy of 36 B per texel (the bytes the halves add), the three
                     alternated, each the median of --launches launches between two stream events; the
                     bar is halves <= plain + copy;
           frame     feedback frames at BASELINE config 3's setting (cap 10 000, min = step = 512,
                     threshold 0.04, the set-up of scripts/feedback_probe.py), --frames of them queued
                     back to back from the adaptive frame's map, without and with the halves,
                     alternated twice.
  quality  at 480x270 (--width / --height), threshold 0.3, min = step = 4, cap 64, 16 feature samples,
           history 8, frame 7 of a static camera and of a camera step of 0.05: the feedback loop
           through the chain (features, motion, the reprojected temporal call on the halves with
           sample_count = half_count, the variance filter at half_spp 1) beside the uniform frames of
           the loop's mean samples per frame, rounded up to even, through the same chain; frame k of
           either renders from sample_base k x cap. PSNR (dB, on sqrt(clip(mean))) against the 1024-spp
           frame of the last camera at sample_base 1 << 20: the last frame noisy, through the variance
           filter alone, and through the temporal stage and the filter. No ordering is asserted.

Prints one JSON line per measurement.
  python scripts/feedback_denoise_quality.py [--skip-quality] [--skip-timing] [--launches 20] [--frames 12]
"""
import argparse
import ctypes
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ray-tracing-gpu-vulkan_amd")]

QUALITY_ROWS = (("static", 0.0), ("camera s 0.05", 0.05))


def psnr(mean, ref):
    a = np.sqrt(np.clip(mean.astype(np.float64), 0.0, 1.0))
    b = np.sqrt(np.clip(ref.astype(np.float64), 0.0, 1.0))
    return float(10.0 * np.log10(1.0 / np.mean((a - b) ** 2)))


def path_camera(rtvk, spp, W, H, s, k):
    """Frame k's RenderCallInfo on the camera path: (13 + s k, 11, -3 + 2 s k), looking at the origin."""
    rci = rtvk.canonical_render_call_info(spp, W, H)
    f32 = np.float32
    x, z = f32(13.0) + f32(s) * f32(k), f32(-3.0) + (f32(2.0) * f32(s)) * f32(k)
    rci.camera_pos.x, rci.camera_pos.z = float(x), float(z)
    rci.camera_dir.x, rci.camera_dir.y, rci.camera_dir.z = -float(x), -rci.camera_pos.y, -float(z)
    return rci


def timing(args, r, torch, rtvk) -> None:
    from rtvk import abi
    W, H = 1920, 1080
    texels = W * H
    f4 = lambda: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    words = lambda: torch.zeros((H, W), dtype=torch.int32, device="cuda")
    acc, acc_a, acc_b = f4(), f4(), f4()
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    cnt, half = words(), words()
    n_copy = 36 * texels
    src = torch.zeros(n_copy, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(n_copy, dtype=torch.uint8, device="cuda")
    hip = rtvk.load_library()      # dlsym on the library's handle finds the HIP runtime it is linked to
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def copy():
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), n_copy, 3, stream)      # hipMemcpyDeviceToDevice
        assert rc == 0, rc

    forms = (("resolve_plain", 120, lambda: r.adaptive_resolve(acc, out, 8, sample_count=cnt)),
             ("resolve_halves", 156, lambda: r.adaptive_resolve(acc, out, 8, sample_count=cnt, accum_a=acc_a, accum_b=acc_b,
                                                                half_count=half)),
             ("copy_36B_per_texel", 72, copy))
    for _ in range(3):
        for _, _, fn in forms:
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in forms}
    for _ in range(max(10, args.launches)):     # the three forms alternated
        for name, _, fn in forms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    med = {}
    for name, per_texel, _ in forms:
        med[name] = statistics.median(ms[name])
        print(json.dumps({"what": "resolve_timing", "name": name, "width": W, "height": H, "launches": len(ms[name]),
                          "median_ms": round(med[name], 4), "min_ms": round(min(ms[name]), 4),
                          "max_ms": round(max(ms[name]), 4), "bytes_per_texel": per_texel,
                          "tb_per_s": round(per_texel * texels / med[name] / 1e9, 3)}), flush=True)
    bar = med["resolve_plain"] + med["copy_36B_per_texel"]
    print(json.dumps({"what": "resolve_bar", "halves_ms": round(med["resolve_halves"], 4),
                      "plain_plus_copy_ms": round(bar, 4), "halves_over_plain": round(med["resolve_halves"] / med["resolve_plain"], 3),
                      "bytes_ratio": round(156 / 120, 3), "met": bool(med["resolve_halves"] <= bar)}), flush=True)

    # feedback frames at config 3's setting, without and with the halves
    cap, mn, thr = 10000, 512, 0.04
    opt = rtvk.make_options(rng_mode=rtvk.HASH)
    rci = rtvk.canonical_render_call_info(cap, W, H)
    ad, fb = rtvk.make_adaptive(thr, mn, mn), rtvk.make_feedback(thr, mn, cap)
    r.set_scene(rtvk.generateRandomScene(0.0))
    with r.sample_map(W, H) as smap:
        smap.schedule(abi.SAMPLE_MAP_ONE_LAUNCH)

        def start():
            r.render_adaptive(rci, acc, out, options=opt, adaptive=ad)
            return smap.set_from_adaptive(0)

        start()
        r.render_sample_map_feedback(rci, acc, out, smap, fb, options=opt)   # warm-up: the planner's buffers
        for run in range(2):
            for with_halves in (False, True):
                mi = start()
                kw = dict(accum_a=acc_a, accum_b=acc_b, half_count=half) if with_halves else {}
                waits = r.host_waits()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.frames):
                    r.render_sample_map_feedback(rci, acc, out, smap, fb, sample_count=cnt, options=opt, **kw)
                queued = time.perf_counter() - t0
                torch.cuda.synchronize()
                total = time.perf_counter() - t0
                print(json.dumps({"what": "feedback_frames", "halves": with_halves, "run": run, "threshold": thr, "min": mn,
                                  "cap": cap, "frames": args.frames, "ms_per_frame": round(total * 1e3 / args.frames, 2),
                                  "host_ms_to_queue_all": round(queued * 1e3, 2), "host_waits": r.host_waits() - waits,
                                  "start_mean_spp": round(mi.samples / texels, 1),
                                  "last_frame_mean_spp": round(float(cnt.double().mean().item()), 1)}), flush=True)


def quality(args, r, torch, rtvk) -> None:
    from rtvk import abi
    W, H, F, N, last, ref_spp = args.width, args.height, 16, 8, 7, 1024
    thr, mn, cap = 0.3, 4, 64
    f4 = lambda: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    acc, acc_a, acc_b, f0, f1, mv, out_a, out_b, mean = (f4() for _ in range(9))
    out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    scratch = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    half = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    hlen = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    params = rtvk.make_temporal(max_history=N)
    fb = rtvk.make_feedback(thr, mn, cap)
    r.set_scene(rtvk.generateRandomScene(0.0))

    def filtered(a, b, **kw):
        r.denoise_variance(a, b, f0, f1, F, out, out_mean=mean, **kw)
        torch.cuda.synchronize()
        return mean.cpu().numpy()[..., :3]

    for name, s in QUALITY_ROWS:
        r.render_device(path_camera(rtvk, ref_spp, W, H, s, last), mean, out,
                        options=rtvk.make_options(rng_mode=rtvk.HASH, sample_base=1 << 20))
        torch.cuda.synchronize()
        ref = mean.cpu().numpy()[..., :3] / np.float32(ref_spp)
        rec = {"what": "feedback_denoise_quality", "row": name, "width": W, "height": H, "threshold": thr, "min": mn,
               "cap": cap, "feature_samples": F, "max_history": N, "frame": last, "camera_step": s, "ref_spp": ref_spp}

        def stage(T, M, rci, **kw):
            r.render_features(rci, f0, f1, samples=F)
            r.render_motion(M, rci, mv)
            M.keep_current(rci)
            r.temporal_reproject(T, acc_a, f0, f1, F, mv, out_a, accum_b=acc_b, out_b=out_b, history_len=hlen, params=params,
                                 **kw)

        # the feedback loop
        spp_sum = 0.0
        with r.sample_map(W, H) as smap, r.temporal(W, H) as T, r.motion(W, H) as M:
            smap.schedule(abi.SAMPLE_MAP_ONE_LAUNCH)
            for k in range(last + 1):
                rci = path_camera(rtvk, cap, W, H, s, k)
                opt = rtvk.make_options(rng_mode=rtvk.HASH, sample_base=k * cap)
                kw = dict(sample_count=cnt, options=opt, accum_a=acc_a, accum_b=acc_b, half_count=half)
                if k == 0:
                    r.render_adaptive(rci, acc, scratch, adaptive=rtvk.make_adaptive(thr, mn, mn), **kw)
                else:
                    if k == 1:
                        smap.set_from_adaptive(0)
                    r.render_sample_map_feedback(rci, acc, scratch, smap, fb, **kw)
                stage(T, M, rci, sample_count=half)
                spp_sum += float(cnt.double().mean().item())
            torch.cuda.synchronize()
            n = cnt.cpu().numpy().astype(np.float32)[..., None]
            rec["feedback_mean_spp_per_frame"] = round(spp_sum / (last + 1), 2)
            rec["feedback_last_frame_mean_spp"] = round(float(n.mean()), 2)
            rec["feedback_history_valid_share"] = round(float((hlen > 1).float().mean().item()), 4)
            rec["feedback_psnr_noisy_db"] = round(psnr(acc.cpu().numpy()[..., :3] / np.maximum(n, 1), ref), 2)
            rec["feedback_psnr_variance_db"] = round(psnr(filtered(acc_a, acc_b, half_count=half), ref), 2)
            rec["feedback_psnr_temporal_variance_db"] = round(psnr(filtered(out_a, out_b, half_spp=1), ref), 2)
        # uniform frames of the same mean samples, rounded up to even
        u = max(2, (int(np.ceil(spp_sum / (last + 1))) + 1) & ~1)
        with r.temporal(W, H) as T, r.motion(W, H) as M:
            for k in range(last + 1):
                rci = path_camera(rtvk, u, W, H, s, k)
                r.render_halves(rci, acc_a, acc_b, scratch, options=rtvk.make_options(rng_mode=rtvk.HASH, sample_base=k * cap))
                stage(T, M, rci, spp=u // 2)
            torch.cuda.synchronize()
            rec["uniform_spp"] = u
            rec["uniform_history_valid_share"] = round(float((hlen > 1).float().mean().item()), 4)
            rec["uniform_psnr_noisy_db"] = round(psnr((acc_a + acc_b).cpu().numpy()[..., :3] / np.float32(u), ref), 2)
            rec["uniform_psnr_variance_db"] = round(psnr(filtered(acc_a, acc_b, half_spp=u // 2), ref), 2)
            rec["uniform_psnr_temporal_variance_db"] = round(psnr(filtered(out_a, out_b, half_spp=1), ref), 2)
        print(json.dumps(rec), flush=True)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    args = ap.parse_args()

    import torch
    import rtvk

    if not torch.cuda.is_available():
        print("feedback_denoise_quality.py needs a GPU", file=sys.stderr)
        return 1
    with rtvk.Renderer(0) as r:
        if not args.skip_quality:
            quality(args, r, torch, rtvk)
        if not args.skip_timing:
            timing(args, r, torch, rtvk)
    return 0


if __name__ == "__main__":
    sys.exit(main())
