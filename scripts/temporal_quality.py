#!/usr/bin/env python3
"""Quality and cost of the temporal stage, canonical scene, counter-based stream,
after scripts/denoise_variance_quality.py.

  quality  at 480x270 (--width / --height), 4 spp, 16 feature samples, the three rows of the CPU
           prototype (tests/test_temporal_quality.py): a static scene with a history cap of 32 at
           frame 5, scene time steps of 0.05 and 0.2 per frame with a cap of 8 at frames 9 and 7.
           Frame k is rendered as two halves at sample_base 4 k and 4 k + 2, the features at
           sample_base 0, the reference is the 1024-spp frame of the same scene time at sample_base
           1 << 20. PSNR (dB, on sqrt(clip(mean))) of the last frame: noisy, the plain and the
           variance-guided filter on that frame alone, the temporal stage alone, and the temporal
           stage ahead of either filter; and the share of texels whose history was valid.
  timing   at 1920x1080, each the median of --launches launches after warm-up between two stream
           events, with min and max, all in this one process: the temporal call with one accumulator
           and with two (every optional output and a sample-count plane given); a device-to-device
           hipMemcpyAsync that moves the same bytes (half of them read, half written) as each; the
           8-spp chain of two 4-spp halves, features and the variance filter (2, 3), with and
           without the temporal call in between.

  --reproject  runs the reprojection's measurements instead ("Reprojection"):
           quality, the five rows of tests/test_temporal_reproject_quality.py at 480x270: frame k's
           camera at (13 + s k, 11, -3 + 2 s k) looking at the origin, scene time k dt, the in-place
           and the reprojected stage side by side on the same frames, each alone and ahead of the
           variance filter;
           timing at 1920x1080 as above: the motion pass's three launches against the feature pass
           at F = 1 (one primary ray per texel each), the reprojected call with one and two
           accumulators on the motion plane of a camera step of 0.05 against the in-place call and
           the copy of the bytes it moves (the in-place call's plus 16 B of motion per texel), and
           the 8-spp chain with the in-place stage and with motion, keep_current and the reprojected
           stage.

Prints one JSON line per measurement.
  python scripts/temporal_quality.py [--reproject] [--skip-quality] [--skip-timing] [--launches 20]
"""
import argparse
import ctypes
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ray-tracing-gpu-vulkan_amd"), str(ROOT / "tests")]

ROWS = (("static", 0.0, 32, 5), ("dt 0.05", 0.05, 8, 9), ("dt 0.2", 0.2, 8, 7))


def psnr(mean, ref):
    a = np.sqrt(np.clip(mean.astype(np.float64), 0.0, 1.0))
    b = np.sqrt(np.clip(ref.astype(np.float64), 0.0, 1.0))
    return float(10.0 * np.log10(1.0 / np.mean((a - b) ** 2)))


REPROJECT_ROWS = (("static", 0.0, 0.0, 32, 5), ("objects dt 0.2", 0.0, 0.2, 8, 7), ("camera s 0.05", 0.05, 0.0, 8, 7),
                  ("camera s 0.2", 0.2, 0.0, 8, 7), ("camera s 0.2, objects dt 0.2", 0.2, 0.2, 8, 7))


def path_camera(rtvk, spp, W, H, s, k):
    """Frame k's RenderCallInfo on the camera path: (13 + s k, 11, -3 + 2 s k), looking at the origin."""
    rci = rtvk.canonical_render_call_info(spp, W, H)
    f32 = np.float32
    x, z = f32(13.0) + f32(s) * f32(k), f32(-3.0) + (f32(2.0) * f32(s)) * f32(k)
    rci.camera_pos.x, rci.camera_pos.z = float(x), float(z)
    rci.camera_dir.x, rci.camera_dir.y, rci.camera_dir.z = -float(x), -rci.camera_pos.y, -float(z)
    return rci


def reproject_measurements(args, r, torch, rtvk) -> int:
    def f4(W, H):
        return torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")

    def u8(W, H):
        return torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")

    def hash_options(base=0):
        return rtvk.make_options(rng_mode=rtvk.HASH, sample_base=base)

    if not args.skip_quality:
        W, H, spp, ref_spp, F = args.width, args.height, 4, 1024, 16
        acc_a, acc_b, f0, f1, mv, t_a, t_b, r_a, r_b, mean = (f4(W, H) for _ in range(10))
        out, scratch = u8(W, H), u8(W, H)
        hlen = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        for name, s, dt, N, last in REPROJECT_ROWS:
            params = rtvk.make_temporal(max_history=N)
            with r.temporal(W, H) as here, r.temporal(W, H) as moved, r.motion(W, H) as M:
                for k in range(last + 1):
                    rci = path_camera(rtvk, spp, W, H, s, k)
                    r.set_scene(rtvk.generateRandomScene(float(np.float32(k * dt))))
                    r.render_halves(rci, acc_a, acc_b, scratch, options=hash_options(spp * k))
                    r.render_features(rci, f0, f1, samples=F, options=hash_options())
                    r.render_motion(M, rci, mv)
                    M.keep_current(rci)
                    r.temporal_accumulate(here, acc_a, f0, f1, F, t_a, accum_b=acc_b, out_b=t_b, spp=spp // 2, params=params)
                    r.temporal_reproject(moved, acc_a, f0, f1, F, mv, r_a, accum_b=acc_b, out_b=r_b, history_len=hlen,
                                         spp=spp // 2, params=params)
                r.render_device(path_camera(rtvk, ref_spp, W, H, s, last), mean, out, options=hash_options(1 << 20))
                torch.cuda.synchronize()
                ref = mean.cpu().numpy()[..., :3] / np.float32(ref_spp)

                def filtered(a, b, half_spp):
                    r.denoise_variance(a, b, f0, f1, F, out, half_spp=half_spp, out_mean=mean)
                    torch.cuda.synchronize()
                    return round(psnr(mean.cpu().numpy()[..., :3], ref), 2)
                rec = {"what": "reproject_quality", "row": name, "width": W, "height": H, "spp": spp, "feature_samples": F,
                       "ref_spp": ref_spp, "camera_step": s, "dt": dt, "max_history": N, "frame": last,
                       "history_valid_share": round(float((hlen > 1).float().mean().item()), 4),
                       "motion_ok_share": round(float((mv[..., 3] > 0).float().mean().item()), 4),
                       "psnr_noisy_db": round(psnr((acc_a + acc_b).cpu().numpy()[..., :3] / np.float32(spp), ref), 2),
                       "psnr_temporal_db": round(psnr(((t_a + t_b) * 0.5).cpu().numpy()[..., :3], ref), 2),
                       "psnr_reprojected_db": round(psnr(((r_a + r_b) * 0.5).cpu().numpy()[..., :3], ref), 2),
                       "static_equal": bool(torch.equal(t_a, r_a) and torch.equal(t_b, r_b))}
                rec["psnr_variance_db"] = filtered(acc_a, acc_b, spp // 2)
                rec["psnr_temporal_variance_db"] = filtered(t_a, t_b, 1)
                rec["psnr_reprojected_variance_db"] = filtered(r_a, r_b, 1)
                print(json.dumps(rec), flush=True)
    if not args.skip_timing:
        W, H, spp, F = 1920, 1080, 8, 16
        texels = W * H
        r.set_scene(rtvk.generateRandomScene(0.0))
        acc_a, acc_b, f0, f1, mv, out_a, out_b, mean = (f4(W, H) for _ in range(8))
        out, scratch = u8(W, H), u8(W, H)
        hlen = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        counts = torch.full((H, W), spp // 2, dtype=torch.int32, device="cuda")
        rci0, rci = path_camera(rtvk, spp, W, H, 0.05, 0), path_camera(rtvk, spp, W, H, 0.05, 1)
        r.render_halves(rci, acc_a, acc_b, scratch, options=hash_options())
        r.render_features(rci, f0, f1, samples=F, options=hash_options())
        torch.cuda.synchronize()

        def timed(name, fn, **extra):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(max(10, args.launches)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ms.append(a.elapsed_time(b))
            rec = {"what": "reproject_timing", "name": name, "width": W, "height": H, "launches": len(ms),
                   "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
            rec.update(extra)
            print(json.dumps(rec), flush=True)
            return statistics.median(ms)

        hip = rtvk.load_library()      # dlsym on the library's handle finds the HIP runtime it is linked to
        hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
        hip.hipMemcpyAsync.restype = ctypes.c_int
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def copy_of(moved):
            n = moved // 2
            src = torch.zeros(n, dtype=torch.uint8, device="cuda")
            dst = torch.zeros(n, dtype=torch.uint8, device="cuda")

            def fn():
                rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), n, 3, stream)      # hipMemcpyDeviceToDevice
                assert rc == 0, rc
            fn.keep = (src, dst)
            return fn

        with r.temporal(W, H) as T, r.motion(W, H) as M:
            # one primary ray per texel each
            M.set_previous(rtvk.generateRandomScene(0.0), rci0)
            t_m = timed("motion_pass", lambda: r.render_motion(M, rci, mv))
            t_f = timed("features_F1", lambda: r.render_features(rci, f0, f1, samples=1, options=hash_options()))
            cx = torch.arange(W, device="cuda", dtype=torch.float32)[None, :] + 0.5
            cy = torch.arange(H, device="cuda", dtype=torch.float32)[:, None] + 0.5
            four_taps = ((mv[..., 0] - cx).abs() > 2.0 ** -6) | ((mv[..., 1] - cy).abs() > 2.0 ** -6)
            print(json.dumps({"what": "ratio", "name": "motion_pass", "motion_over_features_F1": round(t_m / t_f, 3),
                              "texels_off_their_centre_share": round(float(four_taps.float().mean().item()), 4)}), flush=True)
            r.render_features(rci, f0, f1, samples=F, options=hash_options())
            for name, per_texel, two in (("one", 16 * 3 + 4 + 32 + 32 + 16 + 8, False), ("two", 16 * 4 + 4 + 48 + 48 + 32 + 8, True)):
                kw = dict(out_rgba8=out, history_len=hlen, sample_count=counts)
                if two:
                    kw.update(accum_b=acc_b, out_b=out_b)
                t_in = timed("temporal_" + name, lambda: r.temporal_accumulate(T, acc_a, f0, f1, F, out_a, **kw),
                             bytes_per_texel=per_texel, bytes_moved=per_texel * texels)
                moved = (per_texel + 16) * texels
                t_re = timed("reproject_" + name, lambda: r.temporal_reproject(T, acc_a, f0, f1, F, mv, out_a, **kw),
                             bytes_per_texel=per_texel + 16, bytes_moved=moved)
                c = timed("copy_of_reproject_" + name, copy_of(moved), bytes_moved=moved)
                print(json.dumps({"what": "ratio", "name": "reproject_" + name, "reproject_over_in_place": round(t_re / t_in, 3),
                                  "reproject_over_copy": round(t_re / c, 3), "reproject_tb_per_s": round(moved / t_re / 1e9, 3),
                                  "copy_tb_per_s": round(moved / c / 1e9, 3)}), flush=True)
            half = hash_options()

            def chain(reproject):
                def fn():
                    r.render_halves(rci, acc_a, acc_b, scratch, options=half)
                    r.render_features(rci, f0, f1, samples=F, options=half)
                    if reproject:
                        r.render_motion(M, rci, mv)
                        M.keep_current(rci0)       # (the step stays: every launch reprojects along it)
                        r.temporal_reproject(T, acc_a, f0, f1, F, mv, out_a, accum_b=acc_b, out_b=out_b, spp=spp // 2)
                    else:
                        r.temporal_accumulate(T, acc_a, f0, f1, F, out_a, accum_b=acc_b, out_b=out_b, spp=spp // 2)
                    r.denoise_variance(out_a, out_b, f0, f1, F, out, half_spp=1, out_mean=mean)
                return fn
            timed("chain_8spp_temporal_variance", chain(False), spp=spp, reproject=False)
            timed("chain_8spp_reproject_variance", chain(True), spp=spp, reproject=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reproject", action="store_true")
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    args = ap.parse_args()

    import torch
    import rtvk

    if not torch.cuda.is_available():
        print("temporal_quality.py needs a GPU", file=sys.stderr)
        return 1

    def f4(W, H):
        return torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")

    def u8(W, H):
        return torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")

    def hash_options(base=0):
        return rtvk.make_options(rng_mode=rtvk.HASH, sample_base=base)

    with rtvk.Renderer(0) as r:
        if args.reproject:
            return reproject_measurements(args, r, torch, rtvk)
        if not args.skip_quality:
            W, H, spp, ref_spp, F = args.width, args.height, 4, 1024, 16
            acc_a, acc_b, acc, f0, f1, out_a, out_b, out_s, mean = (f4(W, H) for _ in range(9))
            out, scratch = u8(W, H), u8(W, H)
            hlen = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            rci = rtvk.canonical_render_call_info(spp, W, H)
            for name, dt, N, last in ROWS:
                params = rtvk.make_temporal(max_history=N)
                with r.temporal(W, H) as two, r.temporal(W, H) as one:
                    for k in range(last + 1):
                        r.set_scene(rtvk.generateRandomScene(float(np.float32(k * dt))))
                        r.render_halves(rci, acc_a, acc_b, scratch, options=hash_options(spp * k))
                        r.render_features(rci, f0, f1, samples=F, options=hash_options())
                        torch.add(acc_a, acc_b, out=acc)      # the frame's sum (a binary32 sum of the halves)
                        r.temporal_accumulate(two, acc_a, f0, f1, F, out_a, accum_b=acc_b, out_b=out_b, history_len=hlen,
                                              spp=spp // 2, params=params)
                        r.temporal_accumulate(one, acc, f0, f1, F, out_s, spp=spp, params=params)
                    r.render_device(rtvk.canonical_render_call_info(ref_spp, W, H), mean, out, options=hash_options(1 << 20))
                    torch.cuda.synchronize()
                    ref = mean.cpu().numpy()[..., :3] / np.float32(ref_spp)

                    def filtered(call):
                        call()
                        torch.cuda.synchronize()
                        return round(psnr(mean.cpu().numpy()[..., :3], ref), 2)
                    rec = {"what": "quality", "row": name, "width": W, "height": H, "spp": spp, "feature_samples": F,
                           "ref_spp": ref_spp, "dt": dt, "max_history": N, "frame": last,
                           "history_valid_share": round(float((hlen > 1).float().mean().item()), 4),
                           "psnr_noisy_db": round(psnr(acc.cpu().numpy()[..., :3] / np.float32(spp), ref), 2),
                           "psnr_temporal_db": round(psnr(((out_a + out_b) * 0.5).cpu().numpy()[..., :3], ref), 2)}
                    rec["psnr_plain_db"] = filtered(lambda: r.denoise(acc, f0, f1, F, out, spp=spp, out_mean=mean))
                    rec["psnr_variance_db"] = filtered(
                        lambda: r.denoise_variance(acc_a, acc_b, f0, f1, F, out, half_spp=spp // 2, out_mean=mean))
                    rec["psnr_temporal_plain_db"] = filtered(lambda: r.denoise(out_s, f0, f1, F, out, spp=1, out_mean=mean))
                    rec["psnr_temporal_variance_db"] = filtered(
                        lambda: r.denoise_variance(out_a, out_b, f0, f1, F, out, half_spp=1, out_mean=mean))
                    print(json.dumps(rec), flush=True)
        if not args.skip_timing:
            W, H, spp, F = 1920, 1080, 8, 16
            texels = W * H
            r.set_scene(rtvk.generateRandomScene(0.0))
            acc_a, acc_b, f0, f1, out_a, out_b, mean = (f4(W, H) for _ in range(7))
            out, scratch = u8(W, H), u8(W, H)
            hlen = torch.zeros((H, W), dtype=torch.int32, device="cuda")
            rci = rtvk.canonical_render_call_info(spp, W, H)
            r.render_halves(rci, acc_a, acc_b, scratch, options=hash_options())
            r.render_features(rci, f0, f1, samples=F, options=hash_options())
            counts = torch.full((H, W), spp // 2, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()

            def timed(name, fn, **extra):
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                ms = []
                for _ in range(max(10, args.launches)):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    ms.append(a.elapsed_time(b))
                rec = {"what": "timing", "name": name, "width": W, "height": H, "launches": len(ms),
                       "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
                rec.update(extra)
                print(json.dumps(rec), flush=True)
                return statistics.median(ms)

            hip = rtvk.load_library()      # dlsym on the library's handle finds the HIP runtime it is linked to
            hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
            hip.hipMemcpyAsync.restype = ctypes.c_int
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

            def copy_of(moved):
                """A device-to-device copy that moves `moved` bytes: moved / 2 read, moved / 2 written."""
                n = moved // 2
                src = torch.zeros(n, dtype=torch.uint8, device="cuda")
                dst = torch.zeros(n, dtype=torch.uint8, device="cuda")

                def fn():
                    rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), n, 3, stream)      # hipMemcpyDeviceToDevice
                    assert rc == 0, rc
                fn.keep = (src, dst)
                return fn

            with r.temporal(W, H) as T:
                # bytes per texel: A (B), feat0, feat1, the count, HA (HB), HG read; HA (HB), HG, out_a (out_b),
                # rgba8 and the length written
                for name, per_texel, call in (
                        ("temporal_one", 16 * 3 + 4 + 32 + 32 + 16 + 8,
                         lambda: r.temporal_accumulate(T, acc_a, f0, f1, F, out_a, out_rgba8=out, history_len=hlen,
                                                       sample_count=counts)),
                        ("temporal_two", 16 * 4 + 4 + 48 + 48 + 32 + 8,
                         lambda: r.temporal_accumulate(T, acc_a, f0, f1, F, out_a, accum_b=acc_b, out_b=out_b, out_rgba8=out,
                                                       history_len=hlen, sample_count=counts))):
                    moved = per_texel * texels
                    t = timed(name, call, bytes_per_texel=per_texel, bytes_moved=moved)
                    c = timed("copy_of_" + name, copy_of(moved), bytes_moved=moved)
                    print(json.dumps({"what": "ratio", "name": name, "call_over_copy": round(t / c, 3),
                                      "call_tb_per_s": round(moved / t / 1e9, 3), "copy_tb_per_s": round(moved / c / 1e9, 3)}),
                          flush=True)
                half = hash_options()

                def chain(temporal):
                    def fn():
                        r.render_halves(rci, acc_a, acc_b, scratch, options=half)
                        r.render_features(rci, f0, f1, samples=F, options=half)
                        if temporal:
                            r.temporal_accumulate(T, acc_a, f0, f1, F, out_a, accum_b=acc_b, out_b=out_b, spp=spp // 2)
                            r.denoise_variance(out_a, out_b, f0, f1, F, out, half_spp=1, out_mean=mean)
                        else:
                            r.denoise_variance(acc_a, acc_b, f0, f1, F, out, half_spp=spp // 2, out_mean=mean)
                    return fn
                timed("chain_8spp_variance", chain(False), spp=spp, temporal=False)
                timed("chain_8spp_temporal_variance", chain(True), spp=spp, temporal=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
