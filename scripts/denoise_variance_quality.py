#!/usr/bin/env python3
"""Quality and cost of the variance-guided denoise, canonical scene,
counter-based stream, after scripts/denoise_quality.py.

  quality  at 480x270 (--width / --height), for spp in {2, 4, 8, 16, 32, 64, 128}, 16 feature
           samples: the PSNR (dB, on sqrt(clip(mean))) against the 1024-spp frame of the noisy frame
           (the sum of the two halves), of the plain filter on that sum (rt_denoise_device,
           defaults) and of the variance-guided filter on the halves (defaults). Beside the
           defaults: prefilter 0 (the raw half-difference estimate), 1 and 3, k_color 0.125 and
           0.5, and the variance held fixed through the iterations (not in the library: the numpy
           restatement tests/denoise_var_sim.py on the GPU's frames). The frames and the reference
           are rendered on the GPU, whose frames are the oracle's bit for bit.
  timing   at 1920x1080, each the median of --launches launches after warm-up between two stream
           events, with min and max, all in this one process: the plain filter at 1..3 iterations;
           the variance-guided filter at (prefilter, iterations) (0, 1..3) and (1..3, 3), whose
           differences are the cost of one iteration and of one prefilter pass at each step; both
           at 3 iterations with every launch forced to global memory; the 8-spp frame in one
           launch and as two 4-spp halves.

Prints one JSON line per measurement.
  python scripts/denoise_variance_quality.py [--skip-quality] [--skip-timing] [--launches 20]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ray-tracing-gpu-vulkan_amd"), str(ROOT / "tests")]


def psnr(mean, ref):
    a = np.sqrt(np.clip(mean.astype(np.float64), 0.0, 1.0))
    b = np.sqrt(np.clip(ref.astype(np.float64), 0.0, 1.0))
    return float(10.0 * np.log10(1.0 / np.mean((a - b) ** 2)))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--height", type=int, default=270)
    args = ap.parse_args()

    import torch
    import rtvk

    if not torch.cuda.is_available():
        print("denoise_variance_quality.py needs a GPU", file=sys.stderr)
        return 1
    opt = rtvk.make_options(rng_mode=rtvk.HASH)

    def f4(W, H):
        return torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")

    def u8(W, H):
        return torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")

    with rtvk.Renderer(0) as r:
        r.set_scene(rtvk.generateRandomScene(0.0))
        if not args.skip_quality:
            import denoise_var_sim as dv
            W, H, ref_spp, F = args.width, args.height, 1024, 16
            acc_a, acc_b, acc, f0, f1, mean = (f4(W, H) for _ in range(6))
            out, scratch = u8(W, H), u8(W, H)
            r.render_device(rtvk.canonical_render_call_info(ref_spp, W, H), acc, out, options=opt)
            torch.cuda.synchronize()
            ref = acc.cpu().numpy()[..., :3] / np.float32(ref_spp)
            r.render_features(rtvk.canonical_render_call_info(ref_spp, W, H), f0, f1, samples=F, options=opt)
            for spp in (2, 4, 8, 16, 32, 64, 128):
                rci = rtvk.canonical_render_call_info(spp, W, H)
                r.render_halves(rci, acc_a, acc_b, scratch, options=opt)
                torch.add(acc_a, acc_b, out=acc)      # the frame's sum (a binary32 sum of the halves)
                acc[..., 3] = 1.0
                r.denoise(acc, f0, f1, F, out, spp=spp, out_mean=mean)
                torch.cuda.synchronize()
                rec = {"what": "quality", "width": W, "height": H, "spp": spp, "feature_samples": F, "ref_spp": ref_spp,
                       "psnr_noisy_db": round(psnr(acc.cpu().numpy()[..., :3] / np.float32(spp), ref), 2),
                       "psnr_plain_db": round(psnr(mean.cpu().numpy()[..., :3], ref), 2)}

                def guided(**kw):
                    r.denoise_variance(acc_a, acc_b, f0, f1, F, out, half_spp=spp // 2, out_mean=mean,
                                       params=rtvk.make_denoise_variance(**kw))
                    torch.cuda.synchronize()
                    return round(psnr(mean.cpu().numpy()[..., :3], ref), 2)
                rec["psnr_variance_db"] = guided()
                for pre in (0, 1, 3):
                    rec[f"psnr_prefilter{pre}_db"] = guided(prefilter=pre)
                for kc in (0.125, 0.5):
                    rec[f"psnr_k_color_{kc}_db"] = guided(k_color=kc)
                held = dv.denoise(acc_a.cpu().numpy(), acc_b.cpu().numpy(), f0.cpu().numpy(), f1.cpu().numpy(), F,
                                  half_spp=spp // 2, track=False)
                rec["psnr_variance_held_fixed_db"] = round(psnr(held[..., :3], ref), 2)
                print(json.dumps(rec), flush=True)
        if not args.skip_timing:
            W, H, spp, F = 1920, 1080, 8, 16
            acc_a, acc_b, acc, f0, f1, mean = (f4(W, H) for _ in range(6))
            out, scratch = u8(W, H), u8(W, H)
            rci = rtvk.canonical_render_call_info(spp, W, H)

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

            timed("frame", lambda: r.render_device(rci, acc, out, options=opt), spp=spp)
            timed("halves", lambda: r.render_halves(rci, acc_a, acc_b, scratch, options=opt), spp=spp)
            r.render_features(rci, f0, f1, samples=F, options=opt)
            torch.add(acc_a, acc_b, out=acc)
            torch.cuda.synchronize()

            def plain(it):
                p = rtvk.make_denoise(iterations=it)
                return lambda: r.denoise(acc, f0, f1, F, out, spp=spp, out_mean=mean, params=p)

            def guided(pre, it):
                p = rtvk.make_denoise_variance(iterations=it, prefilter=pre)
                return lambda: r.denoise_variance(acc_a, acc_b, f0, f1, F, out, half_spp=spp // 2, out_mean=mean, params=p)

            for it in (1, 2, 3):
                timed("denoise", plain(it), iterations=it)
            for pre, it in ((0, 1), (0, 2), (0, 3), (1, 3), (2, 3), (3, 3)):
                timed("denoise_variance", guided(pre, it), prefilter=pre, iterations=it)
            r.denoise_lds_steps(0)
            timed("denoise", plain(3), iterations=3, lds_max_step=0)
            timed("denoise_variance", guided(0, 3), prefilter=0, iterations=3, lds_max_step=0)
            timed("denoise_variance", guided(2, 3), prefilter=2, iterations=3, lds_max_step=0)
            r.denoise_lds_steps(4)
    return 0


if __name__ == "__main__":
    sys.exit(main())
