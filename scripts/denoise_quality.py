#!/usr/bin/env python3
"""Quality and cost of the denoiser, canonical scene, counter-based stream.

  quality  at 480x270, for spp in {2, 4, 8, 16, 32, 64} and feature samples F in {spp, 16, 64}: the
           PSNR (dB, on sqrt(clip(mean))) of the noisy frame and of the denoised frame (default
           parameters) against the 1024-spp frame. The reference is rendered on the GPU, whose
           frame is the oracle's bit for bit (tests/test_gpu_parity.py); --oracle-ref renders it
           with the CPU oracle instead (minutes).
  timing   at 1920x1080: GPU time of the 8-spp frame, of the feature pass (F = 16) and of the
           denoise (3 iterations), each the median of --launches launches after warm-up, between
           two stream events; the min and max of the same launches give the spread. Then the
           denoise at 1..6 iterations, and at 6 iterations with the LDS form up to step 0, 1, 2, 4
           (rt_debug_denoise_lds_steps): the differences are the cost of one iteration in each form.

Prints one JSON line per measurement.
  python scripts/denoise_quality.py [--skip-quality] [--skip-timing] [--launches 20] [--oracle-ref]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "ray-tracing-gpu-vulkan_amd")]


def psnr(mean, ref):
    a = np.sqrt(np.clip(mean.astype(np.float64), 0.0, 1.0))
    b = np.sqrt(np.clip(ref.astype(np.float64), 0.0, 1.0))
    return float(10.0 * np.log10(1.0 / np.mean((a - b) ** 2)))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-quality", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--oracle-ref", action="store_true")
    args = ap.parse_args()

    import torch
    import rtvk

    if not torch.cuda.is_available():
        print("denoise_quality.py needs a GPU", file=sys.stderr)
        return 1
    opt = rtvk.make_options(rng_mode=rtvk.HASH)

    def buffers(W, H):
        f = lambda: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")   # noqa: E731
        return f(), f(), f(), f(), torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")

    with rtvk.Renderer(0) as r:
        r.set_scene(rtvk.generateRandomScene(0.0))
        if not args.skip_quality:
            W, H, ref_spp = 480, 270, 1024
            acc, f0, f1, mean, out = buffers(W, H)
            if args.oracle_ref:
                from oracle import oracle
                ra, _, _ = oracle.render(oracle.generate_scene(), oracle.render_call_info(ref_spp, W, H), W, H,
                                         opts=oracle.options(rng_mode=2))
                ref = ra[..., :3] / np.float32(ref_spp)
            else:
                r.render_device(rtvk.canonical_render_call_info(ref_spp, W, H), acc, out, options=opt)
                torch.cuda.synchronize()
                ref = acc.cpu().numpy()[..., :3] / np.float32(ref_spp)
            feats = {}
            for spp in (2, 4, 8, 16, 32, 64):
                rci = rtvk.canonical_render_call_info(spp, W, H)
                r.render_device(rci, acc, out, options=opt)
                torch.cuda.synchronize()
                noisy = psnr(acc.cpu().numpy()[..., :3] / np.float32(spp), ref)
                for F in sorted({spp, 16, 64}):
                    if F not in feats:
                        r.render_features(rci, f0, f1, samples=F, options=opt)
                        feats[F] = (f0.clone(), f1.clone())
                    g0, g1 = feats[F]
                    r.denoise(acc, g0, g1, F, out, spp=spp, out_mean=mean)
                    torch.cuda.synchronize()
                    print(json.dumps({"what": "quality", "width": W, "height": H, "spp": spp, "feature_samples": F,
                                      "ref_spp": ref_spp, "psnr_noisy_db": round(noisy, 2),
                                      "psnr_denoised_db": round(psnr(mean.cpu().numpy()[..., :3], ref), 2)}), flush=True)
        if not args.skip_timing:
            W, H, spp, F = 1920, 1080, 8, 16
            acc, f0, f1, mean, out = buffers(W, H)
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

            t_frame = timed("frame", lambda: r.render_device(rci, acc, out, options=opt), spp=spp)
            t_feat = timed("features", lambda: r.render_features(rci, f0, f1, samples=F, options=opt), feature_samples=F)
            t_dn = timed("denoise", lambda: r.denoise(acc, f0, f1, F, out, spp=spp, out_mean=mean), iterations=3)
            print(json.dumps({"what": "cost", "features_plus_denoise_over_frame": round((t_feat + t_dn) / t_frame, 4)}),
                  flush=True)
            for it in range(1, 7):
                p = rtvk.make_denoise(iterations=it)
                timed("denoise", lambda: r.denoise(acc, f0, f1, F, out, spp=spp, out_mean=mean, params=p), iterations=it)
            p6 = rtvk.make_denoise(iterations=6)
            for lds in (0, 1, 2, 4):
                r.denoise_lds_steps(lds)
                timed("denoise", lambda: r.denoise(acc, f0, f1, F, out, spp=spp, out_mean=mean, params=p6), iterations=6,
                      lds_max_step=lds)
            r.denoise_lds_steps(4)
    return 0


if __name__ == "__main__":
    sys.exit(main())
