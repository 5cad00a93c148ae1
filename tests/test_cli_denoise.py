"""The command-line front end's --denoise [F[,ITER]]: one frame of the counter-based stream on one
GPU (plain with --rng hash, or --adaptive), first-hit features of F samples per pixel and the
edge-avoiding denoise; --store writes the denoised image."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

CLI = Path(__file__).resolve().parent.parent / "ray-tracing-gpu-vulkan_amd" / "bin" / "rt_mi355x_cli"
HASH = 2


def run(*args, cwd=None):
    return subprocess.run([str(CLI), *args], capture_output=True, text=True, cwd=cwd, timeout=300)


def test_help_lists_denoise():
    r = run("--help")
    assert r.returncode == 0 and "--denoise" in r.stdout


def test_denoise_refusals(tmp_path):
    """Refused before any device is touched, with a message, and nothing is stored."""
    small = ("--samples", "4", "--width", "64", "--height", "40", "--store")
    r = run("--denoise", "--rng", "hash", "--gpus", "2", *small, cwd=tmp_path)
    assert r.returncode != 0 and "--denoise" in r.stderr and "--gpus" in r.stderr
    r = run("--denoise", "--rng", "pixel", *small, cwd=tmp_path)
    assert r.returncode != 0 and "--rng" in r.stderr
    r = run("--denoise", "--rng", "stream", *small, cwd=tmp_path)
    assert r.returncode != 0 and "--denoise" in r.stderr and "--rng hash" in r.stderr
    r = run("--denoise", *small, cwd=tmp_path)                       # the default stream is the reference's
    assert r.returncode != 0 and "--rng hash" in r.stderr
    r = run("--denoise", "--rng", "hash", "--frames", "2", *small, cwd=tmp_path)
    assert r.returncode != 0 and "--frames" in r.stderr
    for bad in ("0", "257", "16,0", "16,7"):
        r = run("--denoise", bad, "--rng", "hash", *small, cwd=tmp_path)
        assert r.returncode != 0 and "--denoise" in r.stderr, bad
    assert run("--denoise", "16,x", "--rng", "hash", *small, cwd=tmp_path).returncode != 0
    assert not (tmp_path / "render.ppm").exists()


def read_ppm(path, W, H):
    data = path.read_bytes()
    hdr = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(hdr)
    return np.frombuffer(data[len(hdr):], np.uint8).reshape(H, W, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("args,F,it", [((), 16, 3), (("5,2",), 5, 2)])
def test_denoise_store_equals_the_api(tmp_path, oracle, args, F, it):
    import torch
    import rtvk
    W, H, spp = 64, 40, 4
    r = run("--denoise", *args, "--rng", "hash", "--samples", str(spp), "--width", str(W), "--height", str(H), "--store",
            cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "duration_per_frame" in r.stdout and f"{F} feature samples, {it} iterations" in r.stdout
    img = read_ppm(tmp_path / "render.ppm", W, H)
    rci = rtvk.canonical_render_call_info(spp, W, H)
    with rtvk.Renderer(0) as rd:
        rd.set_scene(rtvk.generateRandomScene(0.0))
        acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        f0 = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        f1 = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        noisy = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        rd.render_device(rci, acc, noisy, options=rtvk.make_options(rng_mode=HASH))
        rd.render_features(rci, f0, f1, samples=F)
        rd.denoise(acc, f0, f1, F, out, spp=spp, params=rtvk.make_denoise(iterations=it))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(img, out.cpu().numpy()[..., :3])
        assert not np.array_equal(img, noisy.cpu().numpy()[..., :3])     # the stored image is the denoised one


@pytest.mark.gpu
def test_denoise_of_an_adaptive_frame(tmp_path, oracle):
    import torch
    import rtvk
    W, H = 64, 40
    r = run("--denoise", "--adaptive", "0.2,8,8", "--samples", "32", "--width", str(W), "--height", str(H), "--store",
            cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "adaptive" in r.stdout and "16 feature samples, 3 iterations" in r.stdout
    img = read_ppm(tmp_path / "render.ppm", W, H)
    rci = rtvk.canonical_render_call_info(32, W, H)
    with rtvk.Renderer(0) as rd:
        rd.set_scene(rtvk.generateRandomScene(0.0))
        acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        f0 = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        f1 = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        rd.render_adaptive(rci, acc, out, sample_count=cnt, options=rtvk.make_options(rng_mode=HASH),
                           adaptive=rtvk.make_adaptive(0.2, 8, 8))
        rd.render_features(rci, f0, f1, samples=16)
        rd.denoise(acc, f0, f1, 16, out, sample_count=cnt)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(img, out.cpu().numpy()[..., :3])
