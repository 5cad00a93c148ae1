"""The command-line front end's --denoise-variance [F[,ITER[,PRE]]]: one frame of the counter-based
stream on one GPU rendered as two halves, first-hit features of F samples per pixel and the
variance-guided denoise; --store writes the denoised image. On the GPU the stored bytes are the
restatement's (tests/denoise_var_sim.py on the oracle's halves); every refusal exits non-zero with
its message before anything renders."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import denoise_sim as ds
import denoise_var_sim as dv

CLI = Path(__file__).resolve().parent.parent / "ray-tracing-gpu-vulkan_amd" / "bin" / "rt_mi355x_cli"
HASH = 2


def run(*args, cwd=None):
    return subprocess.run([str(CLI), *args], capture_output=True, text=True, cwd=cwd, timeout=300)


def test_help_lists_denoise_variance():
    r = run("--help")
    assert r.returncode == 0 and "--denoise-variance" in r.stdout


def test_denoise_variance_refusals(tmp_path):
    """Refused before any device is touched, with a message, and nothing is stored."""
    small = ("--samples", "4", "--width", "64", "--height", "40", "--store")
    flag = "--denoise-variance"
    r = run(flag, "--rng", "hash", "--gpus", "2", *small, cwd=tmp_path)
    assert r.returncode != 0 and flag in r.stderr and "--gpus" in r.stderr
    r = run(flag, "--rng", "stream", *small, cwd=tmp_path)
    assert r.returncode != 0 and flag in r.stderr and "--rng hash" in r.stderr
    r = run(flag, *small, cwd=tmp_path)                              # the default stream is the reference's
    assert r.returncode != 0 and flag in r.stderr and "--rng hash" in r.stderr
    r = run(flag, "--rng", "hash", "--frames", "2", *small, cwd=tmp_path)
    assert r.returncode != 0 and flag in r.stderr and "--frames" in r.stderr
    r = run(flag, "--rng", "hash", "--samples", "5", "--width", "64", "--height", "40", "--store", cwd=tmp_path)
    assert r.returncode != 0 and flag in r.stderr and "odd" in r.stderr
    r = run(flag, "--adaptive", "0.2,8,8", *small, cwd=tmp_path)
    assert r.returncode != 0 and flag in r.stderr and "--adaptive" in r.stderr
    r = run(flag, "--adaptive", "0.2,8,8", "--rng", "hash", *small, cwd=tmp_path)
    assert r.returncode != 0 and flag in r.stderr and "--adaptive" in r.stderr
    for extra in (("--rng", "hash"), ()):
        r = run(flag, "--denoise", *extra, *small, cwd=tmp_path)
        assert r.returncode != 0 and flag in r.stderr and "with --denoise" in r.stderr
    for bad in ("0", "257", "16,0", "16,7", "16,3,4"):
        r = run(flag, bad, "--rng", "hash", *small, cwd=tmp_path)
        assert r.returncode != 0 and flag in r.stderr, bad
    for bad in ("16,x", "16,3,x", "16,,2"):
        assert run(flag, bad, "--rng", "hash", *small, cwd=tmp_path).returncode != 0, bad
    assert not (tmp_path / "render.ppm").exists()


def read_ppm(path, W, H):
    data = path.read_bytes()
    hdr = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(hdr)
    return np.frombuffer(data[len(hdr):], np.uint8).reshape(H, W, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("args,F,it,pre", [((), 16, 3, 2), (("5,2,1",), 5, 2, 1)])
def test_denoise_variance_store_equals_the_restatement(tmp_path, oracle, args, F, it, pre):
    W, H, spp = 40, 24, 8
    r = run("--denoise-variance", *args, "--rng", "hash", "--samples", str(spp), "--width", str(W), "--height", str(H),
            "--store", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "duration_per_frame" in r.stdout and "variance-guided" in r.stdout
    assert f"{F} feature samples, {pre} prefilter passes, {it} iterations" in r.stdout
    img = read_ppm(tmp_path / "render.ppm", W, H)
    sc = oracle.generate_scene()
    h = spp // 2
    rci = oracle.render_call_info(h, W, H)
    A, _, _ = oracle.render(sc, rci, W, H, opts=oracle.options(rng_mode=HASH, sample_base=0))
    B, _, _ = oracle.render(sc, rci, W, H, opts=oracle.options(rng_mode=HASH, sample_base=h))
    feat0, feat1 = ds.features(oracle, sc, oracle.render_call_info(spp, W, H), W, H, F)
    mean = dv.denoise(A, B, feat0, feat1, F, half_spp=h, params=(it, pre) + dv.DEFAULTS[2:])
    assert np.isfinite(mean).all()
    np.testing.assert_array_equal(img, oracle.resolve(mean, 1)[..., :3])
    noisy = oracle.resolve(A + B, spp)[..., :3]
    assert not np.array_equal(img, noisy)                                # the stored image is the denoised one
