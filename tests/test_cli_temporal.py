"""The command-line front end's --temporal [N]: the one pairing of --denoise or --denoise-variance with
the frame loop (--frames K [--animate]). Frame k is rendered from a sample range of its own, the
features at sample_base 0, and the temporal stage integrates the frames ahead of the filter; --store
writes the last frame's filtered image. Every refusal exits non-zero with a message naming the option
before anything renders, and without --temporal both filters still refuse --frames as before. On the
GPU the stored bytes are those of the Python chain of test_gpu_temporal.py at t = 0."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

CLI = Path(__file__).resolve().parent.parent / "ray-tracing-gpu-vulkan_amd" / "bin" / "rt_mi355x_cli"


def run(*args, cwd=None):
    return subprocess.run([str(CLI), *args], capture_output=True, text=True, cwd=cwd, timeout=300)


def test_help_lists_temporal():
    r = run("--help")
    assert r.returncode == 0 and "--temporal" in r.stdout


def test_frames_without_temporal_are_refused_as_before(tmp_path):
    small = ("--rng", "hash", "--samples", "4", "--width", "64", "--height", "40", "--store", "--frames", "2")
    r = run("--denoise", *small, cwd=tmp_path)
    assert r.returncode != 0 and r.stderr == "--denoise renders one frame: it cannot run with --frames\n"
    r = run("--denoise-variance", *small, cwd=tmp_path)
    assert r.returncode != 0 and r.stderr == "--denoise-variance renders one frame: it cannot run with --frames\n"
    assert not (tmp_path / "render.ppm").exists()


def test_temporal_refusals(tmp_path):
    """Refused before any device is touched, with a message, and nothing is stored."""
    size = ("--samples", "4", "--width", "64", "--height", "40", "--store")
    loop = ("--frames", "2", "--rng", "hash")
    flag = "--temporal"
    for filt in ("--denoise", "--denoise-variance"):
        r = run(flag, filt, "--rng", "hash", *size, cwd=tmp_path)                       # no --frames
        assert r.returncode != 0 and flag in r.stderr and "--frames" in r.stderr
        r = run(flag, filt, *loop, "--gpus", "2", *size, cwd=tmp_path)
        assert r.returncode != 0 and flag in r.stderr and "--gpus" in r.stderr
        r = run(flag, filt, *loop, "--adaptive", "0.2,8,8", *size, cwd=tmp_path)
        assert r.returncode != 0 and flag in r.stderr and "--adaptive" in r.stderr
        r = run(flag, filt, "--frames", "2", "--rng", "stream", *size, cwd=tmp_path)
        assert r.returncode != 0 and flag in r.stderr and "--rng hash" in r.stderr
        r = run(flag, filt, "--frames", "2", *size, cwd=tmp_path)                       # the default stream
        assert r.returncode != 0 and flag in r.stderr and "--rng hash" in r.stderr
        for bad in ("0", "1", "65536"):                                                 # N outside 2 .. 65535
            r = run(flag, bad, filt, *loop, *size, cwd=tmp_path)
            assert r.returncode != 0 and flag in r.stderr and "max_history" in r.stderr, bad
        assert run(flag, "8x", filt, *loop, *size, cwd=tmp_path).returncode != 0
        # K x samples past 32 bits
        r = run(flag, filt, "--rng", "hash", "--frames", "65536", "--samples", "65536", "--width", "64", "--height", "40",
                cwd=tmp_path)
        assert r.returncode != 0 and flag in r.stderr and "32 bits" in r.stderr
    r = run(flag, *loop, *size, cwd=tmp_path)                                           # no filter
    assert r.returncode != 0 and flag in r.stderr and "--denoise" in r.stderr
    r = run(flag, "--denoise", "--denoise-variance", *loop, *size, cwd=tmp_path)        # both filters: as without
    assert r.returncode != 0 and "with --denoise" in r.stderr
    r = run(flag, "--denoise-variance", *loop, "--samples", "5", "--width", "64", "--height", "40", cwd=tmp_path)
    assert r.returncode != 0 and "odd" in r.stderr
    assert not (tmp_path / "render.ppm").exists()


def read_ppm(path, W, H):
    data = path.read_bytes()
    hdr = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(hdr)
    return np.frombuffer(data[len(hdr):], np.uint8).reshape(H, W, 3)


@pytest.mark.gpu
def test_temporal_store_equals_the_python_chain(tmp_path, oracle):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rtvk
    from test_gpu_temporal import CHAIN, gpu_chain
    W, H = CHAIN["W"], CHAIN["H"]
    r = run("--denoise-variance", str(CHAIN["F"]), "--temporal", str(CHAIN["N"]), "--rng", "hash", "--frames", "3", "--samples",
            str(CHAIN["spp"]), "--width", str(W), "--height", str(H), "--store", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "duration_per_frame" in r.stdout and f"temporal history {CHAIN['N']}" in r.stdout
    img = read_ppm(tmp_path / "render.ppm", W, H)
    _, _, out, lens = gpu_chain(rtvk, torch, oracle, (0.0, 0.0, 0.0), True)
    assert np.all(lens[2] == 3)                                   # a static scene: every texel valid
    np.testing.assert_array_equal(img, out[..., :3])


@pytest.mark.gpu
def test_temporal_store_of_the_plain_filter_equals_the_python_chain(tmp_path, oracle):
    """--denoise F --temporal N: the plain filter behind the stage, one accumulator per frame."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rtvk
    from test_gpu_temporal import CHAIN, gpu_chain
    W, H = CHAIN["W"], CHAIN["H"]
    r = run("--denoise", str(CHAIN["F"]), "--temporal", str(CHAIN["N"]), "--rng", "hash", "--frames", "3", "--samples",
            str(CHAIN["spp"]), "--width", str(W), "--height", str(H), "--store", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert f"temporal history {CHAIN['N']}, plain denoise: {CHAIN['F']} feature samples" in r.stdout
    assert "two halves" not in r.stdout and "reprojected" not in r.stdout
    img = read_ppm(tmp_path / "render.ppm", W, H)
    _, _, out, lens = gpu_chain(rtvk, torch, oracle, (0.0, 0.0, 0.0), False)
    assert np.all(lens[2] == 3)
    np.testing.assert_array_equal(img, out[..., :3])
