"""The command-line front end's --adaptive THRESHOLD[,MIN[,STEP]] (one adaptive frame on one GPU)."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim   # noqa: E402

CLI = Path(__file__).resolve().parent.parent / "ray-tracing-gpu-vulkan_amd" / "bin" / "rt_mi355x_cli"


def run(*args, cwd=None):
    return subprocess.run([str(CLI), *args], capture_output=True, text=True, cwd=cwd, timeout=300)


def test_help_lists_adaptive():
    r = run("--help")
    assert r.returncode == 0 and "--adaptive" in r.stdout


def test_adaptive_refuses_stream_rng_and_many_gpus(tmp_path):
    """Refused before any device is touched, loudly, and nothing is stored."""
    r = run("--adaptive", "0.2,8,8", "--rng", "stream", "--samples", "64", "--width", "64", "--height", "40",
            "--store", cwd=tmp_path)
    assert r.returncode == 2 and "--adaptive" in r.stderr and "--rng stream" in r.stderr
    r = run("--adaptive", "0.2", "--gpus", "2", "--store", cwd=tmp_path)
    assert r.returncode == 2 and "--adaptive" in r.stderr and "--gpus" in r.stderr
    assert run("--adaptive", cwd=tmp_path).returncode == 2
    assert run("--adaptive", "x,8", cwd=tmp_path).returncode == 2
    assert run("--adaptive", "0.2,8,", cwd=tmp_path).returncode == 2
    assert not (tmp_path / "render.ppm").exists()


@pytest.mark.gpu
def test_adaptive_store_matches_simulation(tmp_path, oracle):
    W, H = 64, 40
    r = run("--adaptive", "0.2,8,8", "--samples", "64", "--width", str(W), "--height", str(H), "--store",
            cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    counts, info = sim.simulate(sim.cube(oracle, W, H, 64), 8, 8, 64, 13107)
    sim.assert_not_vacuous(counts, 64)
    _, ref = sim.expected_frame(oracle, counts)
    data = (tmp_path / "render.ppm").read_bytes()
    hdr = b"P6\n64 40\n255\n"
    assert data.startswith(hdr)
    img = np.frombuffer(data[len(hdr):], np.uint8).reshape(H, W, 3)
    np.testing.assert_array_equal(img, ref[..., :3])
    # passes, mean spp and capped tiles next to the frame time
    assert "duration_per_frame" in r.stdout
    assert f"{info['passes']} passes" in r.stdout
    assert f"mean {info['samples'] / (W * H):.2f} spp" in r.stdout
    assert f"{info['tiles_capped']} of {info['tiles']} tiles capped" in r.stdout
