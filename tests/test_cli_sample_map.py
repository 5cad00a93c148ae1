"""The command-line front end's adaptive frame loop: --adaptive THR[,MIN[,STEP]] --frames N
[--animate] [--replay R] (adaptive frames and sample-map replays of their counts)."""
import re
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


def test_help_lists_replay():
    r = run("--help")
    assert r.returncode == 0 and "--replay" in r.stdout


def test_replay_and_many_gpus_are_refused(tmp_path):
    """Refused before any device is touched, and nothing is stored."""
    r = run("--replay", "2", "--store", cwd=tmp_path)
    assert r.returncode == 2 and "--replay" in r.stderr and "--adaptive" in r.stderr and "--frames" in r.stderr
    assert run("--replay", "2", "--adaptive", "0.2", cwd=tmp_path).returncode == 2
    assert run("--replay", "2", "--frames", "3", cwd=tmp_path).returncode == 2
    assert run("--adaptive", "0.2", "--frames", "3", "--replay", cwd=tmp_path).returncode == 2
    r = run("--adaptive", "0.2,8,8", "--frames", "3", "--gpus", "2", "--store", cwd=tmp_path)
    assert r.returncode == 2 and "--adaptive" in r.stderr and "--gpus" in r.stderr
    assert not (tmp_path / "render.ppm").exists()


@pytest.mark.gpu
def test_replayed_frame_matches_simulation(tmp_path, oracle):
    """Frames 1 and 2 replay frame 0's counts at t = 0, so the stored last frame is the adaptive frame."""
    W, H = 64, 40
    r = run("--adaptive", "0.2,8,8", "--samples", "64", "--width", str(W), "--height", str(H), "--frames", "3",
            "--replay", "2", "--store", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    counts, info = sim.simulate(sim.cube(oracle, W, H, 64), 8, 8, 64, 13107)
    sim.assert_not_vacuous(counts, 64)
    _, ref = sim.expected_frame(oracle, counts)
    data = (tmp_path / "render.ppm").read_bytes()
    hdr = b"P6\n64 40\n255\n"
    assert data.startswith(hdr)
    img = np.frombuffer(data[len(hdr):], np.uint8).reshape(H, W, 3)
    np.testing.assert_array_equal(img, ref[..., :3])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("duration_per_frame")]
    # one report line per second of frames: usually one; frames and replays add up over them, and every
    # frame has the adaptive frame's samples, so every line's mean spp is its mean
    assert sum(int(re.search(r"\((\d+) frames", ln).group(1)) for ln in lines) == 3
    assert sum(int(re.search(r"(\d+) replays", ln).group(1)) for ln in lines) == 2
    assert all(f"mean {info['samples'] / (W * H):.2f} spp of at most 64" in ln for ln in lines)
