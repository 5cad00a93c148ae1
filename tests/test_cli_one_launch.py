"""The command-line front end's --map-launch levels|one: the schedule of the sample-map replays of
--adaptive ... --frames ... --replay R."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim   # noqa: E402

CLI = Path(__file__).resolve().parent.parent / "ray-tracing-gpu-vulkan_amd" / "bin" / "rt_mi355x_cli"
LOOP = ("--adaptive", "0.2,8,8", "--samples", "64", "--width", "64", "--height", "40", "--frames", "3")


def run(*args, cwd=None):
    return subprocess.run([str(CLI), *args], capture_output=True, text=True, cwd=cwd, timeout=300)


def test_help_lists_map_launch():
    r = run("--help")
    assert r.returncode == 0 and "--map-launch" in r.stdout


def test_map_launch_without_replay_and_unknown_values_are_refused(tmp_path):
    """Refused before any device is touched, and nothing is stored."""
    r = run(*LOOP, "--map-launch", "one", "--store", cwd=tmp_path)
    assert r.returncode == 2 and "--map-launch" in r.stderr and "--replay" in r.stderr
    assert run("--map-launch", "one", cwd=tmp_path).returncode == 2
    for bad in ("two", "1", ""):
        r = run(*LOOP, "--replay", "1", "--map-launch", bad, "--store", cwd=tmp_path)
        assert r.returncode == 2 and "levels or one" in r.stderr
    assert run(*LOOP, "--replay", "1", "--map-launch", cwd=tmp_path).returncode == 2   # the value is missing
    assert not (tmp_path / "render.ppm").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["one", "levels"])
def test_replay_runs_and_names_the_schedule(tmp_path, oracle, schedule):
    """Frames 0 and 2 are adaptive, frame 1 replays frame 0's counts: at t = 0 the stored last frame is
    the adaptive frame either way, and every report line names the schedule."""
    W, H = 64, 40
    r = run(*LOOP, "--replay", "1", "--map-launch", schedule, "--store", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    counts, info = sim.simulate(sim.cube(oracle, W, H, 64), 8, 8, 64, 13107)
    _, ref = sim.expected_frame(oracle, counts)
    data = (tmp_path / "render.ppm").read_bytes()
    hdr = b"P6\n64 40\n255\n"
    assert data.startswith(hdr)
    np.testing.assert_array_equal(np.frombuffer(data[len(hdr):], np.uint8).reshape(H, W, 3), ref[..., :3])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("duration_per_frame")]
    assert lines and all(f"map launch {schedule}" in ln for ln in lines)
    assert sum(int(re.search(r"\((\d+) frames", ln).group(1)) for ln in lines) == 3
    assert sum(int(re.search(r"(\d+) replays", ln).group(1)) for ln in lines) == 1
    assert all(f"mean {info['samples'] / (W * H):.2f} spp of at most 64" in ln for ln in lines)
