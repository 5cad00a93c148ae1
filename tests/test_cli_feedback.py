"""The command-line front end's --feedback: with --adaptive ... --frames N, frame 0 is the adaptive
frame and every later frame a feedback frame that renders the previous frame's
map, measures it and plans the next on the GPU."""
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim   # noqa: E402
from test_sample_map import texel_counts   # noqa: E402
from test_sample_map_feedback import step   # noqa: E402

CLI = Path(__file__).resolve().parent.parent / "ray-tracing-gpu-vulkan_amd" / "bin" / "rt_mi355x_cli"
LOOP = ("--adaptive", "0.3,4,4", "--samples", "64", "--width", "44", "--height", "27", "--frames", "4")


def run(*args, cwd=None):
    return subprocess.run([str(CLI), *args], capture_output=True, text=True, cwd=cwd, timeout=300)


def test_help_lists_feedback():
    r = run("--help")
    assert r.returncode == 0 and "--feedback" in r.stdout


def test_refusals(tmp_path):
    """Refused before any device is touched, and nothing is stored."""
    r = run(*LOOP, "--feedback", "--replay", "1", "--store", cwd=tmp_path)
    assert r.returncode == 2 and "--feedback" in r.stderr and "--replay" in r.stderr
    r = run(*LOOP, "--feedback", "--gpus", "2", "--store", cwd=tmp_path)
    assert r.returncode == 2 and "--gpus 2" in r.stderr
    r = run("--feedback", "--frames", "3", "--store", cwd=tmp_path)               # no --adaptive
    assert r.returncode == 2 and "--feedback needs --adaptive and --frames" in r.stderr
    r = run("--adaptive", "0.3,4,4", "--feedback", "--store", cwd=tmp_path)       # no --frames
    assert r.returncode == 2 and "--feedback needs --adaptive and --frames" in r.stderr
    assert not (tmp_path / "render.ppm").exists()


@pytest.mark.gpu
def test_feedback_loop_follows_the_simulation(tmp_path, oracle):
    """Four frames at t = 0: the adaptive frame's counts C0, then feedback frames that render C0, C1
    and C2, C_{i+1} the rule applied to the two halves of C_i: the stored last frame is the frame of
    C2, and the report's mean is that of the map planned last, C3."""
    W, H = 44, 27
    r = run(*LOOP, "--feedback", "--store", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    Q = sim.cube(oracle, W, H, 64)
    thr = int(np.floor(float(np.float32(0.3)) * 65536.0 + 0.5))
    counts, _ = sim.simulate(Q, 4, 4, 64, thr)
    table = counts[::8, ::8].ravel().tolist()
    tables = [table]
    for _ in range(3):
        tables.append(step(Q, tables[-1], thr, 4, 64)[0])
    assert tables[1] != tables[0]
    _, ref = sim.expected_frame(oracle, texel_counts(tables[2], W, H))
    data = (tmp_path / "render.ppm").read_bytes()
    hdr = b"P6\n44 27\n255\n"
    assert data.startswith(hdr)
    np.testing.assert_array_equal(np.frombuffer(data[len(hdr):], np.uint8).reshape(H, W, 3), ref[..., :3])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("duration_per_frame")]
    assert lines and sum(int(re.search(r"\((\d+) frames", ln).group(1)) for ln in lines) == 4
    assert sum(int(re.search(r"(\d+) feedback frames", ln).group(1)) for ln in lines) == 3
    mean = int(texel_counts(tables[3], W, H).astype(np.int64).sum()) / (W * H)
    assert f"next map mean {mean:.2f} spp of at most 64" in lines[-1]
