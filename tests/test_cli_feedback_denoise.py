"""The command-line front end's feedback loop through the filters: --adaptive T[,MIN[,STEP]] --samples
CAP --frames K --feedback --denoise-variance [F[,ITER[,PRE]]], optionally with --temporal [N], beside
that --reproject and --camera-step S. Frame 0 is an adaptive halves frame, every later frame a feedback
halves frame, frame k from sample_base k x CAP; --store writes the last frame's filtered image. On the
GPU the stored bytes are those of the Python chain (test_gpu_halves_chain.gpu_chain). Only the
combination with --feedback is new: every command that was refused without it stays refused with the
same text, --denoise (the plain filter) stays refused with --feedback, and nothing is stored on a
refusal."""
import re

import numpy as np
import pytest

from test_cli_temporal import read_ppm, run

W, H = 44, 27
SIZE = ("--samples", "64", "--width", str(W), "--height", str(H))
LOOP = ("--adaptive", "0.3,4,4", *SIZE, "--frames", "4")


def test_help_names_the_pairing():
    r = run("--help")
    assert r.returncode == 0 and "--feedback" in r.stdout and "halves feed the filters" in r.stdout


def test_refusals_that_stay(tmp_path):
    """Refused before any device is touched, with the text the parent gave."""
    r = run("--denoise-variance", "--adaptive", "0.3,4,4", *SIZE, "--rng", "hash", "--store", cwd=tmp_path)
    assert r.returncode == 2 and r.stderr == "--denoise-variance renders two plain halves: it cannot run with --adaptive\n"
    r = run("--denoise-variance", *LOOP, "--store", cwd=tmp_path)                          # frames, no --feedback
    assert r.returncode == 2 and r.stderr == "--denoise-variance renders two plain halves: it cannot run with --adaptive\n"
    for filt in ("--denoise", "--denoise-variance"):
        r = run("--temporal", filt, *LOOP, "--rng", "hash", "--store", cwd=tmp_path)       # no --feedback
        assert r.returncode == 2 and r.stderr == "--temporal renders plain frames: it cannot run with --adaptive\n"
    r = run("--denoise-variance", "--rng", "hash", *SIZE, "--frames", "4", "--store", cwd=tmp_path)   # no --adaptive
    assert r.returncode == 2 and r.stderr == "--denoise-variance renders one frame: it cannot run with --frames\n"
    r = run("--denoise-variance", "--feedback", "--rng", "hash", *SIZE, "--frames", "4", "--store", cwd=tmp_path)
    assert r.returncode == 2 and r.stderr == "--feedback needs --adaptive and --frames\n"
    r = run("--denoise-variance", "--feedback", "--adaptive", "0.3,4,4", *SIZE, "--store", cwd=tmp_path)
    assert r.returncode == 2 and r.stderr == "--feedback needs --adaptive and --frames\n"
    r = run("--denoise-variance", "--feedback", *LOOP, "--replay", "1", "--store", cwd=tmp_path)
    assert r.returncode == 2 and r.stderr == "--feedback plans every frame's map itself: it cannot run with --replay\n"
    assert not (tmp_path / "render.ppm").exists()


def test_the_plain_filter_stays_refused_with_feedback(tmp_path):
    r = run("--denoise", "--feedback", *LOOP, "--store", cwd=tmp_path)
    assert r.returncode == 2 and r.stderr == "--denoise renders one frame: it cannot run with --frames\n"
    r = run("--denoise", "--temporal", "--feedback", *LOOP, "--store", cwd=tmp_path)
    assert r.returncode == 2 and r.stderr == "--temporal renders plain frames: it cannot run with --adaptive\n"
    r = run("--denoise", "--denoise-variance", "--feedback", *LOOP, "--store", cwd=tmp_path)
    assert r.returncode == 2 and "cannot run with --denoise" in r.stderr
    assert not (tmp_path / "render.ppm").exists()


def test_refusals_of_the_pairing(tmp_path):
    """K x CAP past 32 bits, in --temporal's message form; what the flags beside it refuse on their own."""
    big = ("--adaptive", "0.3,4,4", "--samples", "65536", "--width", str(W), "--height", str(H), "--frames", "65536", "--store")
    r = run("--denoise-variance", "--feedback", *big, cwd=tmp_path)
    assert r.returncode == 2 and "--feedback" in r.stderr and "--frames 65536 x --samples 65536 exceeds 32 bits" in r.stderr
    r = run("--denoise-variance", "--temporal", "--feedback", *big, cwd=tmp_path)
    assert r.returncode == 2 and "--frames 65536 x --samples 65536 exceeds 32 bits" in r.stderr
    r = run("--denoise-variance", "--feedback", *LOOP, "--reproject", "--store", cwd=tmp_path)       # no --temporal
    assert r.returncode == 2 and "--reproject" in r.stderr and "--temporal" in r.stderr
    r = run("--denoise-variance", "--feedback", *LOOP, "--camera-step", "0.05", "--store", cwd=tmp_path)
    assert r.returncode == 2 and "--camera-step" in r.stderr and "--temporal" in r.stderr
    r = run("--denoise-variance", "--feedback", *LOOP, "--gpus", "2", "--store", cwd=tmp_path)
    assert r.returncode == 2 and "--gpus 2" in r.stderr
    r = run("--denoise-variance", "--feedback", *LOOP, "--rng", "stream", "--store", cwd=tmp_path)
    assert r.returncode == 2 and "--rng stream" in r.stderr
    r = run("--denoise-variance", "--temporal", "1", "--feedback", *LOOP, "--store", cwd=tmp_path)
    assert r.returncode == 2 and "max_history" in r.stderr
    r = run("--denoise-variance", "16,9", "--feedback", *LOOP, "--store", cwd=tmp_path)
    assert r.returncode == 2 and "--denoise-variance" in r.stderr
    assert not (tmp_path / "render.ppm").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("stage", [(), ("--temporal", "8", "--reproject", "--camera-step", "0.05"), ("--temporal", "8")],
                         ids=["filter", "reprojected", "in-place"])
def test_store_equals_the_python_chain(tmp_path, oracle, stage):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rtvk
    from test_gpu_halves_chain import gpu_chain
    r = run(*LOOP, "--feedback", "--denoise-variance", "16", *stage, "--store", cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("duration_per_frame")]
    assert lines and sum(int(re.search(r"\((\d+) frames", ln).group(1)) for ln in lines) == 4
    assert sum(int(re.search(r"(\d+) feedback frames", ln).group(1)) for ln in lines) == 3
    assert "variance-guided denoise: 16 feature samples" in lines[-1]
    moved = "--reproject" in stage
    assert ("temporal history 8" in lines[-1]) == bool(stage) and ("reprojected" in lines[-1]) == moved
    assert ("temporal history 8 reprojected" in lines[-1]) == moved
    img = read_ppm(tmp_path / "render.ppm", W, H)
    res = gpu_chain(rtvk, torch, oracle, 4, start=None, temporal=bool(stage), reproject=moved,
                    s=0.05 if moved else 0.0, thr=0.3, lo=4, step_spp=4, cap=64, feature_samples=16, history=8)
    np.testing.assert_array_equal(img, res[3]["out"][..., :3])
    # the loop did what it says: several counts in the last frame, and the filter changed the image
    assert len(np.unique(res[3]["half"])) >= 3
    assert not np.array_equal(res[3]["out"], oracle.resolve(res[3]["acc"], 1))
    if stage:
        assert (res[3]["hlen"] >= 3).any()
