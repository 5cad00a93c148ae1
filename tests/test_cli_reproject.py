"""The command-line front end's --reproject and --camera-step S, beside --temporal: frame k's camera
stands at (13 + S k, 11, -3 + 2 S k) and looks at the origin, and with --reproject every frame renders
its motion plane against the frame before and the history follows it. Both are refused without
--temporal, with a message naming the option, before anything renders. On the GPU the stored bytes are
those of the Python chain of test_gpu_temporal_reproject.py on the static scene."""
import numpy as np
import pytest

from test_cli_temporal import read_ppm, run


def test_help_lists_the_flags():
    r = run("--help")
    assert r.returncode == 0 and "--reproject" in r.stdout and "--camera-step" in r.stdout


def test_refusals(tmp_path):
    size = ("--samples", "4", "--width", "64", "--height", "40", "--store")
    loop = ("--frames", "2", "--rng", "hash")
    r = run("--reproject", "--denoise-variance", "--rng", "hash", *size, cwd=tmp_path)
    assert r.returncode != 0 and "--reproject" in r.stderr and "--temporal" in r.stderr
    r = run("--reproject", "--frames", "2", *size, cwd=tmp_path)
    assert r.returncode != 0 and "--reproject" in r.stderr and "--temporal" in r.stderr
    r = run("--camera-step", "0.1", "--denoise", "--rng", "hash", *size, cwd=tmp_path)
    assert r.returncode != 0 and "--camera-step" in r.stderr and "--temporal" in r.stderr
    for bad in ("x", "0.1x", "nan", "inf"):
        r = run("--temporal", "--reproject", "--camera-step", bad, "--denoise", *loop, *size, cwd=tmp_path)
        assert r.returncode != 0 and "--camera-step" in r.stderr, bad
    r = run("--temporal", "--reproject", "--denoise", *loop, *size, "--camera-step", cwd=tmp_path)      # no value
    assert r.returncode != 0 and "--camera-step" in r.stderr
    # --temporal's own refusals hold beside --reproject
    r = run("--temporal", "--reproject", *loop, *size, cwd=tmp_path)                                     # no filter
    assert r.returncode != 0 and "--denoise" in r.stderr
    assert not (tmp_path / "render.ppm").exists()


@pytest.mark.gpu
def test_reproject_store_equals_the_python_chain(tmp_path, oracle):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import rtvk
    from test_gpu_temporal_reproject import CHAIN, gpu_chain
    W, H = CHAIN["W"], CHAIN["H"]
    r = run("--denoise-variance", str(CHAIN["F"]), "--temporal", str(CHAIN["N"]), "--reproject", "--camera-step", str(CHAIN["s"]),
            "--rng", "hash", "--frames", "3", "--samples", str(CHAIN["spp"]), "--width", str(W), "--height", str(H), "--store",
            cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "duration_per_frame" in r.stdout and f"temporal history {CHAIN['N']} reprojected" in r.stdout
    img = read_ppm(tmp_path / "render.ppm", W, H)
    ins, outs = gpu_chain(rtvk, torch, oracle, dt=0.0)
    assert (outs[2][4] == 3).mean() > 0.5 and np.abs(ins[2][4][..., 0] - (np.arange(W) + 0.5)[None, :]).max() > 0.5
    np.testing.assert_array_equal(img, outs[2][3][..., :3])
    # without --reproject the same camera path gives another image: the history stayed in place
    r = run("--denoise-variance", str(CHAIN["F"]), "--temporal", str(CHAIN["N"]), "--camera-step", str(CHAIN["s"]),
            "--rng", "hash", "--frames", "3", "--samples", str(CHAIN["spp"]), "--width", str(W), "--height", str(H), "--store",
            cwd=tmp_path)
    assert r.returncode == 0 and "reprojected" not in r.stdout
    assert not np.array_equal(read_ppm(tmp_path / "render.ppm", W, H), img)
