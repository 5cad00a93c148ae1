"""The command-line front end's refusals, as a table: tests/golden/cli_refusals.json holds, for --help
and for argument lists that exit before any device is touched, the exit code, stdout and stderr the
front end gave when the table was recorded. Every row must come back byte for byte, and nothing may be
stored. The rows hit every message main() can print on stderr but "no HIP device" (a device changes
it) and the two runtime-failure lines, and where the order of the checks decides which message wins,
a row shows the winner.

    python tests/test_cli_refusal_table.py <path to rt_mi355x_cli>

runs ROWS through that binary and rewrites the fixture."""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
CLI = HERE.parent / "ray-tracing-gpu-vulkan_amd" / "bin" / "rt_mi355x_cli"
FIXTURE = HERE / "golden" / "cli_refusals.json"

S = ["--samples", "4", "--width", "64", "--height", "40", "--store"]
HASH = ["--rng", "hash"]
LOOP = ["--frames", "2", *HASH]
AD = ["--adaptive", "0.3,4,4"]
FB = [*AD, "--frames", "4", "--feedback"]
BIG = ["--frames", "65536", "--samples", "65536", "--width", "64", "--height", "40", "--store"]

ROWS = [
    ["--help"],
    ["--store", "--help"],
    # ---- values that do not parse
    ["--adaptive"], ["--adaptive", "x", *S], ["--adaptive", "0.2,x", *S], ["--adaptive", "0.2,8,", *S], ["--adaptive", "0.2x", *S],
    ["--denoise", "4,x", *HASH, *S], ["--denoise", "4x", *HASH, *S],
    ["--denoise-variance", "4,3,x", *HASH, *S], ["--denoise-variance", "4,,2", *HASH, *S],
    ["--temporal", "8x", "--denoise", *LOOP, *S],
    ["--camera-step"], ["--camera-step", "nan", *S], ["--camera-step", "inf", *S], ["--camera-step", "0.1x", *S],
    ["--camera-step", "--store"],
    ["--rng"], ["--rng", "lcg", *S],
    ["--map-launch"], ["--map-launch", "two", *S],
    ["--samples"], ["--width", "-1"], ["--height", ""], ["--gpus", "4294967296"], ["--frames", "x"], ["--replay", "1.5"],
    ["--bogus", "--replay", "1", *S],                     # an unknown argument is named and ignored
    ["--replay", "1", "extra", "--bogus", *S],
    # ---- the loop flags
    ["--replay", "1", *S], ["--replay", "1", *AD, *S], ["--replay", "1", "--frames", "3", *S],
    ["--feedback", *S], ["--feedback", *AD, *S], ["--feedback", "--frames", "3", *S],
    ["--replay", "1", "--feedback", *S],                  # --replay's check comes first
    [*FB, "--replay", "1", *S],
    ["--map-launch", "one", *S], ["--map-launch", "one", *AD, "--frames", "3", *S],
    ["--map-launch", "one", *FB, *S],
    [*FB, "--replay", "1", "--map-launch", "one", *S],    # --feedback with --replay wins over --map-launch
    # ---- --adaptive
    [*AD, "--rng", "stream", *S], [*AD, "--gpus", "2", *S], [*AD, "--rng", "stream", "--gpus", "2", *S],
    [*AD, "--gpus", "2", "--reproject", *S],              # --adaptive's checks come before --reproject's
    [*AD, "--gpus", "2", "--denoise", *S],
    # ---- --reproject and --camera-step
    ["--reproject", "--denoise", *HASH, *S], ["--reproject", *S],
    ["--camera-step", "0.05", "--denoise", *HASH, *S], ["--camera-step", "0", *S],
    ["--reproject", "--camera-step", "0.05", *S],
    # ---- --temporal
    ["--temporal", *LOOP, *S], ["--temporal", "4", *S],
    ["--temporal", "--denoise", *HASH, *S], ["--temporal", "--denoise-variance", *HASH, *S],
    ["--temporal", "--denoise", *LOOP, "--gpus", "2", *S], ["--temporal", "--denoise-variance", *LOOP, "--gpus", "2", *S],
    ["--temporal", "--denoise", *LOOP, *AD, *S], ["--temporal", "--denoise-variance", *LOOP, *AD, *S],
    ["--temporal", "--denoise", *FB, *S],                 # the plain filter stays refused with --feedback
    ["--temporal", "--denoise", "--frames", "2", *S], ["--temporal", "--denoise-variance", "--frames", "2", "--rng", "stream", *S],
    ["--temporal", "--denoise", *HASH, *BIG], ["--temporal", "--denoise-variance", *HASH, *BIG],
    ["--temporal", "--denoise", "--frames", "2", "--gpus", "2", *S],   # --gpus before the stream
    ["--temporal", "1", "--denoise", *HASH, *BIG],        # the 32-bit check before rt_temporal_check
    ["--temporal", "0", "--denoise", *LOOP, *S], ["--temporal", "1", "--denoise-variance", *LOOP, *S],
    ["--temporal", "65536", "--denoise", *LOOP, *S],
    ["--temporal", "1", "--denoise-variance", *FB, *S],
    ["--temporal", "--denoise", "0", *LOOP, *S],          # rt_temporal_check sees the filter's F before the filter does
    ["--temporal", "--denoise-variance", "0", *LOOP, *S],
    # ---- --denoise-variance
    ["--denoise-variance", "--denoise", *HASH, *S], ["--temporal", "--denoise", "--denoise-variance", *LOOP, *S],
    ["--denoise", "--denoise-variance", *FB, *S],
    ["--denoise-variance", *AD, *HASH, *S], ["--denoise-variance", *AD, "--frames", "4", *S],
    ["--denoise-variance", *HASH, "--gpus", "2", *S], ["--denoise-variance", *FB, "--gpus", "2", *S],
    ["--denoise-variance", *LOOP, *S], ["--denoise-variance", *LOOP, "--gpus", "2", *S],
    ["--denoise-variance", *AD, "--feedback", *BIG],      # the 32-bit message in --feedback's wording ...
    ["--denoise-variance", "--temporal", *AD, "--feedback", *BIG],   # ... and, with --temporal, in --temporal's
    ["--denoise-variance", *S], ["--denoise-variance", "--rng", "stream", *S],
    ["--denoise-variance", "--frames", "2", *S],          # --frames before the stream
    ["--denoise-variance", *HASH, "--samples", "5", "--width", "64", "--height", "40", "--store"],
    ["--denoise-variance", *FB, "--samples", "5", "--width", "64", "--height", "40", "--store"],
    ["--denoise-variance", "--samples", "5", "--width", "64", "--height", "40", "--store"],   # the stream before the odd count
    ["--denoise-variance", "16,9", *HASH, *S], ["--denoise-variance", "0", *HASH, *S], ["--denoise-variance", "16,3,9", *HASH, *S],
    ["--denoise-variance", "16,9", *FB, *S],
    # ---- --denoise
    ["--denoise", *HASH, "--gpus", "2", *S],
    ["--denoise", *LOOP, *S], ["--denoise", *FB, *S], ["--denoise", *LOOP, "--gpus", "2", *S],
    ["--denoise", *S], ["--denoise", "--rng", "stream", *S], ["--denoise", "--frames", "2", *S],
    ["--denoise", "0", *HASH, *S], ["--denoise", "16,9", *HASH, *S], ["--denoise", "16,0", *AD, *S],
]


def run_row(cli, argv):
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([str(cli), *argv], capture_output=True, text=True, cwd=tmp, timeout=60)
        stored = (Path(tmp) / "render.ppm").exists()
    return {"argv": argv, "returncode": r.returncode, "stdout": r.stdout, "stderr": r.stderr}, stored


TABLE = json.loads(FIXTURE.read_text()) if FIXTURE.exists() else []


def test_the_fixture_holds_the_rows():
    assert [row["argv"] for row in TABLE] == ROWS


@pytest.mark.parametrize("row", TABLE, ids=[str(i) for i in range(len(TABLE))])
def test_row(row):
    got, stored = run_row(CLI, row["argv"])
    assert got == row
    assert not stored


if __name__ == "__main__":
    rows = []
    for argv in ROWS:
        row, stored = run_row(Path(sys.argv[1]).resolve(), argv)
        assert not stored and (row["returncode"] == 2 or "--help" in argv), row
        rows.append(row)
    FIXTURE.write_text(json.dumps(rows, indent=1) + "\n")
    print(f"{len(rows)} rows -> {FIXTURE}")
