"""The integer rules of device-planned sample maps under AddressSanitizer +
UndefinedBehaviorSanitizer: the feedback rule (csrc/rt_sample_map_feedback.h), the block hand-out the
host plan and the device share (csrc/rt_hand_out.h) and the host twin of the device planner's unit
(csrc/rt_sample_map.cpp device_unit). tests/native/sample_map_feedback_main.cpp is a stand-alone
program with its own main, compiled here with the library's source file and run as a child process;
any sanitizer report or failed check fails the test. CPU only (g++); nothing is loaded into python."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "ray-tracing-gpu-vulkan_amd" / "csrc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


@pytest.mark.timeout(300)
def test_feedback_rules_clean_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = tmp_path / "sample_map_feedback_main"
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", f"-I{ROOT / 'include'}", *SAN, "-o", str(exe),
                        str(ROOT / "tests" / "native" / "sample_map_feedback_main.cpp"), str(CSRC / "rt_sample_map.cpp")],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1",
                            "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "checks passed (ASan + UBSan)" in r.stdout
    assert "runtime error" not in log and "AddressSanitizer" not in log, log[-4000:]
