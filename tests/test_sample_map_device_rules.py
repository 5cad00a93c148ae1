"""The host side of device-planned sample maps on the CPU: the feedback rule
(rt_sample_map_feedback_count) at its anchors and against a Python restatement on
adaptive_sim.converged, the block hand-out the host plan and the device share (rt_debug_hand_out)
against rt_debug_launch_plan, and the host twin of the device planner's unit
(rt_sample_map_device_unit). No GPU."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_sim as sim   # noqa: E402
from test_launch_plan import HASH, make_inputs   # noqa: E402

Q16 = 1 << 16


@pytest.fixture(scope="module")
def lib():
    import rtvk
    rtvk.load_library()
    return rtvk


def restated(E, S, n, m, thr, lo, hi):
    if n == 0:
        return 0
    if not sim.converged(E, S, n, m, thr):
        return min(hi, 2 * n)
    if sim.converged(E, S, n, m, thr >> 1):
        return max(lo, (n // 2 + 1) & ~1)
    return n


def test_rule_anchors(lib):
    f = lib.sample_map_feedback_count
    for n in (2, 4, 6, 10, 16, 30, 32, 34, 62, 64, 1000, 1 << 18, 1 << 19):
        for E, S in ((0, 0), (12345, 67890), (1 << 50, 1 << 51), ((1 << 56) - 1, (1 << 56) - 1)):
            assert f(E, S, n, 64, 0, 4, 64) == min(64, 2 * n)                      # threshold 0: nothing converges
            assert f(E, S, n, 64, 16 * Q16, 4, 64) == max(4, (n // 2 + 1) & ~1)    # threshold 16: everything does, at 8 too
    for thr in (0, 1, 13107, 16 * Q16, 0xffffffff):
        assert f(5, 9, 0, 64, thr, 4, 64) == 0                                     # n = 0 stays 0
    assert f(1, 1, 1 << 19, 64, 0, 2, 1 << 19) == 1 << 19                          # the clamp at the top ...
    assert f(1, 1, 48, 64, 0, 4, 64) == 64
    assert f(0, 1, 4, 64, 16 * Q16, 4, 64) == 4 and f(0, 1, 2, 1, 16 * Q16, 2, 2) == 2   # ... and at the bottom
    assert f(0, 1, 6, 64, 16 * Q16, 2, 64) == 4 and f(0, 1, 12, 64, 16 * Q16, 2, 64) == 6   # n / 2 rounded up to even
    # between the two thresholds the count stays: E / S' = 0.15 against 0.2 and 0.1
    n, m = 32, 64
    guard = n * 3 * m * Q16
    S = 10 * guard
    E = int(0.15 * (S + guard) / 2)
    thr = lib.threshold_q16(0.2)
    assert sim.converged(E, S, n, m, thr) and not sim.converged(E, S, n, m, thr >> 1)
    assert f(E, S, n, m, thr, 4, 64) == 32
    assert f(2 * E, S, n, m, thr, 4, 64) == 64 and f(E // 2, S, n, m, thr, 4, 64) == 16


def test_rule_two_word_compare(lib):
    """E, S near 2^56: 2^17 E and thr S' exceed 64 bits."""
    big = (1 << 56) - 1
    for thr in (0, 1, 13107, Q16, 1 << 17, (1 << 17) + 1, 1 << 18, 16 * Q16, 0xffffffff):
        for E in (big, big - 1, big // 2, big // 2 + 1, 1 << 47, (1 << 47) - 1):
            for S in (big, big - 1, big // 2, 1 << 55, 0):
                assert lib.sample_map_feedback_count(E, S, 32, 64, thr, 4, 64) == restated(E, S, 32, 64, thr, 4, 64)


def test_rule_against_the_python_restatement(lib):
    rng = np.random.default_rng(20260101)
    seen = set()
    for _ in range(4000):
        S = int(rng.integers(0, 1 << 56)) >> int(rng.integers(0, 40))
        E = (int(rng.integers(0, S + 1)) >> int(rng.integers(0, 8))) if S else 0
        n = 2 * int(rng.integers(0, 1 << int(rng.integers(1, 19))))   # every magnitude: below and above max_spp
        m = int(rng.integers(1, 65))
        thr = int(rng.integers(0, 1 << 32)) >> int(rng.integers(0, 20))
        lo = 2 + 2 * int(rng.integers(0, 32))
        hi = lo + 2 * int(rng.integers(0, 1000))
        want = restated(E, S, n, m, thr, lo, hi)
        assert lib.sample_map_feedback_count(E, S, n, m, thr, lo, hi) == want
        seen.add("zero" if n == 0 else "up" if want > n else "down" if want < n else "keep")
    assert seen >= {"up", "down", "keep"}


def test_rule_refusals(lib):
    L = lib.load_library()
    nxt = ctypes.c_uint32(0xdead)
    for args in ((1 << 56, 0, 2, 1, 0, 2, 4), (0, 1 << 56, 2, 1, 0, 2, 4), (0, 0, (1 << 19) + 1, 1, 0, 2, 4),
                 (0, 0, 2, 0, 0, 2, 4), (0, 0, 2, 65, 0, 2, 4), (0, 0, 2, 1, 0, 0, 4), (0, 0, 2, 1, 0, 3, 4),
                 (0, 0, 2, 1, 0, 2, 5), (0, 0, 2, 1, 0, 6, 4), (0, 0, 2, 1, 0, 2, (1 << 19) + 2)):
        assert L.rt_sample_map_feedback_count(*args, ctypes.byref(nxt)) == -1 and nxt.value == 0xdead, args
    assert L.rt_sample_map_feedback_count(0, 0, 2, 1, 0, 2, 4, None) == -1


FULL_GRID_WAVES = 256 * 2 * 768 // 64   # the persistent grid of the walk forms on 256 CUs


@pytest.mark.parametrize("reserve", [0, 640, 8192])
@pytest.mark.parametrize("blocks", [1, 63, 127, 128, 129, 203])
def test_hand_out_is_the_launch_plans(lib, blocks, reserve):
    """A launch of `blocks` blocks (a band of that many tiles at 1 spp is one: one chunk per tile): the
    shared inline gives the plan's n_block_units and first_blocks from the plan's own grid, and the
    same from the full persistent grid, which is what the device assumes."""
    v = make_inputs(lib, "canon", (8 * blocks, 8, 0), 1, HASH, 0, tune=dict(refill_reserve=reserve))
    p = lib.launch_plan(v)
    assert p.n_units == 64 * blocks and p.chunks == 1
    want = (p.n_block_units, p.first_blocks)
    assert lib.hand_out(p.n_units, reserve, p.grid * p.block // 64) == want
    assert lib.hand_out(p.n_units, reserve, FULL_GRID_WAVES) == want
    assert want[0] == (max(0, 64 * blocks - reserve) & ~63) and want[1] == want[0] // 64


@pytest.mark.parametrize("reserve", [0, 640, 8192])
def test_hand_out_of_an_empty_table(lib, reserve):
    """0 blocks: no host launch has none (the host skips it); the device's record is all zero."""
    assert lib.hand_out(0, reserve, FULL_GRID_WAVES) == (0, 0)


COUNTS = [0, 1, 2, 7, 8, 64, 64, 3, 100, 65]


def blocks_at(counts, cap, unit):
    return sum(-(-min(c, cap) // unit) for c in counts)


def test_device_unit(lib):
    f = lib.sample_map_device_unit
    assert f(COUNTS, 64, 3) == 3 and f(COUNTS, 64) == 32 and f(COUNTS, 4096) == 128           # no doubling
    assert lib.sample_map_device_capacity(10, 64, 3) == 10 * 22 and lib.sample_map_device_capacity(1 << 20, 1 << 19, 1) == 1 << 22
    at3 = blocks_at(COUNTS, 64, 3)
    assert f(COUNTS, 64, 3, capacity=at3) == 3
    assert f(COUNTS, 64, 3, capacity=at3 - 1) == 6                                             # one doubling
    assert blocks_at(COUNTS, 64, 6) <= at3 - 1
    assert f(COUNTS, 64, 1, capacity=9) == 64                                                  # several: one block per tile
    assert f(COUNTS, 1 << 19, 3, capacity=9) == 192
    assert f([1 << 19, (1 << 19) + 5, 1], 1 << 19, 3, capacity=3) == 1 << 19                   # held at 2^19
    assert f([], 64) == 32
    # the table at that unit is the host planner's of the clamped counts
    got = lib.sample_map_block_plan([min(c, 64) for c in COUNTS], 0, 6)
    assert len(got["blocks"]) == blocks_at(COUNTS, 64, 6) and got["unit_samples"] == 6


def test_device_unit_refusals(lib):
    from rtvk import RtError
    L = lib.load_library()
    c = np.asarray(COUNTS, np.uint32)
    used = ctypes.c_uint32(0xdead)
    assert L.rt_sample_map_device_unit(c.ctypes.data, len(c), 64, 1, 8, ctypes.byref(used)) == -1   # nine non-zero tiles
    assert b"no unit fits" in L.rt_last_error() and used.value == 0xdead
    assert L.rt_sample_map_device_unit(None, 3, 64, 1, 8, ctypes.byref(used)) == -1
    assert L.rt_sample_map_device_unit(c.ctypes.data, len(c), (1 << 19) + 1, 1, 100, ctypes.byref(used)) == -1
    assert L.rt_sample_map_device_unit(c.ctypes.data, len(c), 64, (1 << 19) + 1, 100, ctypes.byref(used)) == -1
    assert used.value == 0xdead
    with pytest.raises(RtError):
        lib.sample_map_device_unit(COUNTS, 64, 1, capacity=8)
