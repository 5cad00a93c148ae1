"""The hand-over of the two halves without a GPU: rt_half_outputs_check accepts a
valid struct and refuses every case of the header's list by name, the ctypes layout of
rt_half_outputs, and the CPU model (tests/halves_sim.py) on a small synthetic cube. The check compares
addresses and reads nothing, so plain integers stand in for device pointers."""
import ctypes

import numpy as np
import pytest

import halves_sim as hs


@pytest.fixture(scope="module")
def rtvk():
    import rtvk as m
    m.load_library()
    return m


def halves_of(rtvk, a=0x1000, b=0x2000, h=0x3000, reserved=None):
    s = rtvk.abi.HalfOutputs()
    s.accum_a, s.accum_b, s.half_count, s.reserved = a, b, h, reserved
    return s


def test_check_accepts(rtvk):
    rtvk.half_outputs_check(halves_of(rtvk), 0x4000)
    rtvk.half_outputs_check(halves_of(rtvk, h=None), 0x4000)     # half_count is optional
    rtvk.half_outputs_check(halves_of(rtvk), None)               # the frame call refuses a NULL accum itself
    rtvk.half_outputs_check(halves_of(rtvk, h=0x1000), 0x4000)   # only the float4 planes are compared


@pytest.mark.parametrize("kw,accum,field", [
    (None, 0x4000, "halves is NULL"),
    (dict(a=None), 0x4000, "accum_a is NULL"),
    (dict(b=None), 0x4000, "accum_b is NULL"),
    (dict(a=None, b=None), 0x4000, "accum_a is NULL"),
    (dict(reserved=0x10), 0x4000, "reserved"),
    (dict(a=0x1000, b=0x1000), 0x4000, "accum_a and accum_b"),
    (dict(a=0x4000), 0x4000, "accum_a is accum_rgba32f"),
    (dict(b=0x4000), 0x4000, "accum_b is accum_rgba32f"),
])
def test_check_refuses_by_name(rtvk, kw, accum, field):
    with pytest.raises(rtvk.RtError) as e:
        rtvk.half_outputs_check(None if kw is None else halves_of(rtvk, **kw), accum)
    assert e.value.code == -1 and field in str(e.value), (field, str(e.value))


def test_struct_layout_and_bindings(rtvk):
    H = rtvk.abi.HalfOutputs
    assert ctypes.sizeof(H) == 4 * ctypes.sizeof(ctypes.c_void_p) == 32
    assert [(n, getattr(H, n).offset) for n, _ in H._fields_] == [("accum_a", 0), ("accum_b", 8), ("half_count", 16),
                                                                  ("reserved", 24)]
    lib = rtvk.load_library()
    plain = rtvk.abi.EXPORTS["rt_render_adaptive_device"][1]
    halves = rtvk.abi.EXPORTS["rt_render_adaptive_halves_device"][1]
    assert halves[:-2] == plain[:-1] and halves[-1] == plain[-1] and halves[-2] == ctypes.POINTER(H)
    plain = rtvk.abi.EXPORTS["rt_render_sample_map_feedback_device"][1]
    halves = rtvk.abi.EXPORTS["rt_render_sample_map_feedback_halves_device"][1]
    assert halves[:-2] == plain[:-1] and halves[-1] == plain[-1] and halves[-2] == ctypes.POINTER(H)
    for name in ("rt_half_outputs_check", "rt_render_adaptive_halves_device", "rt_render_sample_map_feedback_halves_device"):
        assert hasattr(lib, name)
    assert lib.rt_abi_version() == 2
    # the timing entry point refuses a NULL context before it touches a device
    assert lib.rt_debug_adaptive_resolve(None, 8, 8, 2, None, None, None, None, None) == -1
    assert b"rt_debug_adaptive_resolve" in lib.rt_last_error()


def test_accum_a_without_accum_b_is_a_value_error(rtvk):
    for a, b, h in ((object(), None, None), (None, object(), None), (None, None, object())):
        with pytest.raises(ValueError, match="accum_a and accum_b"):
            rtvk.Renderer._half_outputs(a, b, h, 8, 8)
    assert rtvk.Renderer._half_outputs(None, None, None, 8, 8) is None


def synthetic_cube(seed, S=12, H=11, W=13):
    q = np.random.default_rng(seed).integers(0, 1 << 24, (S, H, W, 3), dtype=np.int64)
    q[:, :, :8] >>= 6        # a quiet tile column: it converges early
    return q


def test_model_feedback_planes():
    Q = synthetic_cube(1)
    table = [0, 4, 12, 2]   # 2 x 2 tiles, ragged both ways
    A, B, half = hs.feedback_planes(Q, table)
    assert np.all(A[:8, :8] == 0) and np.all(B[:8, :8] == 0) and np.all(half[:8, :8] == 0)
    np.testing.assert_array_equal(A[:8, 8:], Q[:2, :8, 8:].sum(axis=0))
    np.testing.assert_array_equal(B[:8, 8:], Q[2:4, :8, 8:].sum(axis=0))
    np.testing.assert_array_equal(A[8:, :8] + B[8:, :8], Q[:12, 8:, :8].sum(axis=0))
    assert half[9, 3] == 6 and half[10, 12] == 1
    a, b, h = hs.feedback_halves(Q, table)
    assert a.dtype == np.float32 and np.all(a[..., 3] == 1) and np.all(b[..., 3] == 1)
    assert np.all(a[:8, :8, :3] == 0)
    # one rounding: the float of the exact rational
    np.testing.assert_array_equal(a[..., :3].astype(np.float64), (A / 2.0 ** 24).astype(np.float32).astype(np.float64))
    assert hs.even_table([0, 1, 2, 7, 64]) == [0, 2, 2, 8, 64]


def test_model_adaptive_planes_against_simulate():
    import adaptive_sim as sim
    Q = synthetic_cube(2, S=32)
    for thr in (0, 3000, 1 << 20):
        counts, _ = sim.simulate(Q, 4, 6, 32, thr)
        A, B, got = hs.adaptive_planes(Q, 4, 6, 32, thr)
        np.testing.assert_array_equal(got, counts)
        for y, x in ((0, 0), (3, 9), (10, 12)):
            n = int(counts[y, x])
            np.testing.assert_array_equal(A[y, x] + B[y, x], Q[:n, y, x].sum(axis=0))
    # threshold 16: one pass, A = the first min / 2 samples, B = the next
    np.testing.assert_array_equal(A, Q[:2].sum(axis=0))
    np.testing.assert_array_equal(B, Q[2:4].sum(axis=0))
    # threshold 0: A holds the first half of every pass (4, then 6, 6, 6, 6, 4)
    A, B, got = hs.adaptive_planes(Q, 4, 6, 32, 0)
    assert np.all(got == 32)
    first = [s for d, k in ((0, 4), (4, 6), (10, 6), (16, 6), (22, 6), (28, 4)) for s in range(d, d + k // 2)]
    np.testing.assert_array_equal(A, Q[first].sum(axis=0))
