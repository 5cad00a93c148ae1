"""normalize's length and reciprocal from one v_rsq_f32 (csrc/rt_device_math.h sqrt_rcp_cr) against
the form it replaced, v_sqrt_f32 then v_rcp_f32 with their exact corrections.

Bar: bit-exact, any NaN equal to any NaN. The frames' parity tests hold the kernels to the oracle bit
for bit; these two hold the primitive itself, over every binary32 input and over the vectors a frame
is least likely to draw."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    if not t.cuda.is_available():
        pytest.skip("no GPU")
    return t


@pytest.fixture(scope="module")
def rtvk(torch):
    import rtvk as m
    return m


def test_normalize_rsq_exhaustive(rtvk):
    """Every one of the 2^32 binary32 x: the new length equals sqrtf(x), the new reciprocal
    1.0f / sqrtf(x), and the square root alone by the same chain sqrtf(x). At most 4096 x of
    [2^-100, 2^100] may take the rare branch (the old form): the check must not pass by sending
    everything there. The branch needs the lengths with an all-ones mantissa, 2 x per pair of
    binades, 200 in range."""
    from rtvk import abi
    out = (ctypes.c_uint64 * 4)()
    abi.check(rtvk.load_library().rt_debug_exact_normalize_exhaustive(0, out))
    print(f"length {out[0]}, reciprocal {out[1]}, sqrt alone {out[2]} mismatches; {out[3]} in-range x on the rare branch")
    assert tuple(out)[:3] == (0, 0, 0), f"length {out[0]}, reciprocal {out[1]}, sqrt alone {out[2]} mismatches"
    assert out[3] <= 4096, f"{out[3]} in-range inputs took the rare branch"


def _dot_f32(x, y):
    """fma(0.5, 0.5, fma(y, y, x * x)) in binary32 (products of binary32 values are exact in binary64)."""
    with np.errstate(all="ignore"):
        xx = x * x
        d = (y.astype(np.float64) * y + xx).astype(np.float32)
        return (np.float64(0.25) + d).astype(np.float32)


def _all_ones_len_vectors(rng):
    """(x, y) whose dot with z = 0.5 is an x' with sqrtf(x') = 1.11..1 x 2^k, for several k."""
    xs, ys = [], []
    for k in (0, 1, 2, 3, 7, 20, 33, 41, 49):          # len just below 2^(k+1): dot just below 4^(k+1)
        top = np.float32(4.0) ** np.float32(k + 1)
        t = top.view(np.uint32) - np.arange(1, 5, dtype=np.uint32)
        t = t.view(np.float32)
        t = t[((np.sqrt(t).view(np.uint32) + 1) & 0x7fffff) == 0]
        assert len(t) == 2, (k, t)
        for target in t:
            y = (rng.uniform(0, 0.99, 400) * np.sqrt(np.float64(target) - 0.25)).astype(np.float32)
            x = np.sqrt(np.float64(target) - 0.25 - y.astype(np.float64) ** 2).astype(np.float32)
            hit = _dot_f32(x, y) == target
            xs.append(x[hit][:12])
            ys.append(y[hit][:12])
    return np.concatenate(xs), np.concatenate(ys)


def test_normalize_awkward_vectors(rtvk):
    """rt_debug_math op 10 (normalize(x, y, 0.5).y as the kernels compute it) against op 11 (the same by
    v_sqrt_f32 and v_rcp_f32) on about 4 000 vectors: zeros and signed zeros, denormals, 1e-20 and
    1e19 (the squares underflow, the dot leaves [2^-100, 2^100] upwards), NaN and infinities,
    near-axis vectors, dots whose length has an all-ones mantissa, random unit-scale vectors and the
    24-bit lattice of random_unit_vector. The ops fix z = 0.5, so no dot of these lies below 0.25:
    the zero and underflowing dots themselves are the exhaustive test's. In the default build
    (RT_NORMALIZE_RSQ 0) normalize is the old form and op 10 is op 11; the comparison
    bites in a build with -DRT_NORMALIZE_RSQ=1 (passed there), the numpy reference in both."""
    from rtvk import abi
    rng = np.random.default_rng(31)
    f = np.float32
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -3e-39, 1.17549435e-38, 1e-20, -1e-20, 1e19, -1e19,
                        3e38, np.inf, -np.inf, np.nan, 1e-8, -1e-8, 1.0, -1.0, 0.5], f)
    sx, sy = [a.ravel() for a in np.meshgrid(special, special)]                     # 400: every pair
    nx = rng.choice(np.array([1e-8, -1e-8, 1e-12, 3e-7, 0.0], f), 300)              # near the z axis,
    ny = rng.choice(np.array([1e-8, -1e-8, 1e-12, 3e-7], f), 300)
    ax = (rng.uniform(1e3, 1e6, 300) * rng.choice([-1, 1], 300)).astype(f)          # and near x and y
    ay = rng.choice(np.array([1e-8, -1e-8, 0.0, 1e-3], f), 300)
    ox, oy = _all_ones_len_vectors(rng)
    assert len(ox) >= 100, len(ox)
    ux, uy = rng.standard_normal(1000).astype(f), rng.standard_normal(1000).astype(f)
    lx = (rng.integers(0, 1 << 24, 1500).astype(f) * f(2.0 ** -24) * f(2) + f(-1)).astype(f)
    ly = (rng.integers(0, 1 << 24, 1500).astype(f) * f(2.0 ** -24) * f(2) + f(-1)).astype(f)
    x = np.concatenate([sx, nx, ax, ay, ox, ux, lx]).astype(f)
    y = np.concatenate([sy, ny, ay, ax, oy, uy, ly]).astype(f)
    pairs = np.ascontiguousarray(np.stack([x, y], 1), f)
    got = {}
    for op in (10, 11):
        out = np.zeros(len(x), f)
        abi.check(rtvk.load_library().rt_debug_math(0, op, pairs.ctypes.data, out.ctypes.data, len(x)))
        got[op] = out
    new, old = got[10], got[11]
    same = (new.view(np.uint32) == old.view(np.uint32)) | (np.isnan(new) & np.isnan(old))
    assert same.all(), (f"{np.count_nonzero(~same)} of {len(x)} differ, e.g. x={x[~same][:3]} y={y[~same][:3]} "
                        f"rsq form={new[~same][:3]} sqrt/rcp form={old[~same][:3]}")
    # the reference is not vacuous: where numpy's correctly rounded operations apply, it is their value
    d = _dot_f32(ux, uy)
    ref = uy * (f(1) / np.sqrt(d))
    n0 = len(sx) + len(nx) + len(ax) + len(ay) + len(ox)
    np.testing.assert_array_equal(old[n0:n0 + len(ux)].view(np.uint32), ref.astype(f).view(np.uint32))
