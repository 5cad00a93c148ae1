"""The reprojected temporal call without a GPU: the numpy restatement
(tests/temporal_reproject_sim.py) against an independent scalar loop, the snap (a motion plane that
names every texel's own centre to within 2^-6 makes the call the in-place call, bit for bit, over a
three-frame chain and when the two calls are mixed), the bilinear taps and their feature stop, taps
that leave the band, ok = 0 and the two plane sets."""
import numpy as np

import motion_sim as ms
import temporal_reproject_sim as tr
import temporal_sim as ts

f32 = np.float32


def frames(seed, H, W, F, n=3):
    """n frames (A, B, feat0, feat1) of random finite inputs that share their guides. The guide is
    smooth over the band, as a surface's is (normal (0.5, -0.5, 0.7) and depth 8 after the division by F,
    each within 2 %), so that a neighbour's history passes the feature stop unless a test changes it."""
    _, feat0, _ = ts.random_inputs(seed, H, W, F)
    rng = np.random.default_rng(seed + 1000)
    feat1 = (f32([0.5, -0.5, 0.7, 8.0]) * f32(F) * rng.uniform(0.98, 1.02, (H, W, 4))).astype(f32)
    out = []
    for k in range(n):
        A, _, _ = ts.random_inputs(seed + 10 * k + 1, H, W, F)
        B, _, _ = ts.random_inputs(seed + 10 * k + 2, H, W, F)
        out.append((A, B, feat0, feat1))
    return out


def same_bits(got, want, what=""):
    for g, w, name in zip(got, want, ("out_a", "out_b", "mean", "history_len")):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            np.testing.assert_array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32),
                                          err_msg=str((what, name)))


def test_a_real_frame_against_itself_is_the_in_place_chain(oracle):
    """The motion plane of the canonical scene against itself (inside the snap, test_motion_host.py)
    over three frames: out_a, out_b, the mean and history_len equal temporal_sim.accumulate's chain bit
    for bit, with two accumulators and with one."""
    W, H, F = 96, 54, 4
    motion = ms.motion(oracle, oracle.generate_scene(0.0), oracle.render_call_info(1, W, H), W, H)
    assert not np.array_equal(motion[..., 0:2], tr.identity_motion(H, W)[..., 0:2])     # rounded, not exact
    for two in (True, False):
        a, b = tr.State(H, W), ts.State(H, W)
        for k, (A, B, feat0, feat1) in enumerate(frames(3, H, W, F)):
            kw = dict(accum_b=B if two else None, spp=2, params=(2, 4.0, 16.0))
            got = tr.reproject(a, A, feat0, feat1, F, motion, **kw)
            want = ts.accumulate(b, A, feat0, feat1, F, **kw)
            same_bits(got, want, (two, k))
            assert np.all(got[3] == min(k + 1, 2))
        for p, q in ((a.ha, b.ha), (a.hg, b.hg)) + (((a.hb, b.hb),) if two else ()):
            np.testing.assert_array_equal(p.view(np.uint32), q.view(np.uint32))


def test_the_two_calls_mix_on_one_state():
    """reproject, accumulate, reproject against three in-place calls, and a reset in between clears the
    set that is current."""
    H, W, F = 7, 9, 5
    motion = tr.identity_motion(H, W)
    motion[..., 0] += f32(2.0 ** -7)           # inside the snap
    fr = frames(8, H, W, F)
    a, b = tr.State(H, W), ts.State(H, W)
    for k, (A, B, feat0, feat1) in enumerate(fr):
        want = ts.accumulate(b, A, feat0, feat1, F, accum_b=B, spp=3)
        if k == 1:
            got = ts.accumulate(a, A, feat0, feat1, F, accum_b=B, spp=3)
        else:
            got = tr.reproject(a, A, feat0, feat1, F, motion, accum_b=B, spp=3)
        same_bits(got, want, k)
    assert np.all(got[3] == 3)
    a.reset()
    A, B, feat0, feat1 = fr[0]
    got = tr.reproject(a, A, feat0, feat1, F, motion, accum_b=B, spp=3)
    assert np.all(got[3] == 1)


# ---- the restatement against a scalar loop --------------------------------------------------------

def scalar_texel(st, A, B, feat0, feat1, F, motion, h, params, y, x):
    """(out_a.rgb, out_b.rgb, n') of one texel, one float32 operation at a time."""
    nmax, kn, kd = f32(params[0]), f32(params[1]), f32(params[2])
    H, W = st.H, st.W
    a = [f32(f32(feat0[y, x, c]) / f32(F)) + f32(2.0 ** -6) for c in range(3)]
    nrm = [f32(feat1[y, x, c]) / f32(F) for c in range(3)]
    z = f32(feat1[y, x, 3]) / f32(F)
    sx, sy, dzm, ok = (f32(v) for v in motion[y, x])
    bx, by = f32(sx - f32(0.5)), f32(sy - f32(0.5))
    jx, jy = np.floor(f32(bx + f32(0.5))), np.floor(f32(by + f32(0.5)))
    if abs(f32(bx - jx)) <= f32(2.0 ** -6) and abs(f32(by - jy)) <= f32(2.0 ** -6):
        tap = [(jx, jy, f32(1.0))]
    else:
        ix, iy = np.floor(bx), np.floor(by)
        fx, fy = f32(bx - ix), f32(by - iy)
        gx, gy = f32(f32(1.0) - fx), f32(f32(1.0) - fy)
        tap = [(ix, iy, f32(gx * gy)), (ix + 1, iy, f32(fx * gy)), (ix, iy + 1, f32(gx * fy)), (ix + 1, iy + 1, f32(fx * fy))]
    ze = f32(z + dzm)
    Wt, S, SB = f32(0.0), [f32(0.0)] * 4, [f32(0.0)] * 3
    for tx, ty, w in tap:
        if not (ok > 0 and w > 0 and 0 <= tx < W and 0 <= ty < H):
            continue
        HA, HB, HG = st.ha[int(ty), int(tx)], st.hb[int(ty), int(tx)], st.hg[int(ty), int(tx)]
        dn = [f32(nrm[c] - HG[c]) for c in range(3)]
        dn2 = f32(f32(f32(dn[0] * dn[0]) + f32(dn[1] * dn[1])) + f32(dn[2] * dn[2]))
        dz = f32(f32(ze - HG[3]) / f32(ze + f32(1.0)))
        stop = f32(f32(f32(1.0) + f32(kn * dn2)) * f32(f32(1.0) + f32(kd * f32(dz * dz))))
        if HA[3] > 0 and stop < 2:
            Wt = f32(Wt + w)
            S = [f32(S[c] + f32(w * HA[c])) for c in range(4)]
            SB = [f32(SB[c] + f32(w * HB[c])) for c in range(3)]
    valid = Wt > 0
    outs = []
    if h == 0:
        n = f32(S[3] / Wt) if valid else f32(0.0)
    else:
        n = min(f32(f32(S[3] / Wt) + f32(1.0)), nmax) if valid else f32(1.0)
    for acc, Ssum in ((A, S), (B, SB)):
        e = [f32(f32(f32(acc[y, x, c]) / f32(h)) / a[c]) if h else f32(0.0) for c in range(3)]
        if valid:
            hist = [f32(Ssum[c] / Wt) for c in range(3)]
            new = hist if h == 0 else [f32(hist[c] + f32(f32(f32(1.0) / n) * f32(e[c] - hist[c]))) for c in range(3)]
        else:
            new = e
        outs.append(np.array([f32(new[c] * a[c]) for c in range(3)], f32))
    return outs[0], outs[1], n


def branch_motion(H, W, seed):
    """A motion plane that takes every branch: snapped texels (exact centres and centres off by up to
    2^-6), four-tap texels at random fractions, taps that leave the band on each of its four sides,
    whole neighbourhoods outside, ok = 0, and a NaN and an infinity under ok = 1."""
    rng = np.random.default_rng(seed)
    m = tr.identity_motion(H, W)
    kind = rng.integers(0, 4, (H, W))
    shift = rng.uniform(-2.5, 2.5, (H, W, 2)).astype(f32)
    m[..., 0:2] += np.where((kind >= 2)[..., None], shift, f32(0.0))                # four taps, up to 2.5 texels away
    m[..., 0] += np.where(kind == 1, f32(2.0 ** -6), f32(0.0))                      # the snap's edge, inside
    m[..., 1] -= np.where(kind == 1, f32(2.0 ** -7), f32(0.0))
    m[..., 2] = rng.uniform(-4.0, 4.0, (H, W)).astype(f32) * (kind == 3)            # dzm: some stops refuse
    m[0, :, 1] = f32(0.25)                      # rows above the band: iy = -1
    m[H - 1, :, 1] = f32(H - 0.25)              # below: iy + 1 = H
    m[:, 0, 0] = f32(0.25)                      # left: ix = -1
    m[:, W - 1, 0] = f32(W - 0.25)              # right: ix + 1 = W
    m[H // 2, W // 2, 0:2] = [-40.0, 3.0]       # the whole neighbourhood outside
    m[H // 2, W // 2 + 1, 0:2] = [3.0, 1.0e9]
    m[1, 1, 3] = 0.0                            # ok = 0
    m[2, 2] = [np.nan, 2.5, 0.0, 1.0]
    m[2, 3] = [2.5, np.inf, 0.0, 1.0]
    m[3, 2] = [2.5, 2.5, np.nan, 1.0]           # a NaN dzm stops every tap
    return m


def test_restatement_equals_the_scalar_loop():
    """Three frames on one state with a branch-covering motion plane, counts with zeros at frames 1 and
    2, every texel of a 9 x 12 band against the scalar loop; the planes the call wrote are checked as
    the next frame's history."""
    H, W, F = 9, 12, 5
    params = (3, 4.0, 16.0)
    st = tr.State(H, W)
    rng = np.random.default_rng(5)
    seen = set()
    for k, (A, B, feat0, feat1) in enumerate(frames(21, H, W, F)):
        feat1 = feat1.copy()
        if k >= 1:      # some guides change: the feature stop refuses taps, histories of unequal length meet
            feat1[::2, ::3, :3] = -feat1[::2, ::3, :3]
        if k == 2:
            feat1[1::2, 1::3, :3] = -feat1[1::2, 1::3, :3]
        motion = branch_motion(H, W, 40 + k)
        counts = rng.integers(1, 4, (H, W)).astype(np.uint32)
        motion[5, 5] = [5.5, 5.5, 0.0, 1.0]      # its own history, whose guide no frame changes
        if k:
            counts[0, 0] = counts[5, 5] = counts[1, 1] = 0
        before = st.copy()
        out_a, out_b, mean, n = tr.reproject(st, A, feat0, feat1, F, motion, accum_b=B, sample_count=counts, params=params)
        assert st.other[0] is before.ha or np.array_equal(st.other[0], before.ha)
        for y in range(H):
            for x in range(W):
                with np.errstate(invalid="ignore"):       # the plane's NaN and infinity
                    wa, wb, wn = scalar_texel(before, A, B, feat0, feat1, F, motion, int(counts[y, x]), params, y, x)
                np.testing.assert_array_equal(out_a[y, x, :3].view(np.uint32), wa.view(np.uint32), err_msg=str((k, y, x)))
                np.testing.assert_array_equal(out_b[y, x, :3].view(np.uint32), wb.view(np.uint32), err_msg=str((k, y, x)))
                assert n[y, x] == np.uint32(wn) and st.ha[y, x, 3] == wn == st.hb[y, x, 3], (k, y, x)
                seen.add((k > 0, int(counts[y, x]) > 0, float(wn) == int(wn), int(n[y, x])))
        np.testing.assert_array_equal(st.hg[..., 3], feat1[..., 3] / f32(F))
        assert np.all(out_a[..., 3] == 1) and np.isfinite(out_a).all() and np.isfinite(mean).all()
    # restarts (n 1), integer and fractional histories, the cap, and unmeasured texels with and without a history
    assert {(True, True, True, 1), (True, True, False, 2), (True, True, True, 3), (True, False, True, 0)} <= seen, seen
    assert any(s[0] and not s[1] and s[3] > 0 for s in seen)


def test_taps_weights_and_the_snap():
    tap, snap = tr.taps(np.array([[[5.5, 3.5, 0, 1], [5.5 + 2.0 ** -6, 3.5 - 2.0 ** -6, 0, 1], [5.5 + 2.0 ** -5, 3.5, 0, 1],
                                   [6.25, 3.0, 0, 1]]], f32))
    assert snap.tolist() == [[True, True, False, False]]
    assert [float(tap[0][i][0, 0]) for i in range(3)] == [5.0, 3.0, 1.0] and all(float(t[2][0, 0]) == 0 for t in tap[1:])
    assert [float(tap[0][i][0, 1]) for i in range(3)] == [5.0, 3.0, 1.0]
    w = [float(t[2][0, 3]) for t in tap]                      # bx 5.75, by 2.5
    assert w == [0.25 * 0.5, 0.75 * 0.5, 0.25 * 0.5, 0.75 * 0.5]
    assert [(float(t[0][0, 3]), float(t[1][0, 3])) for t in tap] == [(5, 2), (6, 2), (5, 3), (6, 3)]
    assert abs(sum(float(t[2][0, 2]) for t in tap) - 1.0) < 1e-6


def test_a_shifted_history_follows_its_motion():
    """A history whose colour is its texel's column index, moved one texel to the right by the motion
    plane, and half a texel: the history each texel integrates is its source's, or the mean of its two
    sources; the column that has no source starts over."""
    H, W, F = 4, 8, 4
    A, B, feat0, feat1 = frames(2, H, W, F, n=1)[0]
    feat1[...] = feat1[0, 0]                                      # one guide everywhere: every tap counts
    feat0[...] = f32(F) * f32(1.0 - 2.0 ** -6)                    # a = 1 exactly
    st = tr.State(H, W)
    ramp = np.zeros((H, W, 4), f32)
    ramp[..., :3] = np.arange(W, dtype=f32)[None, :, None]
    tr.reproject(st, ramp, feat0, feat1, F, tr.identity_motion(H, W), spp=1)
    np.testing.assert_array_equal(st.ha[..., 0], ramp[..., 0])
    for shift, want in ((1.0, lambda x: x - 1.0), (0.5, lambda x: x - 0.5)):
        s2 = st.copy()
        m = tr.identity_motion(H, W)
        m[..., 0] -= f32(shift)
        zero = np.zeros((H, W, 4), f32)
        _, _, _, n = tr.reproject(s2, zero, feat0, feat1, F, m, sample_count=np.zeros((H, W), np.uint32))
        np.testing.assert_array_equal(n[:, 1:], 1)
        np.testing.assert_array_equal(s2.ha[:, 1:, 0], np.broadcast_to(want(np.arange(1, W, dtype=f32)), (H, W - 1)))
        if shift == 1.0:
            assert np.all(n[:, 0] == 0) and np.all(s2.ha[:, 0] == 0)           # no source, no measurement
        else:
            assert np.all(n[:, 0] == 1) and np.all(s2.ha[:, 0, 0] == 0)        # the one tap inside, renormalised
