"""CPU model of an adaptive frame (rt_render_adaptive_device), built on the
unchanged oracle: the per-sample integer cube Q[s, y, x, c] of the counter-based stream, the pass
loop simulated on it with Python ints, and the expected frame stitched from oracle.render(spp=n).
Helper module of test_adaptive.py and test_cli_adaptive.py (no tests here).

A scene is named by `k`: generate_scene's grid half extent, or the name of a scene handed to
register(); the cubes and frames are cached once per scene either way."""
import functools

import numpy as np

HASH = 2


_REGISTERED = {}


def register(name, spheres):
    """Makes `spheres` the scene of the key `name` (a string) for scene(), cube() and expected_frame().
    A name keeps the spheres it was first given."""
    held = _REGISTERED.get(name)
    if held is None:
        held = _REGISTERED[name] = np.array(spheres, copy=True)
        held.setflags(write=False)
    assert held.shape == np.shape(spheres) and np.array_equal(held, spheres), f"scene {name!r} registered with other spheres"
    return name


@functools.lru_cache(maxsize=None)
def _scene(oracle, k):
    return _REGISTERED[k] if isinstance(k, str) else oracle.generate_scene(0.0, k)


def scene(oracle, k=11):
    return _scene(oracle, k)


@functools.lru_cache(maxsize=None)
def _cube(oracle, k, W, H, img_w, img_h, rows, base, max_spp):
    sc = scene(oracle, k)
    rw = None if rows is None else np.array(rows, np.uint32)
    q = np.zeros((max_spp, H, W, 3), np.int64)
    for s in range(max_spp):
        acc, _, _ = oracle.render(sc, oracle.render_call_info(1, img_w, img_h), W, H, rows=rw,
                                  opts=oracle.options(rng_mode=HASH, sample_base=base + s))
        v = acc[..., :3].astype(np.float64) * 2.0 ** 24   # one sample: <= 2^24, exact in binary32
        assert np.array_equal(v, np.floor(v))
        q[s] = v.astype(np.int64)
    q.setflags(write=False)
    return q


def cube(oracle, W, H, max_spp, k=11, rows=None, base=0, image=None):
    """Q[s, y, x, c]: sample base + s of every band pixel as the 8.24 integer the kernels add.
    Computed once per geometry and shared (read-only)."""
    iw, ih = image if image else (W, H)
    return _cube(oracle, k, W, H, iw, ih, None if rows is None else tuple(int(r) for r in rows), base, max_spp)


def converged(E, S, n, m, thr_q16):
    """The criterion in Python ints."""
    return (int(E) << 17) < int(thr_q16) * (int(S) + int(n) * 3 * int(m) * (1 << 16))


def simulate(Q, min_spp, step_spp, max_spp, thr_q16):
    """The pass loop on the cube. Returns (count map [H, W] of per-pixel n, info dict with passes,
    tiles, tiles_capped, samples)."""
    _, H, W, _ = Q.shape
    counts = np.zeros((H, W), np.uint32)
    passes = capped = samples = tiles = 0
    for ty in range(0, H, 8):
        for tx in range(0, W, 8):
            q = Q[:, ty:ty + 8, tx:tx + 8, :]
            m = q.shape[1] * q.shape[2]
            a = np.zeros(q.shape[1:], np.int64)
            b = np.zeros(q.shape[1:], np.int64)
            n = p = 0
            while True:
                k = min_spp if p == 0 else min(step_spp, max_spp - n)
                a += q[n:n + k // 2].sum(axis=0)
                b += q[n + k // 2:n + k].sum(axis=0)
                n += k
                p += 1
                conv = converged(np.abs(a - b).sum(), (a + b).sum(), n, m, thr_q16)
                if conv or n >= max_spp:
                    break
            counts[ty:ty + 8, tx:tx + 8] = n
            passes = max(passes, p)
            capped += int(not conv)
            samples += n * m
            tiles += 1
    return counts, {"passes": passes, "tiles": tiles, "tiles_capped": capped, "samples": samples}


def histogram(counts):
    """{n: tiles} of a count map."""
    t = counts[::8, ::8]
    return {int(n): int((t == n).sum()) for n in np.unique(t)}


def assert_not_vacuous(counts, max_spp):
    """The simulated map exercises the feature: several counts, a capped tile, an early stop."""
    h = histogram(counts)
    assert len(h) >= 4, h
    assert max_spp in h, h
    assert min(h) < max_spp // 2, h


@functools.lru_cache(maxsize=None)
def _uniform(oracle, k, W, H, img_w, img_h, rows, base, n):
    rw = None if rows is None else np.array(rows, np.uint32)
    acc, out, _ = oracle.render(scene(oracle, k), oracle.render_call_info(n, img_w, img_h), W, H, rows=rw,
                                opts=oracle.options(rng_mode=HASH, sample_base=base))
    acc.setflags(write=False)
    out.setflags(write=False)
    return acc, out


def expected_frame(oracle, counts, k=11, rows=None, base=0, image=None):
    """accum and rgba8 of the adaptive frame: every pixel from oracle.render(spp = its n)."""
    H, W = counts.shape
    iw, ih = image if image else (W, H)
    rt = None if rows is None else tuple(int(r) for r in rows)
    acc = np.zeros((H, W, 4), np.float32)
    out = np.zeros((H, W, 4), np.uint8)
    for n in np.unique(counts):
        a, o = _uniform(oracle, k, W, H, iw, ih, rt, base, int(n))
        sel = counts == n
        acc[sel] = a[sel]
        out[sel] = o[sel]
    return acc, out
