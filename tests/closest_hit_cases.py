"""Scenes, ray families and the float64 reference of the closest-hit probe tests
(tests/test_gpu_closest_hit.py on the GPU, tests/test_oracle.py on the CPU). Everything here is plain
numpy from fixed seeds; the oracle's answers are computed once per (scene, family) and shared."""
import numpy as np

MISS = 0xFFFFFFFF
T_MIN, T_MAX = 0.001, 10000.0
N_RAYS = 1 << 16
N_RAYS_BIG = 1 << 14
SCENES = ("canon", "stack", "cloud", "lattice")      # + "big" (device builder only)
GENERIC = ("generic",)
ADVERSARIAL = ("bounce", "axis", "boundary", "tangent", "far_near", "far")
FAMILIES = GENERIC + ADVERSARIAL


def _rec(base, x, y, z, r):
    s = base.copy()
    s[0, :16].view(np.float32)[:] = [x, y, z, r]
    return s


def make_scene(oracle, name):
    """(n, 80) uint8 sphere records of the named scene, built from oracle.generate_scene records."""
    canon = oracle.generate_scene()
    ground, base = canon[:1].copy(), canon[4:5]
    if name == "canon":
        return canon
    if name == "big":
        return oracle.generate_scene(0.0, 40)
    if name == "stack":      # test_grid_one_layer_and_layered_forms' y-stack
        rng = np.random.default_rng(11)
        recs = [ground]
        for k in range(240):
            recs.append(_rec(base, rng.uniform(-4, 4), 0.2 + 4.4 * k / 239, rng.uniform(-4, 4), 0.2))
        return np.concatenate(recs)
    if name == "cloud":      # overlapping spheres, radii at the grid's 8:1 limit, exact duplicates at higher indices
        rng = np.random.default_rng(23)
        recs = [ground]
        for _ in range(300):
            recs.append(_rec(base, rng.uniform(-3, 3), rng.uniform(0.45, 3.45), rng.uniform(-3, 3),
                             rng.uniform(0.06, 0.45)))
        for k in rng.choice(np.arange(1, 301), 20, replace=False):
            recs.append(recs[int(k)].copy())
        return np.concatenate(recs)
    if name == "lattice":    # test_grid_lattice_axis_rays' integer lattice
        recs = [ground]
        for i in range(-6, 7):
            for j in range(-6, 7):
                recs.append(_rec(base, float(i), 0.25, float(j), 0.25 if (i + j) % 3 else 0.5))
        return np.concatenate(recs)
    if name == "nobig":      # test_scene_without_big_spheres' scene: small spheres only
        return np.concatenate([_rec(base, i * 0.9, 0.2, j * 0.9, 0.2) for i in range(-5, 6) for j in range(-5, 6)])
    if name == "manybig":    # test_more_than_four_big_spheres' scene: eight big spheres
        extra = [(0.0, 4.0, 1.0), (-4.0, 4.0, 1.0), (4.0, -4.0, 1.0), (-6.0, -6.0, 2.5)]
        return np.concatenate([canon] + [_rec(canon[1:2], x, rad, z, rad) for x, z, rad in extra])
    raise KeyError(name)


def geometry(scene):
    """float32 [n, 4] (centre, radius) of sphere records."""
    return np.ascontiguousarray(scene[:, :16]).view(np.float32).reshape(-1, 4).copy()


def small_mask(g):
    """The spheres the grid holds: every sphere but the big ones (the ground, the radius-1 three)."""
    return g[:, 3] < 0.75


def grid_layout(g, n_cells, scene_radius, big_ids):
    """The grid's layout restated in float64 from the bounds of the spheres it holds (all but the
    device's big ones, scene_array(3)) and the cell counts the device reports (scene_array(9)["n"]):
    min corner, cell sizes, max corner, and the widened box's margin (64 u of the pad radius + 4e-3
    of the smallest cell)."""
    keep = np.ones(len(g), bool)
    keep[np.asarray(big_ids, np.int64)] = False
    s = g[keep]
    lo = (s[:, :3] - s[:, 3:4]).astype(np.float32).min(axis=0).astype(np.float64)
    hi = (s[:, :3] + s[:, 3:4]).astype(np.float32).max(axis=0).astype(np.float64)
    n = np.asarray(n_cells, np.float64)
    cs = np.maximum(hi - lo, 1e-6) / n
    margin = 64.0 * 2.0 ** -24 * (scene_radius * 1.01 + 100.0) + 4e-3 * cs.min()
    return {"lo": lo, "hi": hi, "cs": cs, "n": np.asarray(n_cells, np.int64), "margin": margin}


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _box(g):
    s = g[small_mask(g)]
    return (s[:, :3] - s[:, 3:4]).min(axis=0) - 0.5, (s[:, :3] + s[:, 3:4]).max(axis=0) + 0.5


def _rays(o, v):
    return np.ascontiguousarray(np.concatenate([o, v], axis=1), np.float32)


def generic(g, n, seed=1):
    """Origins uniform in the scene box (inside spheres and under the ground included) and on a
    shell at camera distance; directions uniform on the sphere, at lengths from 0.1 to 10."""
    rng = np.random.default_rng(seed)
    lo, hi = _box(g)
    o = rng.uniform(lo, hi, size=(n, 3))
    shell = rng.random(n) < 0.5
    o[shell] = _unit(rng, int(shell.sum())) * 17.3
    v = _unit(rng, n) * rng.uniform(0.1, 10.0, size=(n, 1))
    aimed = shell & (rng.random(n) < 0.7)      # most shell rays look at the scene, as a camera's do
    tgt = rng.uniform(lo, hi, size=(n, 3))
    v[aimed] = (tgt - o)[aimed]
    return _rays(o, v)


def _normalize32(v):
    v = v.astype(np.float32)
    return v / np.sqrt((v * v).sum(axis=1, keepdims=True)).astype(np.float32)


def bounce(g, n, gen_rays, gen_ids, gen_t, seed=2):
    """Origins on sphere surfaces: the oracle's hit points of the generic family, re-shot outward,
    inward (a dielectric's refraction) and grazing."""
    rng = np.random.default_rng(seed)
    hit = np.flatnonzero(gen_ids != MISS)
    pick = hit[rng.integers(0, len(hit), n)]
    o32, d32 = gen_rays[pick, :3], _normalize32(gen_rays[pick, 3:])
    p = (o32 + gen_t[pick, None].astype(np.float32) * d32).astype(np.float32)
    c, r = g[gen_ids[pick], :3], g[gen_ids[pick], 3:4]
    nrm = (p.astype(np.float64) - c) / r
    u = _unit(rng, n)
    tan = np.cross(nrm, u)
    tan /= np.maximum(np.linalg.norm(tan, axis=1, keepdims=True), 1e-12)
    kind = rng.integers(0, 4, n)[:, None]
    eps = 10.0 ** rng.uniform(-7, -2, size=(n, 1)) * rng.choice([-1.0, 1.0], size=(n, 1))
    v = np.where(kind == 0, nrm + u, np.where(kind == 1, -nrm + 0.7 * u, np.where(kind == 2, tan + eps * nrm, tan)))
    return _rays(p, v)


# +0, -0, a denormal that normalises to 0 or stays denormal (1 / d infinite), denormals and small
# normals whose reciprocal is finite but beyond 2^100 (4e-39: 2.5e38; 1e-36: o / d overflows for
# |o| > 340; 1e-32), and about 1e-30
_TINY = np.array([0.0, -0.0, 1e-42, -1e-42, 4e-39, -4e-39, 1e-36, -1e-36, 1e-32, -1e-32, 1e-30, -1e-30], np.float32)

# The ray the probe caught on `cloud` (every LBVH form missed sphere 22, t = 0.028013617): the y
# component of its direction normalises to a denormal, 1 / d.y = 2.3e38 is finite, and the node
# test's o.y / d.y overflowed (rt_trace_walk.h node_inv clamped the infinite reciprocal only).
DENORMAL_RAY = np.array([3191271496, 1075883891, 3217741472, 2147483648, 714, 3111091543], np.uint32).view(np.float32)


def axis(g, n, layout, seed=3):
    """Directions with one or two components exactly +0, -0, denormal, with a huge finite
    reciprocal, or about 1e-30, every sign pattern and every axis; origins generic, a third of them
    with a coordinate exactly on a grid plane."""
    rng = np.random.default_rng(seed)
    lo, hi = _box(g)
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    outside = rng.random(n) < 0.3
    o[outside] = (_unit(rng, int(outside.sum())) * rng.uniform(8, 30, size=(int(outside.sum()), 1))).astype(np.float32)
    if layout is not None:
        k = rng.integers(0, 3, n)
        c = rng.integers(0, layout["n"][k] + 1)
        plane = (layout["lo"][k] + c * layout["cs"][k]).astype(np.float32)
        snap = rng.random(n) < 0.34
        o[snap, k[snap]] = plane[snap]
    v = (_unit(rng, n) * rng.uniform(0.3, 3.0, size=(n, 1))).astype(np.float32)
    pattern = rng.integers(1, 7, n)            # bit k set: component k is tiny; never all three
    for k in range(3):
        m = (pattern >> k) & 1 == 1
        v[m, k] = _TINY[rng.integers(0, len(_TINY), int(m.sum()))]
    return _rays(o, v)


def _ulps(x, k):
    x = np.float32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, np.float32(np.inf if k > 0 else -np.inf))
    return x


def boundary(g, n, layout, seed=4):
    """Origins with coordinates exactly on cell planes gmin + c cs, one ulp to either side, and on
    the widened box; directions exactly along cell diagonals (ties of the DDA's three axes at every
    step), face diagonals and axes; rays entering through faces, edges and corners from outside, and
    rays parallel to a face just inside and just outside it."""
    rng = np.random.default_rng(seed)
    lo, hi, cs, nc, mg = layout["lo"], layout["hi"], layout["cs"], layout["n"], layout["margin"]
    planes = []
    for k in range(3):
        vals = [lo[k] + c * cs[k] for c in range(int(nc[k]) + 1)] + [lo[k] - mg, hi[k] + mg]
        pk = []
        for x in vals:
            pk += [_ulps(x, j) for j in (-2, -1, 0, 1, 2)]
        planes.append(np.asarray(pk, np.float32))
    o = np.stack([planes[k][rng.integers(0, len(planes[k]), n)] for k in range(3)], axis=1).astype(np.float64)
    free = rng.random((n, 3)) < 0.35           # some coordinates off the planes
    o = np.where(free, rng.uniform(lo - 0.3, hi + 0.3, size=(n, 3)), o)
    sg = rng.choice([-1.0, 1.0], size=(n, 3))
    kind = rng.integers(0, 4, n)[:, None]
    zero = np.eye(3)[rng.integers(0, 3, n)]
    diag = sg * cs
    v = np.where(kind <= 1, diag, np.where(kind == 2, diag * (1.0 - zero), diag * zero))
    start = rng.integers(0, 3, n)[:, None]     # 0: where it stands; 1, 2: backed out of the grid along -v
    steps = rng.integers(1, 4, size=(n, 1)) + np.max(nc)
    o = np.where(start == 0, o, o - v * steps)
    return _rays(o, v)


def tangent(g, n, seed=5):
    """Rays grazing spheres within rounding: through the pole p = c +- r e_k along d perpendicular to
    e_k (exactly, or tilted by about 1e-7), from p - s d + delta e_k with delta from 0 to a few ulps
    of |p_k| on either side and s in [0.5, 20]: the computed discriminant's sign is decided by
    rounding, and the outside ones fail the AABB gate."""
    rng = np.random.default_rng(seed)
    small = np.flatnonzero(small_mask(g))
    i = small[rng.integers(0, len(small), n)]
    k = rng.integers(0, 3, n)
    sgn = rng.choice([-1.0, 1.0], n)
    ek = np.eye(3)[k]
    c, r = g[i, :3].astype(np.float64), g[i, 3].astype(np.float64)
    pk = (g[i, :3][np.arange(n), k] + np.float32(1) * (sgn * g[i, 3]).astype(np.float32)).astype(np.float32)
    p = c.copy()
    p[np.arange(n), k] = pk
    ang = rng.uniform(0, 2 * np.pi, n)
    axis_al = rng.random(n) < 0.3
    ang[axis_al] = rng.integers(0, 4, int(axis_al.sum())) * (np.pi / 2)
    a, b = np.cos(ang), np.sin(ang)
    a[axis_al], b[axis_al] = np.round(a[axis_al]), np.round(b[axis_al])
    d = np.zeros((n, 3))
    k1, k2 = (k + 1) % 3, (k + 2) % 3
    d[np.arange(n), k1], d[np.arange(n), k2] = a, b
    tilt = np.where(rng.random(n) < 0.4, rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8, -6.5, n), 0.0)
    d[np.arange(n), k] = tilt
    s = rng.uniform(0.5, 20.0, n)
    o = p - s[:, None] * d
    ulp = np.spacing(np.abs(pk)).astype(np.float64)
    delta = rng.integers(-4, 5, n) * ulp * sgn          # positive: outside the sphere's box
    o[np.arange(n), k] = pk.astype(np.float64) + delta - s * tilt
    o32 = o.astype(np.float32)
    exact = tilt == 0.0                                  # the k coordinate exactly delta off the pole
    o32[exact, k[exact]] = (pk.astype(np.float64) + delta)[exact].astype(np.float32)
    return _rays(o32, d)


def far(g, n, dists, seed=6):
    """Origins at the given distances from the scene, aimed at it. Around 1e4 the hits straddle
    t = 10000 (tmax): the re-pad path, the grid's refusal beyond its pad radius, and the report
    accepted at exactly tmax."""
    rng = np.random.default_rng(seed)
    lo, hi = _box(g)
    tgt = rng.uniform(lo, hi, size=(n, 3))
    u = _unit(rng, n)
    u[:, 1] = np.abs(u[:, 1]) * 0.8 + 0.05      # from above the ground
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dist = np.asarray(dists, np.float64)[rng.integers(0, len(dists), n)]
    dist = dist + np.where(dist > 9000.0, rng.uniform(-12.0, 12.0, n), rng.uniform(-0.2, 0.2, n) * dist)
    o = tgt + u * dist[:, None]
    v = (tgt - o) * rng.uniform(0.5, 2.0, size=(n, 1)) / dist[:, None]
    return _rays(o, v)


T_MAX_SUCC = np.nextafter(np.float32(T_MAX), np.float32(np.inf))


def tmax_edge(oracle, scene, rays, ids, t, count=16):
    """From a far batch, by search with the oracle: rays whose float32 t is exactly 10000.0 (the
    report accepted at tmax), then rays on which the sphere they aim at reports exactly the
    successor of 10000.0 (oracle.report_t, the quadratic's t before the range test: the first value
    refused), then the accepted ones moved two ulps further back. Hits near tmax are slid along
    their ray so that t lands within a few ulps of the value wanted."""
    def slide(r, dt):   # origins moved back along the ray by dt
        d = r[:, 3:].astype(np.float64)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        q = r.copy()
        q[:, :3] = (r[:, :3].astype(np.float64) - np.asarray(dt, np.float64).reshape(-1, 1) * d).astype(np.float32)
        return q
    near = np.flatnonzero((ids != MISS) & (np.abs(t.astype(np.float64) - T_MAX) < 15.0))[:4096]
    if len(near) == 0:
        return rays[:0]
    cand = slide(rays[near], T_MAX - t[near].astype(np.float64))
    ci, ct = oracle.closest_hits(scene, cand)
    at = cand[(ci != MISS) & (ct == np.float32(T_MAX))][:count]
    cand = slide(rays[near], float(T_MAX_SUCC) - t[near].astype(np.float64))
    succ = cand[oracle.report_t(scene, cand, ids[near]) == T_MAX_SUCC][:count]
    return np.concatenate([at, succ, slide(at, 2.0 * float(np.spacing(np.float32(T_MAX))))])


def tmax_edge_counts(oracle, scene, rays, ids, t):
    """(rays accepted at exactly tmax, rays that miss although a sphere reports exactly succ(tmax))
    of a batch: the far family's condition on its own inputs."""
    accepted = int(((ids != MISS) & (t == np.float32(T_MAX))).sum())
    miss = np.flatnonzero(ids == MISS)
    refused = 0
    for k in range(len(scene)):   # which sphere reports succ(tmax) is not recorded: ask each
        refused += int((oracle.report_t(scene, rays[miss], np.full(len(miss), k, np.uint32)) == T_MAX_SUCC).sum())
        if refused >= 64:
            break
    return accepted, refused


def family(oracle, scene, name, layout, n, cache):
    """The rays of family `name` on `scene` (n of them, a few more for "far"); `cache` carries the
    generic family and its oracle answers to the bounce family."""
    g = geometry(scene)
    if name == "generic":
        return generic(g, n)
    if name == "bounce":
        gr, gi, gt = cache["generic"]
        return bounce(g, n, gr, gi, gt)
    if name == "axis":
        return axis(g, n, layout)
    if name == "boundary":
        return boundary(g, n, layout)
    if name == "tangent":
        return tangent(g, n)
    if name == "far_near":
        return far(g, n, [2e2])
    if name == "far":
        r = far(g, n, [5e3, 1e4, 1e4, 1e4])
        ids, t = oracle.closest_hits(scene, r)
        return np.concatenate([r, tmax_edge(oracle, scene, r, ids, t)])
    raise KeyError(name)


# ---- the float64 reference --------------------------------------------------------------------

def closest_hits_f64(g, rays, chunk=2048):
    """The plain quadratic in float64: per ray the closest t in [tmin, tmax] (t1 when t1 >= tmin,
    else t2), lowest index on ties. Returns ids, t, the three margins that say how far the ray is
    from a decision rounding could flip: gap (second-best candidate t minus the best; inf with fewer
    than two), disc (the smallest |D| / |oc|^2 over the spheres the ray could reach before its
    winner: the winner's own, and every near miss's and near hit's in front of it) and edge (the
    smallest distance of any root from tmin or tmax); and tscale = |oc|^2 / sqrt(D) + t of the
    winner, the factor by which a rounding error of D (a few u |oc|^2) and of the sum reach t."""
    c, r = g[:, :3].astype(np.float64), g[:, 3].astype(np.float64)
    n = len(rays)
    ids = np.full(n, MISS, np.uint32)
    t_out = np.full(n, np.inf)
    gap, disc, edge, tscale = np.full(n, np.inf), np.full(n, np.inf), np.full(n, np.inf), np.full(n, np.inf)
    if len(g) == 0:
        return ids, t_out, gap, disc, edge, tscale
    for s in range(0, n, chunk):
        o = rays[s:s + chunk, :3].astype(np.float64)
        v = rays[s:s + chunk, 3:].astype(np.float64)
        d = v / np.linalg.norm(v, axis=1, keepdims=True)
        oc = o[:, None, :] - c[None, :, :]
        b = (oc * d[:, None, :]).sum(axis=2)
        oc2 = (oc * oc).sum(axis=2)
        D = b * b - (oc2 - r * r)
        sq = np.sqrt(np.maximum(D, 0.0))
        t1, t2 = -b - sq, -b + sq
        t = np.where(t1 >= T_MIN, t1, t2)
        ok = (D >= 0.0) & (t >= T_MIN) & (t <= T_MAX)
        tc = np.where(ok, t, np.inf)
        w = tc.argmin(axis=1)
        rows = np.arange(len(o))
        tw = tc[rows, w]
        hit = np.isfinite(tw)
        ids[s:s + chunk] = np.where(hit, w, MISS).astype(np.uint32)
        t_out[s:s + chunk] = tw
        tc2 = tc.copy()
        tc2[rows, w] = np.inf
        with np.errstate(invalid="ignore", divide="ignore"):
            gap[s:s + chunk] = np.where(hit, tc2.min(axis=1) - tw, np.inf)
            tscale[s:s + chunk] = np.where(hit, oc2[rows, w] / sq[rows, w] + tw, np.inf)
        rel = np.abs(D) / np.maximum(oc2, 1e-300)
        could = (-b - np.abs(r) < np.where(hit, tw, T_MAX)[:, None]) & (-b + np.abs(r) > 0.0)
        disc[s:s + chunk] = np.where(could, rel, np.inf).min(axis=1)
        real = D >= 0.0
        e = np.minimum(np.where(real, np.abs(t1 - T_MIN), np.inf), np.where(real, np.abs(t2 - T_MIN), np.inf))
        e = np.minimum(e, np.where(real, np.minimum(np.abs(t1 - T_MAX), np.abs(t2 - T_MAX)), np.inf))
        edge[s:s + chunk] = e.min(axis=1)
    return ids, t_out, gap, disc, edge, tscale


# A ray is decided when its three margins clear these thresholds; on decided rays the oracle's
# winner is float64's and its t lies within T_TOL_U * 2^-24 * tscale of float64's. Measured, oracle
# against float64 on the generic family of the five scenes (2^16 rays each, 2^14 on `big`):
#   * every ray whose winner differs (11 rays: canon 3, stack 2, cloud 1, lattice 0, big 5) has
#     disc <= 1.46e-7 (canon 5.1e-8, stack 8.4e-8, cloud 3.2e-8, big 1.46e-7), and none of them has
#     gap / max(1, t) below 1.6e-2 or edge below 14: DISC_MIN is 7 x the worst; no ray was
#     undecided by its gap or its edge, so GAP_MIN and EDGE_MIN have no measured counterpart: they
#     are 17 x the t tolerance below at tscale = 100 (6e-5) and a tenth of tmin;
#   * the worst |t - t64| / (2^-24 tscale) of a decided ray is 3.69 (canon 3.42, stack 3.05, cloud
#     3.69, lattice 3.58, big 3.04): T_TOL_U is 2.7 x that;
#   * undecided: canon 0.11 %, stack 0.10 %, cloud 2.43 %, lattice 0.36 %, big 0.66 % (limit 5 %).
DISC_MIN = 1e-6
GAP_MIN = 1e-3        # x max(1, t)
EDGE_MIN = 1e-4
T_TOL_U = 10.0
UNDECIDED_MAX = 0.05


def decided(t64, gap, disc, edge):
    hit = np.isfinite(t64)
    return (disc >= DISC_MIN) & (edge >= EDGE_MIN) & (gap >= GAP_MIN * np.maximum(1.0, np.where(hit, t64, 1.0)))
