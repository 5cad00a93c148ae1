"""The trace-kernel form matrix as data: for each of the 15 (kernel form, one-layer) pairs of
rt_kernels.hip pick() and for the camera-batch kernel, one recipe (a scene, the tree builder,
options.reserved[1], rt_debug_tune settings) under which a launch runs that kernel, with the
launch_info() words the launch must then report. tests/test_form_matrix_plan.py checks the recipes
against the host plan on the CPU, tests/test_gpu_form_matrix.py runs every recipe through every
launch kind on the GPU. Helper module (no tests here).

Form names are tests/test_gpu_contract.py LAUNCH_FORMS' (rtvk launch_info()["form"])."""
import functools
from collections import namedtuple

import numpy as np

BRUTE, AUTO, LBVH = 1, 0, 2                  # rt_options.accel
STREAM, HASH = 0, 2
# rt_internal.h ACCEL_* by launch_info name
ACCEL = {"brute": 1, "lbvh-global": 2, "lbvh-lds": 3, "lbvh-octant-lds": 4, "lbvh-treelet": 5, "grid-lds": 6,
         "grid-global": 7, "grid-lds-coop": 8, "grid-global-coop": 9, "grid-lds-rec": 10, "grid-lds-cq": 11,
         "grid-lds-rec-cq": 12}
FLAT_TWINS = ("grid-lds", "grid-lds-rec", "grid-global")    # the forms that have a one-layer kernel
LDS_FORMS = ("lbvh-lds", "lbvh-octant-lds", "grid-lds", "grid-lds-coop", "grid-lds-rec", "grid-lds-cq", "grid-lds-rec-cq")
L2_FORMS = ("lbvh-global", "grid-global", "grid-global-coop")
TREE_FORMS = ("lbvh-global", "lbvh-lds", "lbvh-octant-lds", "lbvh-treelet")
NO_ROWS_LDS = 0xffffffff

STACK_CAMERA = ((9.0, 3.0, -9.0), (0.0, 2.0, 0.0))   # a camera that looks at the stack from its side


def stack_scene(oracle):
    """The ground sphere and 240 small spheres (r = 0.2) from y = 0.2 to 4.6 over x, z in [-4, 4]: a
    grid several cells thick in y, so the grid forms run their general 3-D walk."""
    base = oracle.generate_scene()[4:5]
    stack = [oracle.generate_scene()[:1].copy()]   # the ground sphere
    rng = np.random.default_rng(11)
    for k in range(240):
        r = base.copy()
        r[0, :16].view(np.float32)[:] = [rng.uniform(-4, 4), 0.2 + 4.4 * k / 239, rng.uniform(-4, 4), 0.2]
        stack.append(r)
    return np.concatenate(stack)


@functools.lru_cache(maxsize=None)
def scene(oracle, key):
    """The spheres of a scene key, built once (read-only)."""
    sc = {"canon": lambda: oracle.generate_scene(0.0, 11), "stack": lambda: stack_scene(oracle),
          "k40": lambda: oracle.generate_scene(0.0, 40)}[key]()
    sc.setflags(write=False)
    return sc


N_SPHERES = {"canon": 488, "stack": 241, "k40": 6404}

# id: the case's name; scene: a key of scene(); builder: RT_BVH_BUILD (None: unset, the host builder);
# accel / reserved1: rt_options.accel / .reserved[1]; tune: rt_debug_tune settings; form / flat / batch:
# what launch_info() reports (batch: for a HASH launch with the uniform hand-out, not instrumented);
# model: the scene summary of tests/test_launch_plan.py SCENES that stands for the scene in the CPU
# plan, and whether its grid is three cells thick in y.
Recipe = namedtuple("Recipe", "id scene builder accel reserved1 tune form flat batch model layered")


def _r(id, scene, builder, reserved1, form, flat, tune=None, accel=LBVH, batch=False):
    model = {("canon", None): "canon", ("stack", None): "canon", ("canon", "gpu"): "dev1028", ("stack", "gpu"): "dev1028",
             ("k40", "gpu"): "c5"}[(scene, builder)]
    return Recipe(id, scene, builder, accel, reserved1, dict(tune or {}), form, flat, batch, model, scene == "stack")


RECIPES = [
    _r("grid-lds-rec-flat", "canon", None, 12, "grid-lds-rec", True, tune=dict(camera_batches=0)),
    _r("grid-lds-flat", "canon", None, 12, "grid-lds", True, tune=dict(grid_rec=0)),
    _r("grid-lds-coop", "canon", None, 14, "grid-lds-coop", False),
    _r("grid-lds-rec-cq", "canon", None, 16, "grid-lds-rec-cq", False),
    _r("grid-lds-cq", "canon", None, 16, "grid-lds-cq", False, tune=dict(grid_rec=0)),
    _r("lbvh-lds", "canon", None, 6, "lbvh-lds", False),
    _r("lbvh-octant-lds", "canon", None, 8, "lbvh-octant-lds", False),
    _r("lbvh-global", "canon", None, 10, "lbvh-global", False),
    _r("brute", "canon", None, 0, "brute", False, accel=BRUTE),
    _r("grid-lds-rec-3d", "stack", None, 12, "grid-lds-rec", False),
    _r("grid-lds-3d", "stack", None, 12, "grid-lds", False, tune=dict(grid_rec=0)),
    _r("grid-global-flat", "canon", "gpu", 12, "grid-global", True),
    _r("grid-global-coop", "canon", "gpu", 14, "grid-global-coop", False),
    _r("grid-global-3d", "stack", "gpu", 12, "grid-global", False),
    _r("lbvh-treelet", "k40", "gpu", 8, "lbvh-treelet", False),
    _r("camera-batch", "canon", None, 0, "grid-lds-rec", True, accel=AUTO, batch=True),
]
BY_ID = {r.id: r for r in RECIPES}
assert len(BY_ID) == len(RECIPES)


def options(lib, r, **kw):
    """rt_options of recipe `r` (accel and reserved[1] the recipe's) with make_options' keywords."""
    count = kw.pop("count_tests", False)
    o = lib.make_options(accel=r.accel, count_tests=count, **kw)
    o.reserved[1] = r.reserved1
    return o


def rows_lds_check(form, plan, band_h):
    """The rows map of a banded launch in the plan (rt_launch.cpp plan_form): staged past the form's own
    bytes (rounded up to 16) in the LDS forms, at byte 0 of the L2 forms' dynamic LDS (which holds
    nothing else), not in LDS for brute force. The treelet's 65 504 B leave the choice to the
    occupancy: either past them or not staged."""
    own = {"lbvh-lds": plan.lds1_bytes, "lbvh-octant-lds": plan.oct_bytes}.get(form, plan.grid_bytes)
    if form in LDS_FORMS:
        assert own > 0 and plan.rows_lds == (own + 15) & ~15, (form, own, plan.rows_lds)
        assert plan.lds == plan.rows_lds + 4 * band_h
    elif form in L2_FORMS:
        assert plan.rows_lds == 0 and plan.lds == 4 * band_h, (form, plan.rows_lds, plan.lds)
    elif form == "brute":
        assert plan.rows_lds == NO_ROWS_LDS and plan.lds == 0, (form, plan.rows_lds, plan.lds)
    else:
        assert form == "lbvh-treelet"
        assert (plan.rows_lds, plan.lds) in ((NO_ROWS_LDS, 2047 * 32), (2047 * 32, 2047 * 32 + 4 * band_h)), (plan.rows_lds, plan.lds)
