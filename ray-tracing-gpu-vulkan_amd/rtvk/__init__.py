"""rtvk — host-side mirror of the reference's hot-path API over librt_mi355x.so.

Names follow the reference:
  generateRandomScene(t)           src/scene.h:79-157 (t explicit instead of the wall clock)
  RenderCallInfo / Sphere / Scene  src/render_call_info.h:5-13, src/scene.h:16-29
  ray_trace(samples, storeRenderResult, width, height, gpu_count)
                                   src/ray_trace.h:9-15 (headless; renders once and returns)
and the per-frame device work of src/ray_trace.cpp:567-739 is ``Renderer.render_device``.

Everything computes in the HIP library; this module only marshals arguments. Device buffers are
torch tensors (memory + stream plumbing only).
"""
from __future__ import annotations

import ctypes
import weakref
from dataclasses import dataclass
from typing import Iterable, Optional, Sequence

import numpy as np

from . import abi
from .abi import (CHECKERED, DIFFUSE, METAL, REFRACTIVE, SOLID, Adaptive, AdaptiveInfo, Options, RenderCallInfo,
                  RtError, Scene, Sphere, Stats, check, load_library)

__all__ = [
    "DIFFUSE", "METAL", "REFRACTIVE", "SOLID", "CHECKERED", "Sphere", "Scene", "RenderCallInfo",
    "Options", "Stats", "RtError", "generateRandomScene", "canonical_render_call_info",
    "make_options", "Renderer", "MultiRenderer", "render", "ray_trace", "store_ppm", "spheres_to_numpy",
    "load_library", "HASH", "STREAM", "multi_plan", "launch_inputs", "launch_plan", "row_weights", "struct_dict", "partition_strips", "partition_rebalance",
    "Adaptive", "AdaptiveInfo", "make_adaptive", "threshold_q16", "adaptive_tile_converged",
    "partition_tile_rows", "multi_plan_adaptive", "SampleMap", "sample_map_plan", "sample_map_info", "sample_map_block_plan",
    "sample_map_device_capacity", "sample_map_device_unit", "sample_map_feedback_count", "hand_out", "make_feedback",
    "make_denoise", "denoise_check", "make_denoise_variance", "denoise_variance_check",
    "Temporal", "make_temporal", "temporal_check", "Motion", "motion_check", "half_outputs_check",
]

STREAM = abi.RT_RNG_PIXEL_STREAM   # the reference's per-pixel LCG stream (random.glsl)
HASH = abi.RT_RNG_SAMPLE_HASH      # counter-based per-sample streams, chunked across lanes / GPUs

MAX_DEPTH = 50  # shader.rgen:27


def generateRandomScene(t: float = 0.0, grid_half_extent: int = 11):
    """src/scene.h:79-157: ground + 3 big spheres + (2K)^2 grid; K = 11 gives the 488-sphere scene.

    Returns a ctypes array of ``Sphere`` (length 4 + 4K^2)."""
    lib = load_library()
    n = ctypes.c_uint32()
    check(lib.rt_generate_scene(ctypes.c_float(t), grid_half_extent, None, 0, ctypes.byref(n)))
    arr = (Sphere * n.value)()
    check(lib.rt_generate_scene(ctypes.c_float(t), grid_half_extent, ctypes.addressof(arr), n.value,
                                ctypes.byref(n)))
    return arr


def spheres_to_numpy(spheres) -> np.ndarray:
    """Raw 80-byte records as a (n, 80) uint8 array (for hashing / fixtures)."""
    return np.frombuffer(bytes(spheres), dtype=np.uint8).reshape(-1, 80)


def canonical_render_call_info(spp: int, width: int = 1920, height: int = 1080) -> RenderCallInfo:
    """The RenderCallInfo the reference fills every frame (src/ray_trace.cpp:660-676)."""
    rci = RenderCallInfo()
    check(load_library().rt_canonical_render_call_info(spp, width, height, ctypes.byref(rci)))
    return rci


def make_options(max_depth: int = MAX_DEPTH, seed_mode: int = abi.RT_SEED_GLOBAL,
                 rng_mode: int = abi.RT_RNG_PIXEL_STREAM, accel: int = abi.RT_ACCEL_AUTO,
                 accumulate: bool = False, sample_base: int = 0, count_tests: bool = False) -> Options:
    o = Options()
    o.max_depth, o.seed_mode, o.rng_mode, o.accel = max_depth, seed_mode, rng_mode, accel
    o.accumulate, o.sample_base = int(bool(accumulate)), sample_base
    o.reserved[0] = 1 if count_tests else 0
    return o


def make_adaptive(threshold: float, min_spp: int = 8, step_spp: int = 8) -> Adaptive:
    """rt_adaptive of an adaptive frame (Renderer.render_adaptive): every pixel gets `min_spp`
    samples, tiles that have not converged to `threshold` get `step_spp` more per pass, up to the
    RenderCallInfo's samplesPerRenderCall. Counts are even, 0 <= threshold <= 16."""
    a = Adaptive()
    a.min_spp, a.step_spp, a.threshold, a.reserved = min_spp, step_spp, threshold, 0
    return a


def make_feedback(threshold: float, min_spp: int = 4, max_spp: int = 64, unit_samples: int = 0) -> "abi.SampleMapFeedback":
    """rt_sample_map_feedback of a feedback frame (Renderer.render_sample_map_feedback): a tile that
    misses `threshold` doubles its count up to max_spp, one that meets half of it halves down to
    min_spp. Counts are even, 0 <= threshold <= 16."""
    f = abi.SampleMapFeedback()
    f.threshold, f.min_spp, f.max_spp, f.unit_samples, f.reserved = threshold, min_spp, max_spp, unit_samples, 0
    return f


def make_denoise(iterations: int = 3, k_normal: float = 4.0, k_depth: float = 16.0,
                 k_color: float = 1.0) -> "abi.Denoise":
    """rt_denoise of Renderer.denoise: `iterations` a-trous passes (1..6, steps 1, 2, 4, ...), and the
    edge-stopping strengths of the first-hit normal, the relative first-hit depth and the
    demodulated colour (finite, >= 0; 0 switches a term off). The defaults are the library's."""
    d = abi.Denoise()
    d.iterations, d.k_normal, d.k_depth, d.k_color = iterations, k_normal, k_depth, k_color
    return d


def half_outputs_check(halves: Optional["abi.HalfOutputs"], accum_ptr: Optional[int] = None) -> None:
    """rt_half_outputs_check (host only): raises RtError where a halves frame would refuse its
    rt_half_outputs beside `accum_ptr`, the address of the frame's accumulator (pointers are compared,
    nothing is read)."""
    check(load_library().rt_half_outputs_check(ctypes.byref(halves) if halves is not None else None, accum_ptr))


def denoise_check(params: Optional["abi.Denoise"], band_w: int, band_h: int, feature_samples: int) -> None:
    """rt_denoise_check (host only): raises RtError where Renderer.denoise would refuse."""
    check(load_library().rt_denoise_check(ctypes.byref(params) if params is not None else None,
                                          band_w, band_h, feature_samples))


def make_denoise_variance(iterations: int = 3, prefilter: int = 2, k_normal: float = 4.0, k_depth: float = 16.0,
                          k_color: float = 0.25) -> "abi.DenoiseVariance":
    """rt_denoise_variance of Renderer.denoise_variance: `prefilter` feature-only passes over the
    half-buffer variance (0..3), then `iterations` a-trous passes (1..6) whose colour weight is
    k_color times the squared colour difference over the tracked variance. The defaults are the
    library's."""
    d = abi.DenoiseVariance()
    d.iterations, d.prefilter, d.k_normal, d.k_depth, d.k_color = iterations, prefilter, k_normal, k_depth, k_color
    return d


def denoise_variance_check(params: Optional["abi.DenoiseVariance"], band_w: int, band_h: int,
                           feature_samples: int) -> None:
    """rt_denoise_variance_check (host only): raises RtError where Renderer.denoise_variance would
    refuse."""
    check(load_library().rt_denoise_variance_check(ctypes.byref(params) if params is not None else None,
                                                   band_w, band_h, feature_samples))


def make_temporal(max_history: int = 8, k_normal: float = 4.0, k_depth: float = 16.0) -> "abi.TemporalParams":
    """rt_temporal_params of Renderer.temporal_accumulate: a texel's history holds at most
    `max_history` frames (2..65535; the blend weight of a frame never falls below 1 / max_history),
    and it starts over where the first-hit normal or the relative first-hit depth moved, by the
    filters' feature stop with these strengths (finite, >= 0). The defaults are the library's."""
    t = abi.TemporalParams()
    t.max_history, t.k_normal, t.k_depth, t.reserved = max_history, k_normal, k_depth, 0
    return t


def temporal_check(params: Optional["abi.TemporalParams"], band_w: int, band_h: int, feature_samples: int) -> None:
    """rt_temporal_check (host only): raises RtError where Renderer.temporal_accumulate would
    refuse its parameters."""
    check(load_library().rt_temporal_check(ctypes.byref(params) if params is not None else None,
                                           band_w, band_h, feature_samples))


def threshold_q16(threshold: float) -> int:
    """The criterion's integer threshold: floor(double(float32(threshold)) * 65536 + 0.5)."""
    return int(np.floor(float(np.float32(threshold)) * 65536.0 + 0.5))


def adaptive_tile_converged(E: int, S: int, n: int, m: int, thr_q16: int) -> bool:
    """The stop criterion of one tile as the library evaluates it (rt_adaptive_tile_converged,
    host only): 2^17 E < thr_q16 (S + n * 3 * m * 2^16)."""
    c = ctypes.c_int(0)
    check(load_library().rt_adaptive_tile_converged(E, S, n, m, thr_q16, ctypes.byref(c)))
    return bool(c.value)


def _stream_ptr(stream, device: int) -> Optional[int]:
    """hipStream_t of `stream`, or of torch's current stream ON `device` when None (torch's
    current device may be another GPU)."""
    if stream is None:
        import torch
        return torch.cuda.current_stream(device).cuda_stream
    return getattr(stream, "cuda_stream", stream)


def _check_dev_tensor(t, dtype_name: str, shape: Sequence[int]):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError("expected a device (cuda) torch.Tensor")
    if str(t.dtype) != dtype_name or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise ValueError(f"expected contiguous {dtype_name} tensor of shape {tuple(shape)}, "
                         f"got {t.dtype} {tuple(t.shape)}")


class Renderer:
    """One device context: HBM-resident scene + LBVH, and the fused trace kernel.

    Replaces, per GPU, the reference's descriptor set / BLAS / TLAS / pipeline
    (src/ray_trace.cpp:315-527) and its per-frame command buffer (src/vulkan.h:998-1204)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._ctx = ctypes.c_void_p()
        check(self._lib.rt_context_create(device, ctypes.byref(self._ctx)))
        self.device = device
        self.sphere_count = 0
        self._maps = weakref.WeakSet()

    def close(self) -> None:
        for m in list(getattr(self, "_maps", ())):
            m.close()
        if self._ctx:
            self._lib.rt_context_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, spheres, stream=None) -> None:
        """Upload spheres (ctypes Sphere array or (n,80) uint8 records) and build the LBVH, ordered
        on `stream` (torch's current stream by default, like render_device)."""
        buf = spheres if not isinstance(spheres, np.ndarray) else np.ascontiguousarray(spheres, np.uint8)
        n = len(spheres)
        ptr = ctypes.addressof(buf) if not isinstance(buf, np.ndarray) else buf.ctypes.data
        st = _stream_ptr(stream, self.device)
        check(self._lib.rt_set_scene(self._ctx, ptr if n else None, n, st))
        self.sphere_count = n

    def refit_scene(self, spheres, stream=None) -> None:
        """Per-frame update (same count): refit the device-built tree to moved spheres."""
        buf = spheres if not isinstance(spheres, np.ndarray) else np.ascontiguousarray(spheres, np.uint8)
        n = len(spheres)
        ptr = ctypes.addressof(buf) if not isinstance(buf, np.ndarray) else buf.ctypes.data
        st = _stream_ptr(stream, self.device)
        check(self._lib.rt_refit_scene(self._ctx, ptr if n else None, n, st))
        self.sphere_count = n

    def set_scene_device(self, spheres_dev, refit: bool = False, stream=None) -> None:
        """Spheres already on the device: a contiguous uint8 cuda tensor [n, 80]."""
        import torch
        if not spheres_dev.is_cuda or spheres_dev.dtype != torch.uint8 or spheres_dev.dim() != 2 \
                or spheres_dev.shape[1] != 80 or not spheres_dev.is_contiguous():
            raise ValueError("spheres_dev must be a contiguous uint8 cuda tensor [n, 80]")
        n = int(spheres_dev.shape[0])
        st = _stream_ptr(stream, self.device)
        fn = self._lib.rt_refit_scene_device if refit else self._lib.rt_set_scene_device
        check(fn(self._ctx, spheres_dev.data_ptr() if n else None, n, st))
        self.sphere_count = n

    def tune(self, **kv) -> None:
        """Launch-plan parameters of this context (rt_debug_tune; tests and A/B timing only): e.g.
        ``tune(sample_chunks=7)``; None restores a default. No setting changes an image."""
        for k, v in kv.items():
            check(self._lib.rt_debug_tune(self._ctx, k.encode(), -1.0 if v is None else float(v)))

    def tile_costs(self) -> np.ndarray:
        """Per 8x8 tile of the last LBVH launch, the traced segments of its most expensive pixel
        (row-major tiles; empty before the first launch): the key the next launch hands tiles out
        by, longest first."""
        n = ctypes.c_uint64(0)
        check(self._lib.rt_debug_tile_cost(self._ctx, None, 0, ctypes.byref(n)))
        out = np.zeros(n.value, np.uint32)
        if n.value:
            check(self._lib.rt_debug_tile_cost(self._ctx, out.ctypes.data, n.value, ctypes.byref(n)))
        return out

    _SCENE_DTYPES = {0: (np.float32, 4), 1: (np.float32, 1), 2: (np.uint8, 32), 3: (np.uint32, 1),
                     4: (np.uint8, 32), 5: (np.uint8, 32), 6: (np.float32, 4), 7: (np.uint32, 1)}

    def scene_array(self, what: int) -> np.ndarray:
        """Diagnostic copy of one device scene array (rt_debug_scene); what 8 (scene) and 9 (grid
        layout) return a dict."""
        nbytes = ctypes.c_uint64(0)
        if what == 9:
            g = (ctypes.c_uint32 * 5)()
            check(self._lib.rt_debug_scene(self._ctx, 9, g, 20, ctypes.byref(nbytes)))
            return {"n": (int(g[0]), int(g[1]), int(g[2])), "cells": int(g[3]), "refs": int(g[4])}
        if what == 8:
            raw = (ctypes.c_uint8 * 32)()
            check(self._lib.rt_debug_scene(self._ctx, 8, raw, 32, ctypes.byref(nbytes)))
            u = np.frombuffer(bytes(raw), np.uint32)
            f = np.frombuffer(bytes(raw), np.float32)
            return {"n_spheres": int(u[0]), "n_big": int(u[1]), "n_nodes": int(u[2]),
                    "n_leaf": int(u[3]), "device_built": bool(u[4]), "small_rmax": float(f[6]),
                    "scene_radius": float(f[7])}
        self._lib.rt_debug_scene(self._ctx, what, None, 0, ctypes.byref(nbytes))   # size query
        buf = np.zeros(max(1, nbytes.value), np.uint8)
        if nbytes.value:
            check(self._lib.rt_debug_scene(self._ctx, what, buf.ctypes.data, nbytes.value, ctypes.byref(nbytes)))
        dt, w = self._SCENE_DTYPES[what]
        a = buf[: nbytes.value].view(dt)
        return a.reshape(-1, w) if w > 1 else a

    def closest_hits(self, rays, options: Optional[Options] = None):
        """Diagnostic (rt_debug_closest_hits): the closest hit of each of n host rays [n, 6] = (o, v)
        by the production walk `options` selects (accel, reserved[1] the form, reserved[0] bit 1
        force_regate, as render_device reads them), traced along the
        kernels' normalize(v). Returns (ids uint32 [n], 0xffffffff for none; t float32 [n],
        unspecified on a miss). Synchronous; launch_info() then describes the probe's launch."""
        r = np.ascontiguousarray(rays, np.float32)
        if r.ndim != 2 or r.shape[1] != 6:
            raise ValueError("rays must have shape [n, 6]")
        n = r.shape[0]
        ids = np.zeros(n, np.uint32)
        t = np.zeros(n, np.float32)
        check(self._lib.rt_debug_closest_hits(self._ctx, r.ctypes.data if n else None, n,
                                              ctypes.byref(options) if options is not None else None,
                                              ids.ctypes.data if n else None, t.ctypes.data if n else None))
        return ids, t

    def scatter_probe(self, rays, ids, t, seeds, form: int = 0) -> dict:
        """Diagnostic (rt_debug_scatter): one bounce of each of n given hits by the frames' shading
        code. Case i: host ray rays[i] = (o, v), traced along the kernels' normalize(v), hit sphere
        ids[i] at t[i] with the LCG in state seeds[i]. form 0 reads the sphere's records from the
        scene's global arrays, 1 from the static LDS table of the grid kernels (at most 512
        spheres). Returns {"p", "att", "sd" (the raw scatter direction), "d_next" (normalize of it,
        zeros without a scatter): float32 [n, 3]; "scatter", "seed": uint32 [n]}. Synchronous."""
        r = np.ascontiguousarray(rays, np.float32)
        if r.ndim != 2 or r.shape[1] != 6:
            raise ValueError("rays must have shape [n, 6]")
        n = r.shape[0]
        k = np.ascontiguousarray(ids, np.uint32)
        tt = np.ascontiguousarray(t, np.float32)
        sd = np.ascontiguousarray(seeds, np.uint32)
        if k.shape != (n,) or tt.shape != (n,) or sd.shape != (n,):
            raise ValueError("ids, t and seeds must have shape [n]")
        out = {name: np.zeros((n, 3), np.float32) for name in ("p", "att", "sd", "d_next")}
        out["scatter"] = np.zeros(n, np.uint32)
        out["seed"] = np.zeros(n, np.uint32)
        ptr = (lambda a: a.ctypes.data) if n else (lambda a: None)
        check(self._lib.rt_debug_scatter(self._ctx, ptr(r), ptr(k), ptr(tt), ptr(sd), n, form,
                                         *(ptr(out[name]) for name in ("p", "att", "sd", "d_next", "scatter", "seed"))))
        return out

    def render_device(self, rci: RenderCallInfo, accum, out, rows=None,
                      options: Optional[Options] = None, stream=None) -> None:
        """One band on this device, asynchronous on `stream` (torch current stream by default).

        accum: float32 cuda tensor [band_h, band_w, 4]; out: uint8 cuda tensor [band_h, band_w, 4];
        rows: optional int32/uint32 cuda tensor [band_h] of global row indices (strip tiling)."""
        bh, bw = int(accum.shape[0]), int(accum.shape[1])
        _check_dev_tensor(accum, "torch.float32", (bh, bw, 4))
        _check_dev_tensor(out, "torch.uint8", (bh, bw, 4))
        rows_ptr = None
        if rows is not None:
            if rows.numel() != bh or not rows.is_cuda or rows.element_size() != 4 or not rows.is_contiguous():
                raise ValueError("rows must be a contiguous 4-byte cuda tensor of band_h entries")
            rows_ptr = rows.data_ptr()
        check(self._lib.rt_render_device(self._ctx, ctypes.byref(rci), rows_ptr, bw, bh,
                                         accum.data_ptr(), out.data_ptr(),
                                         ctypes.byref(options) if options is not None else None,
                                         _stream_ptr(stream, self.device)))

    @staticmethod
    def _half_outputs(accum_a, accum_b, half_count, bh: int, bw: int) -> Optional["abi.HalfOutputs"]:
        """The rt_half_outputs of a halves frame, or None when no half output is given. accum_a and
        accum_b come together; the tensor checks follow accum and sample_count."""
        if accum_a is None and accum_b is None and half_count is None:
            return None
        if accum_a is None or accum_b is None:
            raise ValueError("give accum_a and accum_b together (half_count needs both)")
        _check_dev_tensor(accum_a, "torch.float32", (bh, bw, 4))
        _check_dev_tensor(accum_b, "torch.float32", (bh, bw, 4))
        h = abi.HalfOutputs()
        h.accum_a, h.accum_b, h.half_count, h.reserved = accum_a.data_ptr(), accum_b.data_ptr(), None, None
        if half_count is not None:
            if not half_count.is_cuda or half_count.element_size() != 4 or half_count.is_floating_point() \
                    or not half_count.is_contiguous() or tuple(half_count.shape) != (bh, bw):
                raise ValueError("half_count must be a contiguous 4-byte integer cuda tensor [band_h, band_w]")
            h.half_count = half_count.data_ptr()
        return h

    def render_adaptive(self, rci: RenderCallInfo, accum, out, sample_count=None, rows=None,
                        options: Optional[Options] = None, adaptive: Optional[Adaptive] = None,
                        stream=None, accum_a=None, accum_b=None, half_count=None) -> AdaptiveInfo:
        """One band rendered to a noise level (rt_render_adaptive_device): `adaptive` from
        make_adaptive(), rci.samplesPerRenderCall the cap, options with rng_mode HASH. Tensors as
        render_device; sample_count: optional 4-byte integer cuda tensor [band_h, band_w] that
        receives each texel's sample count. Ordered on `stream`, but blocks the host once per pass;
        the outputs are valid once `stream` completes. Returns the frame's AdaptiveInfo.
        accum_a, accum_b (float32 [band_h, band_w, 4], together) and the optional half_count (4-byte
        integer [band_h, band_w]) make it a halves frame (rt_render_adaptive_halves_device): they
        receive the frame's two half accumulators and n / 2 per texel, as denoise_variance and the
        temporal calls read them (sample_count=half_count there)."""
        if adaptive is None:
            raise ValueError("adaptive is required (make_adaptive)")
        bh, bw = int(accum.shape[0]), int(accum.shape[1])
        _check_dev_tensor(accum, "torch.float32", (bh, bw, 4))
        _check_dev_tensor(out, "torch.uint8", (bh, bw, 4))
        rows_ptr = None
        if rows is not None:
            if rows.numel() != bh or not rows.is_cuda or rows.element_size() != 4 or not rows.is_contiguous():
                raise ValueError("rows must be a contiguous 4-byte cuda tensor of band_h entries")
            rows_ptr = rows.data_ptr()
        count_ptr = None
        if sample_count is not None:
            if not sample_count.is_cuda or sample_count.element_size() != 4 or sample_count.is_floating_point() \
                    or not sample_count.is_contiguous() or tuple(sample_count.shape) != (bh, bw):
                raise ValueError("sample_count must be a contiguous 4-byte integer cuda tensor [band_h, band_w]")
            count_ptr = sample_count.data_ptr()
        info = AdaptiveInfo()
        halves = self._half_outputs(accum_a, accum_b, half_count, bh, bw)
        if halves is not None:
            check(self._lib.rt_render_adaptive_halves_device(self._ctx, ctypes.byref(rci), rows_ptr, bw, bh,
                                                             accum.data_ptr(), out.data_ptr(), count_ptr,
                                                             ctypes.byref(options) if options is not None else None,
                                                             ctypes.byref(adaptive), ctypes.byref(info),
                                                             ctypes.byref(halves), _stream_ptr(stream, self.device)))
            return info
        check(self._lib.rt_render_adaptive_device(self._ctx, ctypes.byref(rci), rows_ptr, bw, bh,
                                                  accum.data_ptr(), out.data_ptr(), count_ptr,
                                                  ctypes.byref(options) if options is not None else None,
                                                  ctypes.byref(adaptive), ctypes.byref(info),
                                                  _stream_ptr(stream, self.device)))
        return info

    def sample_map(self, width: int, height: int) -> "SampleMap":
        """A sample map of a band of width x height texels on this context (rt_sample_map_create):
        one count per 8x8 tile. Close it before the renderer."""
        m = SampleMap(self, width, height)
        self._maps.add(m)   # closed with the renderer at the latest
        return m

    def render_sample_map(self, rci: RenderCallInfo, accum, out, smap: "SampleMap", sample_count=None, rows=None,
                          options: Optional[Options] = None, stream=None) -> None:
        """One band with smap's per-tile sample counts (rt_render_sample_map_device): every pixel of a
        tile with count n holds what render_device gives at n samples; rci.samplesPerRenderCall is
        the cap (>= the map's max_count), options with rng_mode HASH. Tensors as render_adaptive.
        Asynchronous on `stream`: the whole frame is queued without a host wait."""
        bh, bw = int(accum.shape[0]), int(accum.shape[1])
        _check_dev_tensor(accum, "torch.float32", (bh, bw, 4))
        _check_dev_tensor(out, "torch.uint8", (bh, bw, 4))
        rows_ptr = None
        if rows is not None:
            if rows.numel() != bh or not rows.is_cuda or rows.element_size() != 4 or not rows.is_contiguous():
                raise ValueError("rows must be a contiguous 4-byte cuda tensor of band_h entries")
            rows_ptr = rows.data_ptr()
        count_ptr = None
        if sample_count is not None:
            if not sample_count.is_cuda or sample_count.element_size() != 4 or sample_count.is_floating_point() \
                    or not sample_count.is_contiguous() or tuple(sample_count.shape) != (bh, bw):
                raise ValueError("sample_count must be a contiguous 4-byte integer cuda tensor [band_h, band_w]")
            count_ptr = sample_count.data_ptr()
        check(self._lib.rt_render_sample_map_device(self._ctx, ctypes.byref(rci), rows_ptr, bw, bh,
                                                    accum.data_ptr(), out.data_ptr(), count_ptr,
                                                    ctypes.byref(options) if options is not None else None,
                                                    smap._map if smap is not None else None,
                                                    _stream_ptr(stream, self.device)))

    def render_sample_map_feedback(self, rci: RenderCallInfo, accum, out, smap: "SampleMap", feedback, sample_count=None,
                                   rows=None, options: Optional[Options] = None, tile_error=None, stream=None,
                                   accum_a=None, accum_b=None, half_count=None) -> None:
        """A feedback frame (rt_render_sample_map_feedback_device): smap's counts (rounded up to even)
        render as two halves, each tile's next count follows from their difference by `feedback`
        (make_feedback) and the map is re-planned with those counts on the device; nothing is read
        back. Tensors as render_sample_map; tile_error: optional contiguous int64 cuda tensor
        [tiles, 2] receiving (E, S) per tile. rci.samplesPerRenderCall is the cap: even, >=
        feedback.max_spp and what the map holds. accum_a, accum_b and half_count as in render_adaptive
        (rt_render_sample_map_feedback_halves_device): a tile of count n = 2 h at sample_base b gives
        accum_a = render_device at h samples from b, accum_b the same from b + h, half_count = h."""
        bh, bw = int(accum.shape[0]), int(accum.shape[1])
        _check_dev_tensor(accum, "torch.float32", (bh, bw, 4))
        _check_dev_tensor(out, "torch.uint8", (bh, bw, 4))
        rows_ptr = None
        if rows is not None:
            if rows.numel() != bh or not rows.is_cuda or rows.element_size() != 4 or not rows.is_contiguous():
                raise ValueError("rows must be a contiguous 4-byte cuda tensor of band_h entries")
            rows_ptr = rows.data_ptr()
        count_ptr = None
        if sample_count is not None:
            if not sample_count.is_cuda or sample_count.element_size() != 4 or sample_count.is_floating_point() \
                    or not sample_count.is_contiguous() or tuple(sample_count.shape) != (bh, bw):
                raise ValueError("sample_count must be a contiguous 4-byte integer cuda tensor [band_h, band_w]")
            count_ptr = sample_count.data_ptr()
        err_ptr = None
        if tile_error is not None:
            tiles = ((bw + 7) // 8) * ((bh + 7) // 8)
            if not tile_error.is_cuda or tile_error.element_size() != 8 or tile_error.is_floating_point() \
                    or not tile_error.is_contiguous() or tile_error.numel() != 2 * tiles:
                raise ValueError(f"tile_error must be a contiguous 8-byte integer cuda tensor of 2 x {tiles} entries")
            err_ptr = tile_error.data_ptr()
        halves = self._half_outputs(accum_a, accum_b, half_count, bh, bw)
        if halves is not None:
            check(self._lib.rt_render_sample_map_feedback_halves_device(
                self._ctx, ctypes.byref(rci), rows_ptr, bw, bh, accum.data_ptr(), out.data_ptr(), count_ptr,
                ctypes.byref(options) if options is not None else None, smap._map if smap is not None else None,
                ctypes.byref(feedback) if feedback is not None else None, err_ptr, ctypes.byref(halves),
                _stream_ptr(stream, self.device)))
            return
        check(self._lib.rt_render_sample_map_feedback_device(self._ctx, ctypes.byref(rci), rows_ptr, bw, bh,
                                                             accum.data_ptr(), out.data_ptr(), count_ptr,
                                                             ctypes.byref(options) if options is not None else None,
                                                             smap._map if smap is not None else None,
                                                             ctypes.byref(feedback) if feedback is not None else None,
                                                             err_ptr, _stream_ptr(stream, self.device)))

    def render_features(self, rci: RenderCallInfo, feat0, feat1, samples: int = 16, rows=None,
                        options: Optional[Options] = None, stream=None) -> None:
        """First-hit feature buffers of one band (rt_render_features_device): feat0 = (sum albedo.rgb,
        sum hit), feat1 = (sum n.xyz, sum depth) over the camera rays of samples [sample_base,
        sample_base + samples) of the HASH stream, float32 cuda tensors [band_h, band_w, 4]. options
        as render_device with rng_mode HASH (the default here) and accumulate off; rows as
        render_device. Asynchronous on `stream`, no host wait."""
        bh, bw = int(feat0.shape[0]), int(feat0.shape[1])
        _check_dev_tensor(feat0, "torch.float32", (bh, bw, 4))
        _check_dev_tensor(feat1, "torch.float32", (bh, bw, 4))
        rows_ptr = None
        if rows is not None:
            if rows.numel() != bh or not rows.is_cuda or rows.element_size() != 4 or not rows.is_contiguous():
                raise ValueError("rows must be a contiguous 4-byte cuda tensor of band_h entries")
            rows_ptr = rows.data_ptr()
        if options is None:
            options = make_options(rng_mode=HASH)
        check(self._lib.rt_render_features_device(self._ctx, ctypes.byref(rci), rows_ptr, bw, bh,
                                                  feat0.data_ptr(), feat1.data_ptr(), samples,
                                                  ctypes.byref(options), _stream_ptr(stream, self.device)))

    def denoise(self, accum, feat0, feat1, feature_samples: int, out, spp: Optional[int] = None,
                sample_count=None, out_mean=None, params: Optional["abi.Denoise"] = None, stream=None) -> None:
        """Edge-avoiding denoise of a summed accumulator (rt_denoise_device), guided by render_features'
        buffers of `feature_samples` samples. accum, feat0, feat1: float32 cuda tensors [band_h,
        band_w, 4] of contiguous image rows; out: uint8 [band_h, band_w, 4]; the texels' sample counts
        are `spp` or the 4-byte integer cuda tensor sample_count [band_h, band_w] (exactly one of
        them); out_mean: optional float32 [band_h, band_w, 4] receiving (mean, 1); params from
        make_denoise() (None: the defaults). The outputs must not alias the inputs. Asynchronous on
        `stream`; no host wait once the context's band buffers stand."""
        bh, bw = int(accum.shape[0]), int(accum.shape[1])
        for t in (accum, feat0, feat1):
            _check_dev_tensor(t, "torch.float32", (bh, bw, 4))
        _check_dev_tensor(out, "torch.uint8", (bh, bw, 4))
        if (spp is None) == (sample_count is None):
            raise ValueError("give exactly one of spp and sample_count")
        count_ptr = None
        if sample_count is not None:
            if not sample_count.is_cuda or sample_count.element_size() != 4 or sample_count.is_floating_point() \
                    or not sample_count.is_contiguous() or tuple(sample_count.shape) != (bh, bw):
                raise ValueError("sample_count must be a contiguous 4-byte integer cuda tensor [band_h, band_w]")
            count_ptr = sample_count.data_ptr()
        mean_ptr = None
        if out_mean is not None:
            _check_dev_tensor(out_mean, "torch.float32", (bh, bw, 4))
            mean_ptr = out_mean.data_ptr()
        check(self._lib.rt_denoise_device(self._ctx, accum.data_ptr(), count_ptr, int(spp or 0),
                                          feat0.data_ptr(), feat1.data_ptr(), feature_samples, bw, bh,
                                          ctypes.byref(params) if params is not None else None,
                                          mean_ptr, out.data_ptr(), _stream_ptr(stream, self.device)))

    def denoise_variance(self, accum_a, accum_b, feat0, feat1, feature_samples: int, out,
                         half_spp: Optional[int] = None, half_count=None, out_mean=None,
                         params: Optional["abi.DenoiseVariance"] = None, stream=None) -> None:
        """Variance-guided denoise of a frame rendered as two halves (rt_denoise_variance_device):
        accum_a and accum_b are the halves' summed accumulators (render_halves, or two sample-map
        frames), each texel holding `half_spp` samples or those of the 4-byte integer cuda tensor
        half_count [band_h, band_w] (exactly one of them). The other tensors, params
        (make_denoise_variance(); None: the defaults) and the stream are as for denoise."""
        bh, bw = int(accum_a.shape[0]), int(accum_a.shape[1])
        for t in (accum_a, accum_b, feat0, feat1):
            _check_dev_tensor(t, "torch.float32", (bh, bw, 4))
        _check_dev_tensor(out, "torch.uint8", (bh, bw, 4))
        if (half_spp is None) == (half_count is None):
            raise ValueError("give exactly one of half_spp and half_count")
        count_ptr = None
        if half_count is not None:
            if not half_count.is_cuda or half_count.element_size() != 4 or half_count.is_floating_point() \
                    or not half_count.is_contiguous() or tuple(half_count.shape) != (bh, bw):
                raise ValueError("half_count must be a contiguous 4-byte integer cuda tensor [band_h, band_w]")
            count_ptr = half_count.data_ptr()
        mean_ptr = None
        if out_mean is not None:
            _check_dev_tensor(out_mean, "torch.float32", (bh, bw, 4))
            mean_ptr = out_mean.data_ptr()
        check(self._lib.rt_denoise_variance_device(self._ctx, accum_a.data_ptr(), accum_b.data_ptr(), count_ptr,
                                                   int(half_spp or 0), feat0.data_ptr(), feat1.data_ptr(),
                                                   feature_samples, bw, bh,
                                                   ctypes.byref(params) if params is not None else None,
                                                   mean_ptr, out.data_ptr(), _stream_ptr(stream, self.device)))

    def temporal(self, width: int, height: int) -> "Temporal":
        """The state of a temporal stage for a band of width x height texels on this context
        (rt_temporal_create): every texel's history is empty. Close it before the renderer."""
        t = Temporal(self, width, height)
        self._maps.add(t)   # closed with the renderer at the latest
        return t

    @staticmethod
    def _temporal_pointers(temporal, floats, accum_b, out_b, out_rgba8, history_len, spp, sample_count):
        """The tensor checks the two temporal calls share; `floats` are their required float32 planes.
        Returns the pointers (sample_count, out_rgba8, history_len), None for what is not given."""
        if not isinstance(temporal, Temporal) or not temporal._state:
            raise ValueError("temporal is closed or not a Temporal")
        bh, bw = temporal.height, temporal.width
        if (accum_b is None) != (out_b is None):
            raise ValueError("give accum_b and out_b together or neither")
        for t in tuple(floats) + (() if accum_b is None else (accum_b, out_b)):
            _check_dev_tensor(t, "torch.float32", (bh, bw, 4))
        if (spp is None) == (sample_count is None):
            raise ValueError("give exactly one of spp and sample_count")

        def words(t, name):
            if t is None:
                return None
            if not t.is_cuda or t.element_size() != 4 or t.is_floating_point() or not t.is_contiguous() \
                    or tuple(t.shape) != (bh, bw):
                raise ValueError(f"{name} must be a contiguous 4-byte integer cuda tensor [band_h, band_w]")
            return t.data_ptr()
        count_ptr, len_ptr = words(sample_count, "sample_count"), words(history_len, "history_len")
        rgba_ptr = None
        if out_rgba8 is not None:
            _check_dev_tensor(out_rgba8, "torch.uint8", (bh, bw, 4))
            rgba_ptr = out_rgba8.data_ptr()
        return count_ptr, rgba_ptr, len_ptr

    def temporal_accumulate(self, temporal: "Temporal", accum_a, feat0, feat1, feature_samples: int, out_a,
                            accum_b=None, out_b=None, out_rgba8=None, history_len=None, spp: Optional[int] = None,
                            sample_count=None, params: Optional["abi.TemporalParams"] = None, stream=None) -> None:
        """One frame into `temporal`'s history (rt_temporal_accumulate_device): accum_a (and accum_b,
        a frame rendered as two halves) are summed accumulators of the temporal's band, each texel
        holding `spp` samples or those of the 4-byte integer cuda tensor sample_count [band_h, band_w]
        (exactly one of them); feat0 and feat1 are render_features' buffers of `feature_samples`
        samples, rendered at the same sample_base every frame. out_a (and out_b, given exactly when
        accum_b is) receive the integrated accumulators at 1 sample: denoise reads out_a with spp=1,
        denoise_variance out_a and out_b with half_spp=1. Optional: out_rgba8, uint8 [band_h, band_w,
        4], the integrated mean's bytes; history_len, a 4-byte integer tensor [band_h, band_w], the
        frames every texel's history holds. The float tensors are float32 cuda [band_h, band_w, 4];
        params from make_temporal() (None: the defaults). Asynchronous on `stream`, no host wait."""
        count_ptr, rgba_ptr, len_ptr = self._temporal_pointers(temporal, (accum_a, feat0, feat1, out_a), accum_b, out_b,
                                                               out_rgba8, history_len, spp, sample_count)
        check(self._lib.rt_temporal_accumulate_device(
            self._ctx, temporal._state, accum_a.data_ptr(), None if accum_b is None else accum_b.data_ptr(), count_ptr,
            int(spp or 0), feat0.data_ptr(), feat1.data_ptr(), feature_samples,
            ctypes.byref(params) if params is not None else None, out_a.data_ptr(),
            None if out_b is None else out_b.data_ptr(), rgba_ptr, len_ptr, _stream_ptr(stream, self.device)))

    def motion(self, width: int, height: int) -> "Motion":
        """The state of a motion pass for a band of width x height texels on this context
        (rt_motion_create): its scratch and the previous frame, which is the current one until
        set_previous or keep_current says otherwise. Close it before the renderer."""
        m = Motion(self, width, height)
        self._maps.add(m)   # closed with the renderer at the latest
        return m

    def render_motion(self, motion: "Motion", rci: RenderCallInfo, motion_out, options: Optional[Options] = None,
                      stream=None) -> None:
        """Where the surface seen through each texel's centre stood in the previous frame's image
        (rt_render_motion_device): motion_out, a float32 cuda tensor [band_h, band_w, 4] of the
        motion's band (contiguous image rows from rci.offset), receives (sx, sy, dzm, ok) per texel,
        sx and sy in band coordinates with texel centres at + 0.5. options selects the walk as for a
        frame. Asynchronous on `stream`, no host wait."""
        if not isinstance(motion, Motion) or not motion._state:
            raise ValueError("motion is closed or not a Motion")
        _check_dev_tensor(motion_out, "torch.float32", (motion.height, motion.width, 4))
        check(self._lib.rt_render_motion_device(self._ctx, motion._state, ctypes.byref(rci), motion_out.data_ptr(),
                                                ctypes.byref(options) if options is not None else None,
                                                _stream_ptr(stream, self.device)))

    def temporal_reproject(self, temporal: "Temporal", accum_a, feat0, feat1, feature_samples: int, motion, out_a,
                           accum_b=None, out_b=None, out_rgba8=None, history_len=None, spp: Optional[int] = None,
                           sample_count=None, params: Optional["abi.TemporalParams"] = None, stream=None) -> None:
        """temporal_accumulate with every texel's history fetched from where `motion` (render_motion's
        float32 cuda tensor [band_h, band_w, 4] of the same band) says its surface was
        (rt_temporal_reproject_device): one tap where nothing moved, four bilinear taps elsewhere,
        each checked against the guide. The other arguments are temporal_accumulate's. The state's
        first reprojected call allocates its second plane set; later ones queue one launch."""
        count_ptr, rgba_ptr, len_ptr = self._temporal_pointers(temporal, (accum_a, feat0, feat1, motion, out_a), accum_b,
                                                               out_b, out_rgba8, history_len, spp, sample_count)
        check(self._lib.rt_temporal_reproject_device(
            self._ctx, temporal._state, accum_a.data_ptr(), None if accum_b is None else accum_b.data_ptr(), count_ptr,
            int(spp or 0), feat0.data_ptr(), feat1.data_ptr(), feature_samples, motion.data_ptr(),
            ctypes.byref(params) if params is not None else None, out_a.data_ptr(),
            None if out_b is None else out_b.data_ptr(), rgba_ptr, len_ptr, _stream_ptr(stream, self.device)))

    def render_halves(self, rci: RenderCallInfo, accum_a, accum_b, out, rows=None,
                      options: Optional[Options] = None, stream=None) -> None:
        """A frame of rci.samplesPerRenderCall = 2 h samples per pixel as the two halves
        denoise_variance reads: two render_device calls of h samples, accum_a at options.sample_base
        and accum_b at sample_base + h, in the HASH stream (the default options; anything else is a
        ValueError), so accum_a + accum_b holds the samples of the one frame. `out` receives the
        second half's bytes and is scratch."""
        n = int(rci.samplesPerRenderCall)
        if n % 2:
            raise ValueError("render_halves needs an even samplesPerRenderCall")
        if options is None:
            options = make_options(rng_mode=HASH)
        if options.rng_mode != HASH:
            raise ValueError("render_halves needs the counter-based stream (rng_mode HASH)")
        if options.accumulate:
            raise ValueError("render_halves does not accumulate")
        half = RenderCallInfo.from_buffer_copy(bytes(rci))
        half.samplesPerRenderCall = n // 2
        second = Options.from_buffer_copy(bytes(options))
        second.sample_base = options.sample_base + n // 2
        self.render_device(half, accum_a, out, rows=rows, options=options, stream=stream)
        self.render_device(half, accum_b, out, rows=rows, options=second, stream=stream)

    def denoise_lds_steps(self, max_step: int) -> None:
        """Diagnostic (rt_debug_denoise_lds_steps): denoise iterations of step <= max_step (0, 1, 2
        or 4, the default) stage their taps in LDS; the image does not depend on it."""
        check(self._lib.rt_debug_denoise_lds_steps(self._ctx, max_step))

    def adaptive_resolve(self, accum, out, count: int, sample_count=None, accum_a=None, accum_b=None, half_count=None,
                         stream=None) -> None:
        """Timing (rt_debug_adaptive_resolve): the resolve of adaptive and feedback frames alone, one
        launch over the context's zero planes with `count` as every tile's count; with accum_a and
        accum_b the resolve that also hands the halves over. Tensors as render_adaptive."""
        bh, bw = int(accum.shape[0]), int(accum.shape[1])
        _check_dev_tensor(accum, "torch.float32", (bh, bw, 4))
        _check_dev_tensor(out, "torch.uint8", (bh, bw, 4))
        if sample_count is not None and (not sample_count.is_cuda or sample_count.element_size() != 4 or
                                         not sample_count.is_contiguous() or tuple(sample_count.shape) != (bh, bw)):
            raise ValueError("sample_count must be a contiguous 4-byte integer cuda tensor [band_h, band_w]")
        halves = self._half_outputs(accum_a, accum_b, half_count, bh, bw)
        check(self._lib.rt_debug_adaptive_resolve(self._ctx, bw, bh, count, accum.data_ptr(), out.data_ptr(),
                                                  None if sample_count is None else sample_count.data_ptr(),
                                                  ctypes.byref(halves) if halves is not None else None,
                                                  _stream_ptr(stream, self.device)))

    def host_waits(self) -> int:
        """Host waits inside calls documented as queued without one (rt_debug_host_waits)."""
        v = ctypes.c_uint64()
        check(self._lib.rt_debug_host_waits(self._ctx, ctypes.byref(v)))
        return int(v.value)

    def stats(self) -> Stats:
        st = Stats()
        check(self._lib.rt_get_stats(self._ctx, ctypes.byref(st)))
        return st

    def steals(self) -> int:
        """Tail steals of the last instrumented launch (count_tests; rt_debug_steals; counter-based
        stream only)."""
        v = ctypes.c_uint64()
        check(self._lib.rt_debug_steals(self._ctx, ctypes.byref(v)))
        return int(v.value)

    def grid_cells(self) -> dict:
        """Of the last instrumented (count_tests) grid-walk launch: cells visited and visited cells
        without references (rt_debug_grid_cells)."""
        v = (ctypes.c_uint64 * 2)()
        check(self._lib.rt_debug_grid_cells(self._ctx, v))
        return {"cells": int(v[0]), "empty": int(v[1])}

    def launch_info(self) -> dict:
        """Of the last launch: sample chunks per pixel (of the LPT order's tail ranks; head_chunks:
        of its head ranks, None when there is no head), the kernel form it ran, its dynamic LDS
        bytes, the CU count, whether its grid walk was the one-layer form (flat_grid: the grid is
        one cell thick in y), whether its camera rays started at the camera position itself
        (pinhole_origin) and whether it ran the camera-batch form of the LDS grid kernel
        (camera_batches) (rt_debug_launch_info)."""
        v = (ctypes.c_uint32 * 4)()
        check(self._lib.rt_debug_launch_info(self._ctx, v))
        forms = {1: "brute", 2: "lbvh-global", 3: "lbvh-lds", 4: "lbvh-octant-lds", 5: "lbvh-treelet", 6: "grid-lds", 7: "grid-global",
                 8: "grid-lds-coop", 9: "grid-global-coop", 10: "grid-lds-rec", 11: "grid-lds-cq", 12: "grid-lds-rec-cq"}
        return {"chunks": int(v[0]) & 0xffff, "head_chunks": (int(v[0]) >> 16) or None,
                "form": forms.get(int(v[1]) & 0xffff, str(v[1])), "lds_bytes": int(v[2]), "cus": int(v[3]),
                "flat_grid": bool((int(v[1]) >> 16) & 1), "pinhole_origin": bool((int(v[1]) >> 17) & 1),
                "camera_batches": bool((int(v[1]) >> 18) & 1)}

    def launch_plan(self):
        """(abi.LaunchInputs, abi.LaunchPlan) of the last launch (rt_debug_launch_plan): the inputs
        carry the occupancies the launch queried, so rtvk.launch_plan(inputs) recomputes the plan."""
        inputs, plan = abi.LaunchInputs(), abi.LaunchPlan()
        check(self._lib.rt_debug_launch_plan(self._ctx, ctypes.byref(inputs), ctypes.sizeof(inputs),
                                             ctypes.byref(plan), ctypes.sizeof(plan)))
        return inputs, plan

    def scatter_rows(self, src_accum, src_rgba8, rows, dst_accum, dst_rgba8, stream=None) -> None:
        """dst[rows[i]] = src[i] (device), the reorder after a multi-GPU gather; either image may
        be None (both its source and destination)."""
        src = src_rgba8 if src_rgba8 is not None else src_accum
        dst = dst_rgba8 if dst_rgba8 is not None else dst_accum
        if src is None or dst is None:
            raise ValueError("nothing to scatter")
        n, w, dh = int(src.shape[0]), int(src.shape[1]), int(dst.shape[0])
        if (src_rgba8 is None) != (dst_rgba8 is None) or (src_accum is None) != (dst_accum is None):
            raise ValueError("each image needs both a source and a destination, or neither")
        if src_rgba8 is not None:
            _check_dev_tensor(src_rgba8, "torch.uint8", (n, w, 4))
            _check_dev_tensor(dst_rgba8, "torch.uint8", (dh, w, 4))
        if src_accum is not None:
            _check_dev_tensor(src_accum, "torch.float32", (n, w, 4))
            _check_dev_tensor(dst_accum, "torch.float32", (dh, w, 4))
        self._check_rows(rows, n, dh)
        check(self._lib.rt_scatter_rows(self._ctx, src_accum.data_ptr() if src_accum is not None else None,
                                        src_rgba8.data_ptr() if src_rgba8 is not None else None,
                                        rows.data_ptr(), n, w, dh,
                                        dst_accum.data_ptr() if dst_accum is not None else None,
                                        dst_rgba8.data_ptr() if dst_rgba8 is not None else None,
                                        _stream_ptr(stream, self.device)))

    @staticmethod
    def _check_rows(rows, n, limit):
        if rows.numel() != n or not rows.is_cuda or rows.element_size() != 4 or not rows.is_contiguous():
            raise ValueError("rows must be a contiguous 4-byte cuda tensor of one entry per band row")
        if n and (int(rows.min()) < 0 or int(rows.max()) >= limit):
            raise ValueError(f"rows must lie in [0, {limit})")

    def gather_rows(self, src_accum, rows, dst_accum, stream=None) -> None:
        """dst[i] = src[rows[i]] (device float4 accumulators), the inverse of scatter_rows."""
        sh, w = int(src_accum.shape[0]), int(src_accum.shape[1])
        n = int(dst_accum.shape[0])
        _check_dev_tensor(src_accum, "torch.float32", (sh, w, 4))
        _check_dev_tensor(dst_accum, "torch.float32", (n, w, 4))
        self._check_rows(rows, n, sh)
        check(self._lib.rt_gather_rows(self._ctx, src_accum.data_ptr(), rows.data_ptr(), n, w, sh,
                                       dst_accum.data_ptr(), _stream_ptr(stream, self.device)))

    def resolve_rgba8(self, accum, spp: int, out, stream=None) -> None:
        """out = rgba8 tonemap of the summed float4 accumulator `accum` (device tensors), exactly
        as the trace kernel stores a pixel (rt_resolve_rgba8)."""
        n = accum.numel() // 4
        if out.numel() != 4 * n:
            raise ValueError("out must hold 4 bytes per accumulator texel")
        check(self._lib.rt_resolve_rgba8(self._ctx, accum.data_ptr(), n, spp, out.data_ptr(),
                                         _stream_ptr(stream, self.device)))

    def launch_ms(self, back: int = 0) -> float:
        """Trace-kernel ms of the launch `back` launches before the most recent one (rt_launch_ms:
        waits for that launch only, not for the ones queued after it)."""
        v = ctypes.c_float()
        check(self._lib.rt_launch_ms(self._ctx, back, ctypes.byref(v)))
        return float(v.value)

    def launch_row_weights(self, band_rows: int, back: int = 0) -> np.ndarray:
        """Per band row of the launch `back` launches before the most recent one, its share of the
        launch's work from the tile-cost record (rt_launch_row_weights; ratios only)."""
        w = np.zeros(max(1, band_rows), np.float64)
        check(self._lib.rt_launch_row_weights(self._ctx, back, w.ctypes.data, band_rows))
        return w[:band_rows]

    def kernel_times(self, n: int = 64) -> list:
        """Trace-kernel durations (ms) of the last `n` launches (at most 64 kept), oldest first:
        HIP events recorded around the kernel on its launch stream (rt_debug_kernel_times)."""
        buf = (ctypes.c_float * max(1, n))()
        got = ctypes.c_uint32(0)
        check(self._lib.rt_debug_kernel_times(self._ctx, buf, n, ctypes.byref(got)))
        return [float(buf[i]) for i in range(got.value)]


class SampleMap:
    """Per-tile sample counts of a band on one Renderer (rt_sample_map). Setting
    the map is the one synchronous step; Renderer.render_sample_map then queues whole frames."""

    def __init__(self, renderer: Renderer, width: int, height: int):
        self._lib = renderer._lib
        self._map = ctypes.c_void_p()
        self.renderer = renderer
        self.width, self.height = int(width), int(height)
        self.tiles_x, self.tiles_y = (self.width + 7) // 8, (self.height + 7) // 8
        check(self._lib.rt_sample_map_create(renderer._ctx, self.width, self.height, ctypes.byref(self._map)))

    def close(self) -> None:
        if self._map:
            self._lib.rt_sample_map_destroy(self._map)
            self._map = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set(self, tile_counts, quantum: int = 0, stream=None) -> abi.SampleMapInfo:
        """tile_counts: contiguous 4-byte integer cuda tensor of tiles_y x tiles_x counts (row-major;
        any shape with that many entries), written by earlier work on `stream`; quantum rounds every
        non-zero count up to a multiple of itself (rt_sample_map_set_device)."""
        n = self.tiles_x * self.tiles_y
        if not tile_counts.is_cuda or tile_counts.element_size() != 4 or tile_counts.is_floating_point() \
                or not tile_counts.is_contiguous() or tile_counts.numel() != n:
            raise ValueError(f"tile_counts must be a contiguous 4-byte integer cuda tensor of {n} entries")
        info = abi.SampleMapInfo()
        check(self._lib.rt_sample_map_set_device(self._map, tile_counts.data_ptr(), quantum,
                                                 _stream_ptr(stream, self.renderer.device), ctypes.byref(info)))
        return info

    def set_from_adaptive(self, quantum: int = 0, stream=None) -> abi.SampleMapInfo:
        """The count table of the renderer's last completed adaptive frame of this band size
        (rt_sample_map_set_from_adaptive)."""
        info = abi.SampleMapInfo()
        check(self._lib.rt_sample_map_set_from_adaptive(self._map, quantum, _stream_ptr(stream, self.renderer.device),
                                                        ctypes.byref(info)))
        return info

    def set_async(self, tile_counts, unit: int = 0, count_cap: int = 1 << 19, stream=None) -> None:
        """The set call without a host wait (rt_sample_map_set_device_async): tile_counts as in set(),
        clamped to count_cap and planned on the device behind the frames queued on the map, under the
        one-launch schedule with units of `unit` samples (0: automatic from count_cap), doubled until
        the table fits the map's block capacity. The map is device-planned afterwards: frames need
        samplesPerRenderCall >= count_cap; info, schedule_info and debug_blocks wait for the planner."""
        n = self.tiles_x * self.tiles_y
        if not tile_counts.is_cuda or tile_counts.element_size() != 4 or tile_counts.is_floating_point() \
                or not tile_counts.is_contiguous() or tile_counts.numel() != n:
            raise ValueError(f"tile_counts must be a contiguous 4-byte integer cuda tensor of {n} entries")
        check(self._lib.rt_sample_map_set_device_async(self._map, tile_counts.data_ptr(), unit, count_cap,
                                                       _stream_ptr(stream, self.renderer.device)))

    def debug_feedback(self) -> dict:
        """What the map's feedback frames left on the device (rt_debug_sample_map_feedback): {next:
        the counts the last frame's update chose, raised, lowered: tiles moved over all frames}."""
        nxt = np.zeros(self.tiles_x * self.tiles_y, np.uint32)
        up, down = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(self._lib.rt_debug_sample_map_feedback(self._map, nxt.ctypes.data, ctypes.byref(up), ctypes.byref(down)))
        return {"next": nxt, "raised": up.value, "lowered": down.value}

    def debug_limit_blocks(self, limit: int) -> None:
        """Tests: set_async plans for at most max(limit, tiles) table entries (0: the map's capacity)."""
        check(self._lib.rt_debug_sample_map_limit_blocks(self._map, limit))

    @property
    def info(self) -> abi.SampleMapInfo:
        info = abi.SampleMapInfo()
        check(self._lib.rt_sample_map_get_info(self._map, ctypes.byref(info)))
        return info

    def schedule(self, schedule: int, unit_samples: int = 0) -> None:
        """The schedule the next set call plans by (rt_sample_map_set_schedule): abi.SAMPLE_MAP_LEVELS
        (the default: one launch per distinct count) or abi.SAMPLE_MAP_ONE_LAUNCH (one launch of a block
        table, any number of distinct counts) with units of at most unit_samples samples (0: automatic)."""
        check(self._lib.rt_sample_map_set_schedule(self._map, schedule, unit_samples))

    def schedule_info(self) -> dict:
        """{schedule, unit_samples, n_blocks} of the plan the map holds (rt_sample_map_get_schedule)."""
        sched, unit, nb = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
        check(self._lib.rt_sample_map_get_schedule(self._map, ctypes.byref(sched), ctypes.byref(unit), ctypes.byref(nb)))
        return {"schedule": sched.value, "unit_samples": unit.value, "n_blocks": nb.value}

    def debug_blocks(self):
        """The block table the device holds (rt_debug_sample_map_blocks): uint32 [n_blocks, 4] rows
        (tile, s0, s1, 0), empty for a level plan."""
        nb = ctypes.c_uint64(0)
        check(self._lib.rt_debug_sample_map_blocks(self._map, None, 0, ctypes.byref(nb)))
        blocks = np.zeros((nb.value, 4), np.uint32)
        if nb.value:
            check(self._lib.rt_debug_sample_map_blocks(self._map, blocks.ctypes.data, nb.value, ctypes.byref(nb)))
        return blocks

    def debug_plan(self) -> dict:
        """What the device holds after the last set call (rt_debug_sample_map), in sample_map_plan's form."""
        n = self.tiles_x * self.tiles_y
        order, quantised = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        levels = np.zeros(abi.SAMPLE_MAP_MAX_LEVELS, np.uint32)
        level_tiles = np.zeros(abi.SAMPLE_MAP_MAX_LEVELS, np.uint32)
        check(self._lib.rt_debug_sample_map(self._map, order.ctypes.data, levels.ctypes.data, level_tiles.ctypes.data,
                                            quantised.ctypes.data))
        j = min(self.info.levels, abi.SAMPLE_MAP_MAX_LEVELS)
        return {"order": order, "levels": levels[:j].copy(), "level_tiles": level_tiles[:j].copy(),
                "quantised": quantised}


class Temporal:
    """The history of a temporal stage for one band on one Renderer (rt_temporal):
    per texel the integrated colour, the number of frames it holds and the last frame's guide.
    Renderer.temporal_accumulate feeds it one frame at a time."""

    def __init__(self, renderer: Renderer, width: int, height: int):
        self._lib = renderer._lib
        self._state = ctypes.c_void_p()
        self.renderer = renderer
        self.width, self.height = int(width), int(height)
        check(self._lib.rt_temporal_create(renderer._ctx, self.width, self.height, ctypes.byref(self._state)))

    def close(self) -> None:
        if self._state:
            self._lib.rt_temporal_destroy(self._state)
            self._state = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, stream=None) -> None:
        """Empties every texel's history (rt_temporal_reset), queued on `stream` without a host wait:
        the next temporal_accumulate is a first frame."""
        if not self._state:
            raise ValueError("the Temporal is closed")
        check(self._lib.rt_temporal_reset(self._state, _stream_ptr(stream, self.renderer.device)))


class Motion:
    """The state of a motion pass for one band on one Renderer (rt_motion): the
    pass's device scratch and the previous frame, its camera and sphere centres.
    Renderer.render_motion reads it; a frame loop calls render_motion, then keep_current."""

    def __init__(self, renderer: Renderer, width: int, height: int):
        self._lib = renderer._lib
        self._state = ctypes.c_void_p()
        self.renderer = renderer
        self.width, self.height = int(width), int(height)
        check(self._lib.rt_motion_create(renderer._ctx, self.width, self.height, ctypes.byref(self._state)))

    def close(self) -> None:
        if self._state:
            self._lib.rt_motion_destroy(self._state)
            self._state = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_previous(self, spheres, prev_rci: RenderCallInfo, stream=None) -> None:
        """The previous frame given explicitly (rt_motion_set_previous): its spheres (ctypes Sphere
        array or (n, 80) uint8 records, as Renderer.set_scene takes them) and its RenderCallInfo."""
        if not self._state:
            raise ValueError("the Motion is closed")
        buf = spheres if not isinstance(spheres, np.ndarray) else np.ascontiguousarray(spheres, np.uint8)
        n = len(spheres)
        ptr = ctypes.addressof(buf) if not isinstance(buf, np.ndarray) else buf.ctypes.data
        check(self._lib.rt_motion_set_previous(self._state, ptr if n else None, n, ctypes.byref(prev_rci),
                                               _stream_ptr(stream, self.renderer.device)))

    def keep_current(self, rci: RenderCallInfo, stream=None) -> None:
        """The renderer's current scene and `rci` become the previous frame (rt_motion_keep_current),
        queued on `stream` behind the scene's upload or build."""
        if not self._state:
            raise ValueError("the Motion is closed")
        check(self._lib.rt_motion_keep_current(self.renderer._ctx, self._state, ctypes.byref(rci),
                                               _stream_ptr(stream, self.renderer.device)))


def motion_check(band_w: int, band_h: int, rci: Optional[RenderCallInfo], prev_rci: Optional[RenderCallInfo] = None) -> None:
    """rt_motion_check (host only): raises RtError where Renderer.render_motion would refuse its band
    or its two RenderCallInfo."""
    check(load_library().rt_motion_check(band_w, band_h, ctypes.byref(rci) if rci is not None else None,
                                         ctypes.byref(prev_rci) if prev_rci is not None else None))


def sample_map_block_plan(counts, quantum: int = 0, unit_samples: int = 0) -> dict:
    """The block table of a host table under SAMPLE_MAP_ONE_LAUNCH (rt_sample_map_block_plan; host
    only): {blocks: uint32 [n_blocks, 4] rows (tile, s0, s1, 0), unit_samples: the U used}. unit_samples
    0: automatic. Raises RtError for what the library refuses (a count or unit above 2^19, a table of
    2^25 blocks or more)."""
    c = np.ascontiguousarray(np.asarray(counts).reshape(-1), np.uint32)
    n = len(c)
    lib = load_library()
    nb, used = ctypes.c_uint64(0), ctypes.c_uint32(0)
    check(lib.rt_sample_map_block_plan(c.ctypes.data if n else None, n, quantum, unit_samples, None, 0,
                                       ctypes.byref(nb), ctypes.byref(used)))
    blocks = np.zeros((nb.value, 4), np.uint32)
    check(lib.rt_sample_map_block_plan(c.ctypes.data if n else None, n, quantum, unit_samples,
                                       blocks.ctypes.data if nb.value else None, nb.value, None, None))
    return {"blocks": blocks, "unit_samples": used.value}


def sample_map_device_capacity(n_tiles: int, count_cap: int, unit: int = 0) -> int:
    """Entries of the block table a device-planned map of n_tiles tiles is allocated for
    (csrc/rt_sample_map_device.h device_capacity), restated: min(tiles x ceil(cap / U0), 2^22)."""
    u0 = unit or min(128, max(32, count_cap // 32))
    return min(n_tiles * max(1, -(-count_cap // u0)), 1 << 22)


def sample_map_device_unit(counts, count_cap: int, unit: int = 0, capacity: int | None = None) -> int:
    """The unit the device planner chooses for the host table `counts` (rt_sample_map_device_unit; host
    only). capacity None: the capacity of a map of len(counts) tiles."""
    c = np.ascontiguousarray(np.asarray(counts).reshape(-1), np.uint32)
    if capacity is None:
        capacity = sample_map_device_capacity(len(c), count_cap, unit)
    used = ctypes.c_uint32(0)
    check(load_library().rt_sample_map_device_unit(c.ctypes.data if len(c) else None, len(c), count_cap, unit, capacity,
                                                   ctypes.byref(used)))
    return used.value


def sample_map_feedback_count(E: int, S: int, n: int, m: int, thr_q16: int, min_spp: int, max_spp: int) -> int:
    """The next count of a tile under the feedback rule (rt_sample_map_feedback_count; host only)."""
    nxt = ctypes.c_uint32(0)
    check(load_library().rt_sample_map_feedback_count(E, S, n, m, thr_q16, min_spp, max_spp, ctypes.byref(nxt)))
    return nxt.value


def hand_out(n_units: int, reserve: int, grid_waves: int) -> tuple[int, int]:
    """(n_block_units, first_blocks) of a launch of n_units units (rt_debug_hand_out; host only)."""
    nbu, fb = ctypes.c_uint32(0), ctypes.c_uint32(0)
    check(load_library().rt_debug_hand_out(n_units, reserve, grid_waves, ctypes.byref(nbu), ctypes.byref(fb)))
    return nbu.value, fb.value


def sample_map_plan(counts, quantum: int = 0) -> dict:
    """The plan of a host table of per-tile sample counts (rt_sample_map_plan; host only, no GPU
    needed): {order, levels, level_tiles, quantised} as uint32 arrays. Launch j of a sample-map frame
    renders samples [levels[j-1], levels[j]) on the tiles order[:level_tiles[j]]. Raises RtError for
    what the library refuses (a count above 2^19, more than 64 levels)."""
    c = np.ascontiguousarray(np.asarray(counts).reshape(-1), np.uint32)
    n = len(c)
    order, quantised = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    levels = np.zeros(abi.SAMPLE_MAP_MAX_LEVELS, np.uint32)
    level_tiles = np.zeros(abi.SAMPLE_MAP_MAX_LEVELS, np.uint32)
    j = ctypes.c_uint32(0)
    check(load_library().rt_sample_map_plan(c.ctypes.data if n else None, n, quantum, order.ctypes.data if n else None,
                                            levels.ctypes.data, level_tiles.ctypes.data, ctypes.byref(j),
                                            quantised.ctypes.data if n else None))
    return {"order": order, "levels": levels[:j.value].copy(), "level_tiles": level_tiles[:j.value].copy(),
            "quantised": quantised}


def sample_map_info(counts, width: int, height: int, quantum: int = 0) -> abi.SampleMapInfo:
    """The SampleMapInfo a set call reports for the host table `counts` over a width x height band
    (rt_debug_sample_map_info; host only)."""
    c = np.ascontiguousarray(np.asarray(counts).reshape(-1), np.uint32)
    if len(c) != ((width + 7) // 8) * ((height + 7) // 8):
        raise ValueError("one count per 8x8 tile of the band")
    info = abi.SampleMapInfo()
    check(load_library().rt_debug_sample_map_info(c.ctypes.data, width, height, quantum, ctypes.byref(info)))
    return info


class MultiRenderer:
    """One process driving `gpu_count` GPUs (rt_multi): one context + stream per device and one
    RCCL communicator over them. A frame tiles the image into row-exact interleaved strips
    (partition_strips), re-dealt between frames from the devices' measured kernel times, and
    gathers every device's rows to device 0 over xGMI (grouped ncclSend / ncclRecv), where they
    are reordered; the image equals the one-GPU image bit for bit.

    logical=True (tests on a one-GPU box): `gpu_count` logical devices on GPU 0 running the same
    frame plans, each RCCL send / receive pair a device copy (rt_debug_multi_create_logical), or
    with logical="rccl" RCCL send / receive of a one-rank communicator to itself
    (rt_debug_multi_create_logical_rccl)."""

    def __init__(self, gpu_count: int = 1, logical=False):
        self._lib = load_library()
        self._m = ctypes.c_void_p()
        create = (self._lib.rt_debug_multi_create_logical_rccl if logical == "rccl"
                  else self._lib.rt_debug_multi_create_logical if logical else self._lib.rt_multi_create)
        check(create(gpu_count, ctypes.byref(self._m)))
        n = ctypes.c_uint32()
        check(self._lib.rt_multi_device_count(self._m, ctypes.byref(n)))
        self.device_count = n.value

    def close(self) -> None:
        if self._m:
            self._lib.rt_multi_destroy(self._m)
            self._m = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_scene(self, spheres) -> None:
        buf = spheres if not isinstance(spheres, np.ndarray) else np.ascontiguousarray(spheres, np.uint8)
        ptr = ctypes.addressof(buf) if not isinstance(buf, np.ndarray) else buf.ctypes.data
        check(self._lib.rt_multi_set_scene(self._m, ptr if len(spheres) else None, len(spheres)))

    def render(self, rci: RenderCallInfo, accum, out, options: Optional[Options] = None, stream=None) -> None:
        """One frame into device-0 tensors accum (float32 [H, W, 4]) and out (uint8 [H, W, 4])."""
        W, H = rci.image_size.x, rci.image_size.y
        _check_dev_tensor(accum, "torch.float32", (H, W, 4))
        _check_dev_tensor(out, "torch.uint8", (H, W, 4))
        if accum.device.index != 0 or out.device.index != 0:
            raise ValueError("MultiRenderer.render gathers to device 0: accum and out must live on cuda:0")
        check(self._lib.rt_multi_render(self._m, ctypes.byref(rci),
                                        ctypes.byref(options) if options is not None else None,
                                        accum.data_ptr(), out.data_ptr(), _stream_ptr(stream, 0)))

    def render_adaptive(self, rci: RenderCallInfo, accum, out, sample_count=None,
                        options: Optional[Options] = None, adaptive: Optional[Adaptive] = None,
                        stream=None) -> AdaptiveInfo:
        """One adaptive frame over the devices (rt_multi_render_adaptive) into device-0 tensors accum
        (float32 [H, W, 4]), out (uint8 [H, W, 4]) and the optional sample_count (4-byte integer
        [H, W]); `adaptive` from make_adaptive(), rci.samplesPerRenderCall the cap, options with
        rng_mode HASH. Equals Renderer.render_adaptive on the whole image bit for bit. Blocks the
        host on the per-pass readbacks only; the outputs are valid once `stream` completes. Returns
        the frame's totals."""
        if adaptive is None:
            raise ValueError("adaptive is required (make_adaptive)")
        W, H = rci.image_size.x, rci.image_size.y
        _check_dev_tensor(accum, "torch.float32", (H, W, 4))
        _check_dev_tensor(out, "torch.uint8", (H, W, 4))
        if accum.device.index != 0 or out.device.index != 0:
            raise ValueError("MultiRenderer.render_adaptive gathers to device 0: accum and out must live on cuda:0")
        count_ptr = None
        if sample_count is not None:
            if not sample_count.is_cuda or sample_count.element_size() != 4 or sample_count.is_floating_point() \
                    or not sample_count.is_contiguous() or tuple(sample_count.shape) != (H, W):
                raise ValueError("sample_count must be a contiguous 4-byte integer cuda tensor [H, W]")
            if sample_count.device.index != 0:
                raise ValueError("MultiRenderer.render_adaptive: sample_count must live on cuda:0")
            count_ptr = sample_count.data_ptr()
        info = AdaptiveInfo()
        check(self._lib.rt_multi_render_adaptive(self._m, ctypes.byref(rci),
                                                 ctypes.byref(options) if options is not None else None,
                                                 ctypes.byref(adaptive), accum.data_ptr(), out.data_ptr(), count_ptr,
                                                 ctypes.byref(info), _stream_ptr(stream, 0)))
        return info

    def adaptive_device_info(self, device: int) -> AdaptiveInfo:
        """The last adaptive frame's numbers of one device (rt_multi_adaptive_device_info): the
        imbalance of the static tile-row deal; zeros for a device that rendered nothing."""
        info = AdaptiveInfo()
        check(self._lib.rt_multi_adaptive_device_info(self._m, device, ctypes.byref(info)))
        return info

    def info(self) -> dict:
        """{devices, rccl_ranks (ncclCommCount of the communicator), strip_rows, launches of the
        last frame} (rt_multi_info)."""
        v = (ctypes.c_uint32 * 4)()
        check(self._lib.rt_multi_info(self._m, v))
        return {"devices": int(v[0]), "rccl_ranks": int(v[1]), "strip_rows": int(v[2]), "launches": int(v[3])}

    def kernel_times(self, frames: Optional[int] = None) -> list:
        """Trace-kernel ms of the last frame on each device that rendered rows (device order); with
        `frames`, a list of such lists for each of the last `frames` frames, oldest first."""
        if frames is None:
            buf = (ctypes.c_float * max(1, self.device_count))()
            got = ctypes.c_uint32(0)
            check(self._lib.rt_multi_kernel_times(self._m, buf, self.device_count, ctypes.byref(got)))
            return [float(buf[i]) for i in range(got.value)]
        cap = frames * self.device_count
        buf = (ctypes.c_float * max(1, cap))()
        got = ctypes.c_uint32(0)
        check(self._lib.rt_multi_kernel_times_frames(self._m, frames, buf, cap, ctypes.byref(got)))
        n = got.value // max(1, frames)
        return [[float(buf[f * n + d]) for d in range(n)] for f in range(frames)]

    def stats(self) -> Stats:
        st = Stats()
        check(self._lib.rt_multi_stats(self._m, ctypes.byref(st)))
        return st

    def partition(self, height: int) -> list:
        """The rows each device renders in the next frame (band order), one uint32 array per
        device (rt_multi_partition)."""
        counts = np.zeros(self.device_count, np.uint32)
        rows = np.zeros(max(1, height), np.uint32)
        check(self._lib.rt_multi_partition(self._m, rows.ctypes.data, counts.ctypes.data, height))
        return _split(rows, counts)

    def tune(self, **kv) -> None:
        """Balancer settings (rt_debug_multi_tune): balance=0/1, tolerance, blend in (0, 1], lag 1-8;
        None restores a default."""
        for k, v in kv.items():
            check(self._lib.rt_debug_multi_tune(self._m, k.encode(), -1.0 if v is None else float(v)))

    def feedback(self, device_ms: Sequence[float]) -> None:
        """Device times the next frame re-deals from, as if measured (rt_debug_multi_feedback)."""
        buf = (ctypes.c_float * max(1, len(device_ms)))(*device_ms)
        check(self._lib.rt_debug_multi_feedback(self._m, buf, len(device_ms)))

    def balance_info(self) -> dict:
        v = (ctypes.c_double * 4)()
        check(self._lib.rt_debug_multi_balance_info(self._m, v))
        return {"frames": int(v[0]), "rebalances": int(v[1]), "rows_moved": int(v[2]),
                "predicted_imbalance": float(v[3])}


def _split(rows: np.ndarray, counts: np.ndarray) -> list:
    out, at = [], 0
    for c in counts:
        out.append(rows[at:at + int(c)].copy())
        at += int(c)
    return out


def _flat(parts: Sequence) -> tuple:
    counts = np.asarray([len(p) for p in parts], np.uint32)
    rows = np.ascontiguousarray(np.concatenate([np.asarray(p, np.uint32) for p in parts])
                                if len(parts) else np.zeros(0, np.uint32), np.uint32)
    return rows, counts


def partition_strips(n_devices: int, height: int) -> list:
    """The row-exact interleaved strips every multi-device frame starts from (rt_partition_strips):
    one uint32 array of global rows per device, band order."""
    counts = np.zeros(n_devices, np.uint32)
    rows = np.zeros(max(1, height), np.uint32)
    check(load_library().rt_partition_strips(n_devices, height, rows.ctypes.data, counts.ctypes.data))
    return _split(rows, counts)


def partition_tile_rows(n_devices: int, height: int) -> list:
    """The static partition of adaptive multi-device frames (rt_partition_tile_rows): whole 8-row
    tile rows dealt round robin, one uint32 array of global rows per device (empty beyond the tile
    rows), band order."""
    counts = np.zeros(max(1, n_devices), np.uint32)
    rows = np.zeros(max(1, height), np.uint32)
    check(load_library().rt_partition_tile_rows(n_devices, height, rows.ctypes.data, counts.ctypes.data))
    return _split(rows, counts[:n_devices])


def partition_rebalance(parts: Sequence, cost: np.ndarray, measured: Optional[Sequence] = None,
                        device_ms: Optional[Sequence[float]] = None, tolerance: float = 0.001) -> tuple:
    """One balancing step (rt_partition_rebalance): rescale the per-row costs `cost` (float64 [H],
    <= 0 unknown; updated in place) to the device times `device_ms` measured on partition
    `measured`, then re-deal `parts`. Returns (new parts, rows moved, predicted max / mean)."""
    lib = load_library()
    n, H = len(parts), int(cost.shape[0])
    if cost.dtype != np.float64 or not cost.flags.c_contiguous:
        raise ValueError("cost must be a contiguous float64 array")
    rows, counts = _flat(parts)
    if len(rows) != H:
        raise ValueError("the partition must hold every row exactly once")
    m_rows = m_counts = m_ms = None
    keep = []
    if measured is not None:
        mr, mc = _flat(measured)
        ms = np.ascontiguousarray(np.asarray(device_ms, np.float32))
        if len(ms) != n or len(mc) != n:
            raise ValueError("one measured time per device")
        keep = [mr, mc, ms]
        m_rows, m_counts, m_ms = mr.ctypes.data, mc.ctypes.data, ms.ctypes.data
    moved = ctypes.c_uint32(0)
    pred = ctypes.c_double(1.0)
    check(lib.rt_partition_rebalance(n, H, rows.ctypes.data, counts.ctypes.data, cost.ctypes.data, m_rows, m_counts,
                                     m_ms, float(tolerance), ctypes.byref(moved), ctypes.byref(pred)))
    del keep
    return _split(rows, counts), int(moved.value), float(pred.value)


def launch_inputs(**kv) -> abi.LaunchInputs:
    """An abi.LaunchInputs (rt::launch::Inputs, csrc/rt_launch.h) with its header filled and every
    tuning value unset; fields by keyword (grid_n / grid_cs: sequences of 3; occ: rows of (accel,
    flags, lds_lo, lds_hi, blocks); tuning values as tune_<key>)."""
    v = abi.LaunchInputs()
    v.version, v.bytes = abi.LAUNCH_PLAN_VERSION, ctypes.sizeof(abi.LaunchInputs)
    for k in abi.TUNING_KEYS:
        setattr(v, "tune_" + k, -1.0)
    for k, x in kv.items():
        if k in ("grid_n", "grid_cs"):
            for i in range(3):
                getattr(v, k)[i] = x[i]
        elif k == "occ":
            v.n_occ = len(x)
            for i, row in enumerate(x):
                v.occ[i] = abi.LaunchOccRow(*row)
        else:
            if not hasattr(v, k):
                raise KeyError(k)
            setattr(v, k, x)
    return v


def launch_plan(inputs: abi.LaunchInputs) -> abi.LaunchPlan:
    """The launch plan rt_render_device computes from `inputs` (rt_debug_launch_plan without a
    context; host only, no GPU needed). Raises RtError for what the library refuses ("band too
    large", an occupancy the table in the inputs does not answer, values outside the domain)."""
    plan = abi.LaunchPlan()
    check(load_library().rt_debug_launch_plan(None, ctypes.byref(inputs), ctypes.sizeof(inputs), ctypes.byref(plan),
                                              ctypes.sizeof(plan)))
    return plan


CAMERA_BATCH_REASONS = ("on", "tune", "stream", "table", "count", "form", "pinhole", "depth", "lds", "occupancy")


def camera_batches(inputs: abi.LaunchInputs, tune: float = -1.0, max_depth: int = 0, table: bool = False,
                   kernel_blocks: int = -1) -> dict:
    """Whether rt_render_device runs the camera-batch form for the launch launch_plan(inputs) plans
    (rt_debug_camera_batches; host only): {"on", "why" (CAMERA_BATCH_REASONS), "static_lds",
    "lds_total"}."""
    out = (ctypes.c_uint32 * 3)()
    check(load_library().rt_debug_camera_batches(ctypes.byref(inputs), ctypes.sizeof(inputs), float(tune), int(max_depth),
                                                 1 if table else 0, int(kernel_blocks), out))
    return {"on": out[0] == 0, "why": CAMERA_BATCH_REASONS[out[0]], "static_lds": int(out[1]), "lds_total": int(out[2])}


def row_weights(cost, order, tiles_x: int, band_h: int, head_tiles: int = 0, head_chunks: int = 1,
                chunks: int = 1) -> np.ndarray:
    """Per band row, its share of a launch's work from the tile-cost record `cost` (row-major tiles,
    tiles_x per tile row) and the hand-out `order` (None: none kept): what rt_launch_row_weights
    computes for a recorded launch (rt_debug_row_weights; host only)."""
    c = np.ascontiguousarray(cost, np.uint32)
    o = None if order is None else np.ascontiguousarray(order, np.uint32)
    if o is not None and len(o) != len(c):
        raise ValueError("order and cost must be equally long")
    w = np.zeros(band_h, np.float64)
    check(load_library().rt_debug_row_weights(c.ctypes.data if len(c) else None, None if o is None else o.ctypes.data,
                                              len(c), tiles_x, band_h, head_tiles, head_chunks, chunks,
                                              w.ctypes.data if band_h else None))
    return w


def struct_dict(s: ctypes.Structure) -> dict:
    """A ctypes struct of words, doubles and arrays of them as a plain dict (nested lists)."""
    def val(x):
        if isinstance(x, ctypes.Array):
            return [val(e) for e in x]
        if isinstance(x, ctypes.Structure):
            return [val(getattr(x, n)) for n, _ in x._fields_]
        return x
    return {n: val(getattr(s, n)) for n, _ in s._fields_}


PLAN_OPS = {1: "load_rows", 2: "group_start", 3: "send", 4: "recv", 5: "group_end", 6: "render",
            7: "store_rows", 8: "resolve", 9: "render_adaptive", 10: "send_counts", 11: "recv_counts",
            12: "store_tiles"}


def multi_plan(n_devices: int, width: int, height: int, band_starts: Optional[Sequence[int]] = None,
               accumulate: bool = False, parts: Optional[Sequence] = None) -> dict:
    """The frame plan rt_multi executes (rt_debug_multi_plan; host only, no GPU needed): the parts
    [(device, whole, rows)] and the ordered steps [{op, dev, peer, part, flags, count}]. band_starts
    None: the row-exact strips (rt_multi_render's first frame); else the bands of rt_render; parts:
    an explicit partition (one row array per device, e.g. a re-dealt one; rt_debug_multi_plan_rows)."""
    lib = load_library()
    n = ctypes.c_uint64(0)
    if parts is not None:
        rows, counts = _flat(parts)
        if len(counts) != n_devices:
            raise ValueError("one row array per device")
        call = lambda out, cap: lib.rt_debug_multi_plan_rows(n_devices, width, height, rows.ctypes.data,  # noqa: E731
                                                              counts.ctypes.data, int(accumulate), out, cap,
                                                              ctypes.byref(n))
    else:
        bs = None if band_starts is None else (ctypes.c_uint32 * len(band_starts))(*band_starts)
        nb = 0 if band_starts is None else len(band_starts)
        call = lambda out, cap: lib.rt_debug_multi_plan(n_devices, width, height, bs, nb, int(accumulate),  # noqa: E731
                                                         out, cap, ctypes.byref(n))
    return _read_plan(call, n)


def multi_plan_adaptive(n_devices: int, width: int, height: int) -> dict:
    """The plan of an adaptive frame (rt_debug_multi_plan_adaptive; host only): multi_plan's form
    over partition_tile_rows' parts, with the ops render_adaptive, send_counts / recv_counts and
    store_tiles."""
    lib = load_library()
    n = ctypes.c_uint64(0)
    return _read_plan(lambda out, cap: lib.rt_debug_multi_plan_adaptive(n_devices, width, height, out, cap,
                                                                       ctypes.byref(n)), n)


def _read_plan(call, n) -> dict:
    check(call(None, 0))
    buf = np.zeros(n.value, np.uint32)
    check(call(buf.ctypes.data, n.value))
    n_parts, n_steps = int(buf[0]), int(buf[1])
    at, parts, steps = 2, [], []
    for _ in range(n_parts):
        dev, whole, nr = (int(v) for v in buf[at:at + 3])
        parts.append((dev, bool(whole), buf[at + 3:at + 3 + nr].copy()))
        at += 3 + nr
    for _ in range(n_steps):
        op, dev, peer, part, flags, lo, hi = (int(v) for v in buf[at:at + 7])
        steps.append({"op": PLAN_OPS.get(op, op), "dev": dev, "peer": peer, "part": part, "flags": flags,
                      "count": lo | (hi << 32)})
        at += 7
    assert at == len(buf)
    return {"parts": parts, "steps": steps}


@dataclass
class RenderResult:
    accum: np.ndarray   # float32 [H, W, 4] — the rgba32f sum image (binding 3)
    rgba8: np.ndarray   # uint8   [H, W, 4] — the tonemapped image (binding 0)
    stats: Stats


def render(spheres, rci: RenderCallInfo | Sequence[RenderCallInfo], options: Optional[Options] = None,
           accum: Optional[np.ndarray] = None) -> RenderResult:
    """Host-buffer frame (rt_render): one band per RenderCallInfo, band i on device i % ndev."""
    lib = load_library()
    rcis = [rci] if isinstance(rci, RenderCallInfo) else list(rci)
    arr = (RenderCallInfo * len(rcis))(*rcis)
    W, H = rcis[0].image_size.x, rcis[0].image_size.y
    acc = np.zeros((H, W, 4), np.float32) if accum is None else np.ascontiguousarray(accum, np.float32)
    out = np.zeros((H, W, 4), np.uint8)
    st = Stats()
    sp = spheres if not isinstance(spheres, np.ndarray) else np.ascontiguousarray(spheres, np.uint8)
    sptr = ctypes.addressof(sp) if not isinstance(sp, np.ndarray) else sp.ctypes.data
    check(lib.rt_render(sptr, len(spheres), ctypes.addressof(arr), len(rcis), acc.ctypes.data,
                        out.ctypes.data, ctypes.byref(options) if options is not None else None,
                        ctypes.byref(st)))
    return RenderResult(acc, out, st)


def store_ppm(path: str, rgba8: np.ndarray) -> None:
    h, w = rgba8.shape[:2]
    img = np.ascontiguousarray(rgba8, np.uint8)
    check(load_library().rt_store_ppm(str(path).encode(), img.ctypes.data, w, h))


def ray_trace(samples: int = 10, storeRenderResult: bool = False, width: int = 1920,
              height: int = 1080, gpu_count: int = 1) -> None:
    """src/ray_trace.h:9-15, same parameters and defaults (the C symbol, called through ctypes)."""
    load_library().ray_trace(samples, storeRenderResult, width, height, gpu_count)
