"""ctypes binding of libwgt.so — the C-ABI declared in include/wgt_api.h.

The product has no CPU fallback: if libwgt.so is missing, loading fails loudly;
if no HIP device is present, wgt_create returns an error.  Build with
`python -c "import __graft_entry__ as g; g.build()"` or `make -C webgputracer_amd`.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WGT_LIB_PATH") or os.path.join(PKG_DIR, "libwgt.so")  # override: A/B runs

# Byte layouts of include/wgt_api.h (= the reference GPU buffers)
QUAD_DTYPE = np.dtype([("pos", "<f4", 4), ("right", "<f4", 4), ("up", "<f4", 4), ("norm", "<f4", 4),
                       ("w", "<f4", 3), ("d", "<f4"), ("col", "<f4", 3), ("emissive", "<f4")])
SPHERE_DTYPE = np.dtype([("center", "<f4", 3), ("radius", "<f4"), ("col", "<f4", 3), ("emissive", "<f4")])
TRI_DTYPE = np.dtype([("v0", "<f4", 4), ("e1", "<f4", 4), ("e2", "<f4", 4), ("face_norm", "<f4", 4),
                      ("col", "<f4", 3), ("emissive", "<f4")])
CAMERA_DTYPE = np.dtype([("origin", "<f4", 3), ("pad0", "<f4"), ("target", "<f4", 3), ("pad1", "<f4"),
                         ("aspect", "<f4"), ("fovy", "<f4"), ("spp", "<u4"), ("seed", "<u4")])
TILE_DTYPE = np.dtype([("x0", "<u4"), ("y0", "<u4"), ("seed", "<u4"), ("frame", "<u4")])
assert QUAD_DTYPE.itemsize == 96 and SPHERE_DTYPE.itemsize == 32
assert TRI_DTYPE.itemsize == 80 and CAMERA_DTYPE.itemsize == 48 and TILE_DTYPE.itemsize == 16

API_VERSION = 2  # WGT_API_VERSION of include/wgt_api.h
WGT_OK, WGT_E_INVALID, WGT_E_HIP, WGT_E_NOSCENE, WGT_E_IO, WGT_E_NOMEM = 0, -1, -2, -3, -4, -5
NO_HIT = 0xFFFFFFFF
WGT_HIT_EMISSIVE, WGT_HIT_FRONT_FACE = 1, 2  # wgt_hit_buffers.flags
HIT_FIELDS = ("prim", "dist", "pos", "norm", "col", "flags")


class WgtHitBuffers(ctypes.Structure):
    """wgt_hit_buffers: planar outputs of the hit-record calls (None / 0 = field not written)."""
    _fields_ = [(k, ctypes.c_void_p) for k in HIT_FIELDS]


NEAREST_FIELDS = ("prim", "dist", "pos", "uv")


class WgtNearestBuffers(ctypes.Structure):
    """wgt_nearest_buffers (32 bytes): planar outputs of the closest-point queries (None / 0 = not written)."""
    _fields_ = [(k, ctypes.c_void_p) for k in NEAREST_FIELDS]


NEAREST_K_FIELDS = ("count", "prim", "dist", "pos", "uv")
WGT_NEAREST_MAX_K = 32


class WgtNearestKBuffers(ctypes.Structure):
    """wgt_nearest_k_buffers (40 bytes): planar outputs of the k-nearest closest-point queries (None / 0 = not
    written)."""
    _fields_ = [(k, ctypes.c_void_p) for k in NEAREST_K_FIELDS]


OVERLAP_FIELDS = ("hit", "count", "prim")
WGT_OVERLAP_MAX_K = 32


class WgtOverlapBuffers(ctypes.Structure):
    """wgt_overlap_buffers (24 bytes): planar outputs of the triangle overlap queries (None / 0 = not written)."""
    _fields_ = [(k, ctypes.c_void_p) for k in OVERLAP_FIELDS]


RADIANCE_FIELDS = ("rgb", "prim", "seed")  # the Python names; the struct's third field is seed_out


class WgtRadianceBuffers(ctypes.Structure):
    """wgt_radiance_buffers (24 bytes): planar outputs of the radiance queries (None / 0 = not written)."""
    _fields_ = [(k, ctypes.c_void_p) for k in ("rgb", "prim", "seed_out")]


MULTI_HIT_FIELDS = ("count", "prim", "dist")
WGT_MULTI_HIT_TRIS_ONLY = 1  # wgt_trace_multi_hits' flags
WGT_MULTI_HIT_MAX_K = 32


class WgtMultiHitBuffers(ctypes.Structure):
    """wgt_multi_hit_buffers (24 bytes): outputs of the multi-hit queries (None / 0 = not written)."""
    _fields_ = [(k, ctypes.c_void_p) for k in MULTI_HIT_FIELDS]


WGT_DENOISE_DEMODULATE = 1  # wgt_denoise_params.flags


class WgtDenoiseParams(ctypes.Structure):
    """wgt_denoise_params (16 bytes); wgt_denoise_defaults fills the defaults."""
    _fields_ = [("iterations", ctypes.c_uint32), ("normal_power", ctypes.c_uint32), ("sigma_pos", ctypes.c_float),
                ("flags", ctypes.c_uint32)]


class WgtDenoiseVarianceParams(ctypes.Structure):
    """wgt_denoise_variance_params (24 bytes); wgt_denoise_variance_defaults fills the defaults."""
    _fields_ = [("iterations", ctypes.c_uint32), ("normal_power", ctypes.c_uint32), ("sigma_pos", ctypes.c_float),
                ("flags", ctypes.c_uint32), ("sigma_lum", ctypes.c_float), ("min_history", ctypes.c_uint32)]


WGT_TEMPORAL_MATCH_PRIM = 1  # wgt_temporal_params.flags


class WgtTemporalParams(ctypes.Structure):
    """wgt_temporal_params (16 bytes); wgt_temporal_defaults fills the defaults."""
    _fields_ = [("max_history", ctypes.c_uint32), ("normal_min", ctypes.c_float), ("plane_tol", ctypes.c_float),
                ("flags", ctypes.c_uint32)]


class WgtTemporalState(ctypes.Structure):
    """wgt_temporal_state (24 bytes): the history the caller owns (None / 0 = NULL)."""
    _fields_ = [("rgba32f", ctypes.c_void_p), ("len", ctypes.c_void_p), ("moments", ctypes.c_void_p)]


class WgtMotionBuffers(ctypes.Structure):
    """wgt_motion_buffers (16 bytes): where each hit lay before the update, 3 planes of n floats each."""
    _fields_ = [("pos_prev", ctypes.c_void_p), ("norm_prev", ctypes.c_void_p)]


class WgtSamplePlanParams(ctypes.Structure):
    """wgt_sample_plan_params (28 bytes); wgt_sample_plan_defaults fills the defaults."""
    _fields_ = [("side_min", ctypes.c_uint32), ("side_max", ctypes.c_uint32), ("gain", ctypes.c_float),
                ("lum_floor", ctypes.c_float), ("min_history", ctypes.c_uint32), ("dilate", ctypes.c_uint32),
                ("budget_spp", ctypes.c_float)]


class WgtStats(ctypes.Structure):
    _fields_ = [("queries", ctypes.c_uint64), ("traced_rays", ctypes.c_uint64), ("samples", ctypes.c_uint64),
                ("nan_rays", ctypes.c_uint64), ("node_visits", ctypes.c_uint64), ("tri_tests", ctypes.c_uint64),
                ("pixels", ctypes.c_uint64), ("loop_wave_iters", ctypes.c_uint64),
                ("loop_lane_iters", ctypes.c_uint64), ("trav_wave_steps", ctypes.c_uint64),
                ("trav_lane_steps", ctypes.c_uint64), ("cyc_service", ctypes.c_uint64),
                ("cyc_trav", ctypes.c_uint64), ("kernel_ms", ctypes.c_float),
                ("trace_ms", ctypes.c_float), ("shade_ms", ctypes.c_float), ("iterations", ctypes.c_uint32),
                ("cyc_refill", ctypes.c_uint64), ("cyc_finalise", ctypes.c_uint64),
                ("cyc_shade", ctypes.c_uint64), ("cyc_camera", ctypes.c_uint64), ("cyc_quads", ctypes.c_uint64),
                ("cyc_root", ctypes.c_uint64), ("stack_spills", ctypes.c_uint64),
                ("stack_refills", ctypes.c_uint64), ("stack_overflows", ctypes.c_uint64),
                ("top_node_visits", ctypes.c_uint64), ("cyc_node_steps", ctypes.c_uint64),
                ("cyc_top_steps", ctypes.c_uint64), ("cyc_tri_steps", ctypes.c_uint64),
                ("quad_ref_scans", ctypes.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class WgtSceneInfo(ctypes.Structure):
    _fields_ = [("n_lights", ctypes.c_uint32), ("n_quads", ctypes.c_uint32), ("n_spheres", ctypes.c_uint32),
                ("n_tris", ctypes.c_uint32), ("bvh_nodes", ctypes.c_uint32), ("bvh_leaves", ctypes.c_uint32),
                ("bvh_max_depth", ctypes.c_uint32), ("bvh_max_leaf", ctypes.c_uint32),
                ("device_bytes", ctypes.c_uint64), ("sah_cost", ctypes.c_double), ("bvh_width", ctypes.c_uint32),
                ("bvh_stack", ctypes.c_uint32), ("bvh2_nodes", ctypes.c_uint32), ("bvh2_depth", ctypes.c_uint32),
                ("bvh_compact", ctypes.c_uint32), ("bvh_compact_step", ctypes.c_float), ("ps_waves", ctypes.c_uint32),
                ("ps_park", ctypes.c_uint32), ("ps_stack", ctypes.c_uint32), ("node_form", ctypes.c_uint32),
                ("ps_resident", ctypes.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class WgtOrderStats(ctypes.Structure):
    """wgt_order_stats (40 bytes): how the persistent kernel's launches got their queue order."""
    _fields_ = [("today", ctypes.c_uint64), ("refine", ctypes.c_uint64), ("reuse", ctypes.c_uint64),
                ("invalidations", ctypes.c_uint64), ("nb", ctypes.c_uint32), ("refine_side", ctypes.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


# Every symbol include/wgt_api.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "wgt_create", "wgt_destroy", "wgt_last_error", "wgt_version", "wgt_build_id", "wgt_device_count",
    "wgt_upload_scene", "wgt_scene_info_get", "wgt_render_tile", "wgt_render_tiles_async",
    "wgt_render_tiles_stats", "wgt_render_tiles_profile", "wgt_trace_rays", "wgt_trace_rays_async",
    "wgt_occluded_rays", "wgt_occluded_rays_async", "wgt_trace_hits", "wgt_trace_hits_async",
    "wgt_render_gbuffer", "wgt_render_gbuffer_async", "wgt_sync", "wgt_selftest_math", "wgt_stream",
    "wgt_pipeline_stream",
    "wgt_scene_cornell", "wgt_make_triangles", "wgt_load_obj", "wgt_procedural_mesh",
    "wgt_write_obj", "wgt_write_png", "wgt_bvh_build", "wgt_bvh_build_compact",
    "wgt_render_frames",
    "wgt_update_triangles", "wgt_update_timing", "wgt_bvh_read", "wgt_bvh_refit",
    "wgt_update_triangles_device", "wgt_update_vertices_device",
    "wgt_rebuild_triangles", "wgt_rebuild_triangles_device", "wgt_bvh_build_morton",
    "wgt_denoise_defaults", "wgt_denoise_workspace_bytes", "wgt_denoise", "wgt_denoise_async",
    "wgt_temporal_defaults", "wgt_temporal_accumulate", "wgt_temporal_accumulate_async",
    "wgt_denoise_variance_defaults", "wgt_denoise_variance_workspace_bytes", "wgt_denoise_variance",
    "wgt_denoise_variance_async",
    "wgt_motion_snapshot", "wgt_motion_snapshot_read", "wgt_motion_reproject", "wgt_motion_reproject_async",
    "wgt_temporal_accumulate_motion", "wgt_temporal_accumulate_motion_async",
    "wgt_render_tile_sampled", "wgt_render_tiles_sampled_async", "wgt_render_gbuffer_sampled",
    "wgt_render_gbuffer_sampled_async",
    "wgt_sample_plan_defaults", "wgt_sample_plan_workspace_bytes", "wgt_sample_plan", "wgt_sample_plan_async",
    "wgt_order_info", "wgt_order_read", "wgt_order_reset",
    "wgt_nearest_points", "wgt_nearest_points_async", "wgt_nearest_points_stats", "wgt_nearest_points_spec",
    "wgt_trace_radiance", "wgt_trace_radiance_async", "wgt_trace_radiance_stats",
    "wgt_trace_multi_hits", "wgt_trace_multi_hits_async", "wgt_trace_multi_hits_stats",
    "wgt_nearest_k_points", "wgt_nearest_k_points_async", "wgt_nearest_k_points_stats", "wgt_nearest_k_points_spec",
    "wgt_overlap_triangles", "wgt_overlap_triangles_async", "wgt_overlap_triangles_stats", "wgt_overlap_triangles_spec",
    "wgt_overlap_self", "wgt_overlap_self_async", "wgt_overlap_self_stats", "wgt_overlap_self_spec",
]

_lib = None


class WgtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"wgt error {code}: {msg}")
        self.code = code


def lib():
    """Load libwgt.so (raises if it was not built: there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built; run __graft_entry__.build() (no CPU fallback exists)")
    # One HIP runtime per process: torch ships its own libamdhip64.so.7.  Loaded
    # first, it is the one libwgt.so binds to (same SONAME), so device pointers and
    # streams from torch and from libwgt.so belong to one runtime; loaded after
    # libwgt.so's /opt/rocm copy, torch's would initialise a second runtime, which
    # fails ("No HIP GPUs are available").
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    P, U32, I = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    sig = {
        "wgt_create": (I, [I, ctypes.POINTER(P)]),
        "wgt_destroy": (None, [P]),
        "wgt_last_error": (ctypes.c_char_p, [P]),
        "wgt_version": (I, []),
        "wgt_build_id": (ctypes.c_char_p, []),
        "wgt_device_count": (I, [ctypes.POINTER(I)]),
        "wgt_upload_scene": (I, [P, P, U32, P, U32, P, U32, P, U32]),
        "wgt_scene_info_get": (I, [P, ctypes.POINTER(WgtSceneInfo)]),
        "wgt_render_tile": (I, [P, P, U32, U32, U32, U32, U32, U32, P, P, P, P]),
        "wgt_render_tiles_async": (I, [P, P, U32, U32, U32, U32, P, U32, P, P, P, P]),
        "wgt_render_tiles_stats": (I, [P, P, U32, U32, U32, U32, P, U32, P]),
        "wgt_render_tiles_profile": (I, [P, P, U32, U32, U32, U32, P, U32, P]),
        "wgt_trace_rays": (I, [P, P, U32, P, P]),
        "wgt_trace_rays_async": (I, [P, P, U32, P, P, P]),
        "wgt_occluded_rays": (I, [P, P, P, U32, P]),
        "wgt_occluded_rays_async": (I, [P, P, P, U32, P, P]),
        "wgt_trace_hits": (I, [P, P, U32, ctypes.POINTER(WgtHitBuffers)]),
        "wgt_trace_hits_async": (I, [P, P, U32, ctypes.POINTER(WgtHitBuffers), P]),
        "wgt_render_gbuffer": (I, [P, P, U32, U32, U32, U32, U32, U32, ctypes.POINTER(WgtHitBuffers), P]),
        "wgt_render_gbuffer_async": (I, [P, P, U32, U32, U32, U32, P, U32, ctypes.POINTER(WgtHitBuffers), P, P]),
        "wgt_sync": (I, [P]),
        "wgt_selftest_math": (I, [P, U32, U32, P]),
        "wgt_stream": (P, [P]),
        "wgt_pipeline_stream": (P, [P, U32]),
        "wgt_scene_cornell": (I, [P, ctypes.POINTER(U32), P, ctypes.POINTER(U32), P, ctypes.POINTER(U32)]),
        "wgt_make_triangles": (I, [P, U32, P, I, P, P]),
        "wgt_load_obj": (I, [ctypes.c_char_p, P, P, I, P, ctypes.POINTER(U32)]),
        "wgt_procedural_mesh": (I, [I, U32, U32, P, ctypes.POINTER(U32)]),
        "wgt_write_obj": (I, [ctypes.c_char_p, P, U32]),
        "wgt_write_png": (I, [ctypes.c_char_p, P, U32, U32]),
        "wgt_bvh_build": (I, [P, U32, P, U32, P, ctypes.POINTER(WgtSceneInfo)]),
        "wgt_render_frames": (I, [P, P, U32, U32, P, U32, P, P]),
        "wgt_update_triangles": (I, [P, P, U32]),
        "wgt_update_triangles_device": (I, [P, P, U32, P]),
        "wgt_update_vertices_device": (I, [P, P, U32, P, U32, P]),
        "wgt_update_timing": (I, [P, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]),
        "wgt_bvh_read": (I, [P, P, U32, P, P, P, ctypes.POINTER(ctypes.c_float)]),
        "wgt_bvh_refit": (I, [P, P, U32, P, U32, P, P, P, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(WgtSceneInfo)]),
        "wgt_rebuild_triangles": (I, [P, P, U32]),
        "wgt_rebuild_triangles_device": (I, [P, P, U32, P]),
        "wgt_bvh_build_morton": (I, [P, U32, P, U32, P, P, P, ctypes.POINTER(ctypes.c_float),
                                     ctypes.POINTER(WgtSceneInfo)]),
        "wgt_denoise_defaults": (I, [ctypes.POINTER(WgtDenoiseParams)]),
        "wgt_denoise_workspace_bytes": (ctypes.c_size_t, [U32, U32]),
        "wgt_denoise": (I, [P, ctypes.POINTER(WgtDenoiseParams), U32, U32, P, ctypes.POINTER(WgtHitBuffers), P, P]),
        "wgt_denoise_async": (I, [P, ctypes.POINTER(WgtDenoiseParams), U32, U32, P, ctypes.POINTER(WgtHitBuffers), P,
                                  ctypes.c_size_t, P, P, P]),
        "wgt_temporal_defaults": (I, [ctypes.POINTER(WgtTemporalParams)]),
        "wgt_temporal_accumulate": (I, [P, ctypes.POINTER(WgtTemporalParams), U32, U32, P, P, P,
                                        ctypes.POINTER(WgtHitBuffers), ctypes.POINTER(WgtTemporalState),
                                        ctypes.POINTER(WgtHitBuffers), ctypes.POINTER(WgtTemporalState), P]),
        "wgt_temporal_accumulate_async": (I, [P, ctypes.POINTER(WgtTemporalParams), U32, U32, P, P, P,
                                              ctypes.POINTER(WgtHitBuffers), ctypes.POINTER(WgtTemporalState),
                                              ctypes.POINTER(WgtHitBuffers), ctypes.POINTER(WgtTemporalState), P, P]),
        "wgt_denoise_variance_defaults": (I, [ctypes.POINTER(WgtDenoiseVarianceParams)]),
        "wgt_denoise_variance_workspace_bytes": (ctypes.c_size_t, [U32, U32]),
        "wgt_denoise_variance": (I, [P, ctypes.POINTER(WgtDenoiseVarianceParams), U32, U32,
                                     ctypes.POINTER(WgtTemporalState), ctypes.POINTER(WgtHitBuffers), P, P, P]),
        "wgt_denoise_variance_async": (I, [P, ctypes.POINTER(WgtDenoiseVarianceParams), U32, U32,
                                           ctypes.POINTER(WgtTemporalState), ctypes.POINTER(WgtHitBuffers), P,
                                           ctypes.c_size_t, P, P, P, P]),
        "wgt_motion_snapshot": (I, [P, P]),
        "wgt_motion_snapshot_read": (I, [P, P, U32]),
        "wgt_motion_reproject": (I, [P, U32, ctypes.POINTER(WgtHitBuffers), ctypes.POINTER(WgtMotionBuffers)]),
        "wgt_motion_reproject_async": (I, [P, U32, ctypes.POINTER(WgtHitBuffers), ctypes.POINTER(WgtMotionBuffers), P]),
        "wgt_temporal_accumulate_motion": (I, [P, ctypes.POINTER(WgtTemporalParams), U32, U32, P, P, P,
                                               ctypes.POINTER(WgtHitBuffers), ctypes.POINTER(WgtMotionBuffers),
                                               ctypes.POINTER(WgtTemporalState), ctypes.POINTER(WgtHitBuffers),
                                               ctypes.POINTER(WgtTemporalState), P]),
        "wgt_temporal_accumulate_motion_async": (I, [P, ctypes.POINTER(WgtTemporalParams), U32, U32, P, P, P,
                                                     ctypes.POINTER(WgtHitBuffers), ctypes.POINTER(WgtMotionBuffers),
                                                     ctypes.POINTER(WgtTemporalState), ctypes.POINTER(WgtHitBuffers),
                                                     ctypes.POINTER(WgtTemporalState), P, P]),
        "wgt_render_tile_sampled": (I, [P, P, U32, U32, U32, U32, U32, U32, P, P, P, P, P]),
        "wgt_render_tiles_sampled_async": (I, [P, P, U32, U32, U32, U32, P, U32, P, P, P, P, P]),
        "wgt_render_gbuffer_sampled": (I, [P, P, U32, U32, U32, U32, U32, U32, P, ctypes.POINTER(WgtHitBuffers), P]),
        "wgt_render_gbuffer_sampled_async": (I, [P, P, U32, U32, U32, U32, P, U32, P, ctypes.POINTER(WgtHitBuffers), P,
                                                 P]),
        "wgt_sample_plan_defaults": (I, [ctypes.POINTER(WgtSamplePlanParams)]),
        "wgt_sample_plan_workspace_bytes": (ctypes.c_size_t, [U32, U32]),
        "wgt_sample_plan": (I, [P, ctypes.POINTER(WgtSamplePlanParams), U32, U32, ctypes.POINTER(WgtTemporalState), P,
                                ctypes.POINTER(ctypes.c_uint64)]),
        "wgt_sample_plan_async": (I, [P, ctypes.POINTER(WgtSamplePlanParams), U32, U32,
                                      ctypes.POINTER(WgtTemporalState), P, ctypes.c_size_t, P, P, P]),
        "wgt_order_info": (I, [P, ctypes.POINTER(WgtOrderStats)]),
        "wgt_order_read": (I, [P, P, U32, ctypes.POINTER(U32)]),
        "wgt_order_reset": (I, [P]),
        "wgt_nearest_points": (I, [P, P, P, U32, ctypes.POINTER(WgtNearestBuffers)]),
        "wgt_nearest_points_async": (I, [P, P, P, U32, ctypes.POINTER(WgtNearestBuffers), P]),
        "wgt_nearest_points_stats": (I, [P, P, P, U32, ctypes.POINTER(WgtNearestBuffers),
                                         ctypes.POINTER(ctypes.c_uint64)]),
        "wgt_nearest_points_spec": (I, [P, U32, U32, P, P, U32, ctypes.POINTER(WgtNearestBuffers)]),
        "wgt_trace_radiance": (I, [P, P, P, U32, U32, U32, ctypes.POINTER(WgtRadianceBuffers)]),
        "wgt_trace_radiance_async": (I, [P, P, P, U32, U32, U32, ctypes.POINTER(WgtRadianceBuffers), P]),
        "wgt_trace_radiance_stats": (I, [P, P, P, U32, U32, U32, ctypes.POINTER(WgtRadianceBuffers),
                                         ctypes.POINTER(ctypes.c_uint64)]),
        "wgt_trace_multi_hits": (I, [P, P, P, U32, U32, U32, ctypes.POINTER(WgtMultiHitBuffers)]),
        "wgt_trace_multi_hits_async": (I, [P, P, P, U32, U32, U32, ctypes.POINTER(WgtMultiHitBuffers), P]),
        "wgt_trace_multi_hits_stats": (I, [P, P, P, U32, U32, U32, ctypes.POINTER(WgtMultiHitBuffers),
                                           ctypes.POINTER(ctypes.c_uint64)]),
        "wgt_nearest_k_points": (I, [P, P, P, U32, U32, ctypes.POINTER(WgtNearestKBuffers)]),
        "wgt_nearest_k_points_async": (I, [P, P, P, U32, U32, ctypes.POINTER(WgtNearestKBuffers), P]),
        "wgt_nearest_k_points_stats": (I, [P, P, P, U32, U32, ctypes.POINTER(WgtNearestKBuffers),
                                           ctypes.POINTER(ctypes.c_uint64)]),
        "wgt_nearest_k_points_spec": (I, [P, U32, U32, P, P, U32, U32, ctypes.POINTER(WgtNearestKBuffers)]),
        "wgt_overlap_triangles": (I, [P, P, U32, U32, ctypes.POINTER(WgtOverlapBuffers)]),
        "wgt_overlap_triangles_async": (I, [P, P, U32, U32, ctypes.POINTER(WgtOverlapBuffers), P]),
        "wgt_overlap_triangles_stats": (I, [P, P, U32, U32, ctypes.POINTER(WgtOverlapBuffers),
                                            ctypes.POINTER(ctypes.c_uint64)]),
        "wgt_overlap_triangles_spec": (I, [P, U32, U32, P, U32, U32, ctypes.POINTER(WgtOverlapBuffers)]),
        "wgt_overlap_self": (I, [P, P, U32, ctypes.POINTER(WgtOverlapBuffers)]),
        "wgt_overlap_self_async": (I, [P, P, U32, ctypes.POINTER(WgtOverlapBuffers), P]),
        "wgt_overlap_self_stats": (I, [P, P, U32, ctypes.POINTER(WgtOverlapBuffers), ctypes.POINTER(ctypes.c_uint64)]),
        "wgt_overlap_self_spec": (I, [P, U32, U32, P, U32, ctypes.POINTER(WgtOverlapBuffers)]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("WGT_LIB_PATH") and not hasattr(L, name):
            continue  # an older build loaded for same-box A/B timing
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    if L.wgt_version() != API_VERSION:  # the structs above mirror this version of include/wgt_api.h
        raise ImportError(f"{LIB_PATH}: ABI version {L.wgt_version()}, this wrapper mirrors {API_VERSION}")
    _lib = L
    return L


def ptr(a):
    """Host numpy array -> void* (None passes NULL)."""
    if a is None:
        return None
    return a.ctypes.data_as(ctypes.c_void_p)


def check(rc, ctx=None):
    if rc != WGT_OK:
        msg = lib().wgt_last_error(ctx)
        raise WgtError(rc, msg.decode() if msg else "")
    return rc
