"""webgputracer_amd — MI355X-native (gfx950) path-tracing hot path of kugimasa/WebGPUTracer.

The per-pixel path tracer of resources/shader/path_tracer.wgsl re-built as hand-written
HIP kernels behind a C-ABI (include/wgt_api.h, libwgt.so), with a BVH + Moller-Trumbore
triangle extension, tile sharding over GPUs and an RCCL gather (webgputracer_amd.dist).
"""
from .tracer import (WGT_HIT_EMISSIVE, WGT_HIT_FRONT_FACE, Context, build_id, bvh_build, bvh_build_compact, bvh_build_morton, bvh_refit, camera_param,
                     cornell_scene, denoise_defaults, denoise_variance_defaults, denoise_variance_workspace_bytes,
                     denoise_workspace_bytes, device_count, load_obj, make_triangles,
                     mesh_scene, nearest_k_points_spec, nearest_points_spec, overlap_self_spec, overlap_triangles_spec, procedural_mesh, sample_plan_defaults, sample_plan_workspace_bytes, temporal_defaults,
                     tile_grid, write_obj, write_png)

__all__ = ["WGT_HIT_EMISSIVE", "WGT_HIT_FRONT_FACE", "Context", "build_id", "bvh_build", "bvh_build_compact", "bvh_build_morton", "bvh_refit", "camera_param",
           "cornell_scene", "denoise_defaults", "denoise_variance_defaults", "denoise_variance_workspace_bytes",
           "denoise_workspace_bytes", "device_count", "load_obj", "make_triangles",
           "mesh_scene", "nearest_k_points_spec", "nearest_points_spec", "overlap_self_spec", "overlap_triangles_spec", "procedural_mesh", "sample_plan_defaults", "sample_plan_workspace_bytes", "temporal_defaults",
           "tile_grid", "write_obj", "write_png"]
