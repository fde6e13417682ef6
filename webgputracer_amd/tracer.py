"""Python face of the C-ABI (include/wgt_api.h), used by tests and bench.py.

Mirrors the reference's host objects for the path-tracing hot path:
  Scene::Scene (scene.cpp:14-36)            -> cornell_scene(), mesh_scene()
  Scene::LoadObj (scene.cpp:56-131)         -> load_obj()
  Camera::Update (camera.cpp:64-70)         -> camera_param()
  Renderer::InitDevice / OnRender dispatch  -> Context.render_tile / render_tiles_async
  sample_hit (path_tracer.wgsl:290-310)     -> Context.trace_rays, Context.occluded (dist < a limit)
  HitInfo (path_tracer.wgsl:27-36)          -> Context.trace_hits, Context.render_gbuffer (whole records)
  (none: the triangle nearest to a point)   -> Context.nearest_points, nearest_points_spec (host brute force)
  compute_sample's path loop (:386-393)     -> Context.trace_radiance (a path per caller ray and RNG state)
  (none: every surface along a ray)         -> Context.trace_multi_hits (k nearest hits, hit count), points_inside
  (none: the triangles around a point)      -> Context.nearest_k_points (k nearest, count within a radius), nearest_k_points_spec
  (none: the triangles a triangle cuts)     -> Context.overlap_triangles (whether, how many, which), overlap_triangles_spec
  (none: the triangles a mesh's own cut)    -> Context.overlap_self, self_intersections (neighbours by index excluded), overlap_self_spec
The C++ mirror (include/wgt/{scene,camera,renderer}.h) is the same API for C++ callers.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._lib import (CAMERA_DTYPE, HIT_FIELDS, MULTI_HIT_FIELDS, NEAREST_FIELDS, NEAREST_K_FIELDS, OVERLAP_FIELDS, RADIANCE_FIELDS, WGT_MULTI_HIT_TRIS_ONLY, WgtMultiHitBuffers, WgtNearestBuffers, WgtNearestKBuffers, WgtOverlapBuffers, WgtRadianceBuffers, QUAD_DTYPE, SPHERE_DTYPE, TILE_DTYPE, TRI_DTYPE, WgtDenoiseParams,
                   WgtDenoiseVarianceParams,
                   WgtHitBuffers, WgtMotionBuffers, WgtSamplePlanParams, WgtOrderStats, WgtSceneInfo, WgtStats, WgtTemporalParams, WgtTemporalState, WGT_E_HIP, WGT_HIT_EMISSIVE, WGT_HIT_FRONT_FACE, WgtError, check, lib, ptr)

COL_WHITE = np.array([0.73, 0.73, 0.73], np.float32)  # color_util.h:8
MESH_KINDS = {"bunny": (0, 69451), "sponza": (1, 262267)}


def cornell_scene():
    """The reference Cornell box (scene.cpp:14-36): (lights[1], quads[17], spheres[1])."""
    L = lib()
    lights, quads, spheres = np.zeros(4, QUAD_DTYPE), np.zeros(32, QUAD_DTYPE), np.zeros(4, SPHERE_DTYPE)
    nl, nq, ns = ctypes.c_uint32(4), ctypes.c_uint32(32), ctypes.c_uint32(4)
    check(L.wgt_scene_cornell(ptr(lights), ctypes.byref(nl), ptr(quads), ctypes.byref(nq), ptr(spheres),
                              ctypes.byref(ns)))
    return lights[:nl.value].copy(), quads[:nq.value].copy(), spheres[:ns.value].copy()


def make_triangles(verts, col=COL_WHITE, emissive=False, translation=(0.0, 0.0, 0.0)):
    """Triangle ctor (triangle.cpp:3-16) on verts (n, 3, 3) after Vertex::Translate."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 9)
    out = np.zeros(len(v), TRI_DTYPE)
    c = np.ascontiguousarray(col, np.float32).reshape(3)
    t = np.ascontiguousarray(translation, np.float32).reshape(3)
    check(lib().wgt_make_triangles(ptr(v), len(v), ptr(c), int(emissive), ptr(t), ptr(out)))
    return out


def load_obj(path, col=COL_WHITE, translation=(0.0, 0.0, 0.0), emissive=False):
    """Scene::LoadObj (scene.cpp:56-65) through the own OBJ reader."""
    L = lib()
    c = np.ascontiguousarray(col, np.float32).reshape(3)
    t = np.ascontiguousarray(translation, np.float32).reshape(3)
    n = ctypes.c_uint32(0)
    check(L.wgt_load_obj(str(path).encode(), ptr(c), ptr(t), int(emissive), None, ctypes.byref(n)))
    out = np.zeros(n.value, TRI_DTYPE)
    check(L.wgt_load_obj(str(path).encode(), ptr(c), ptr(t), int(emissive), ptr(out), ctypes.byref(n)))
    return out[:n.value]


def write_obj(path, tris):
    check(lib().wgt_write_obj(str(path).encode(), ptr(np.ascontiguousarray(tris)), len(tris)))


def write_png(path, rgba8):
    rgba8 = np.ascontiguousarray(rgba8, np.uint8)
    h, w = rgba8.shape[:2]
    check(lib().wgt_write_png(str(path).encode(), ptr(rgba8), w, h))


def procedural_mesh(kind: str, target_tris: int | None = None, seed: int = 1):
    """Deterministic stand-in for an absent asset (kind: 'bunny' | 'sponza')."""
    k, default = MESH_KINDS[kind]
    target = default if target_tris is None else int(target_tris)
    L = lib()
    n = ctypes.c_uint32(0)
    check(L.wgt_procedural_mesh(k, target, seed, None, ctypes.byref(n)))
    out = np.zeros(n.value, TRI_DTYPE)
    check(L.wgt_procedural_mesh(k, target, seed, ptr(out), ctypes.byref(n)))
    return out[:n.value]


def mesh_scene(kind: str, target_tris: int | None = None, seed: int = 1, obj_path: str | None = None):
    """Mesh configs (BASELINE configs 3-5): reference light + the 5 Cornell walls +
    the mesh (the two inner boxes removed) + the dummy sphere."""
    lights, quads, spheres = cornell_scene()
    tris = load_obj(obj_path) if obj_path else procedural_mesh(kind, target_tris, seed)
    return lights, quads[:5].copy(), spheres, tris


def bvh_build(tris):
    """Host-only BVH build (wgt_bvh_build): (info, nodes (n, 8, 4) f32, leaf-ordered tris (n, 4, 4) f32)."""
    tris = np.ascontiguousarray(tris, TRI_DTYPE)
    L = lib()
    info = WgtSceneInfo()
    check(L.wgt_bvh_build(ptr(tris), len(tris), None, 0, None, ctypes.byref(info)))
    nodes = np.zeros((info.bvh_nodes, 8, 4), np.float32)
    recs = np.zeros((len(tris), 4, 4), np.float32)
    check(L.wgt_bvh_build(ptr(tris), len(tris), ptr(nodes), info.bvh_nodes, ptr(recs), ctypes.byref(info)))
    return info.as_dict(), nodes, recs


def bvh_build_compact(tris):
    """Host-only compact form of the same tree (wgt_bvh_build_compact):
    (cnodes (n, 16) u32, crefs (n, 4) i32, step)."""
    tris = np.ascontiguousarray(tris, TRI_DTYPE)
    L = lib()
    info = WgtSceneInfo()
    check(L.wgt_bvh_build(ptr(tris), len(tris), None, 0, None, ctypes.byref(info)))
    cn = np.zeros((info.bvh_nodes, 16), np.uint32)
    cr = np.zeros((info.bvh_nodes, 4), np.int32)
    step = ctypes.c_float(0.0)
    check(L.wgt_bvh_build_compact(ptr(tris), len(tris), ptr(cn), ptr(cr), info.bvh_nodes, ctypes.byref(step)))
    return cn, cr, step.value


def _tree_arrays(n_nodes, n_tris):
    """Host arrays of a whole tree in the export layouts: nodes, leaf-ordered records, compact nodes, compact refs."""
    return (np.zeros((n_nodes, 8, 4), np.float32), np.zeros((n_tris, 4, 4), np.float32),
            np.zeros((n_nodes, 16), np.uint32), np.zeros((n_nodes, 4), np.int32))


def bvh_refit(built_from, now):
    """Host-only refit (wgt_bvh_refit): the tree an upload of `built_from` alone followed by
    Context.update_triangles(now) must hold, as (info, nodes (n, 8, 4) f32, leaf-ordered tris (n_tris, 4, 4)
    f32, cnodes (n, 16) u32, crefs (n, 4) i32, step): bvh_build's and bvh_build_compact's layouts."""
    a = np.ascontiguousarray(built_from, TRI_DTYPE)
    b = np.ascontiguousarray(now, TRI_DTYPE)
    if len(a) != len(b):
        raise ValueError(f"bvh_refit: {len(b)} triangles now, {len(a)} built from")
    L = lib()
    info = WgtSceneInfo()
    step = ctypes.c_float(0.0)
    check(L.wgt_bvh_refit(ptr(a), ptr(b), len(a), None, 0, None, None, None, ctypes.byref(step), ctypes.byref(info)))
    nodes, recs, cn, cr = _tree_arrays(info.bvh_nodes, len(a))
    check(L.wgt_bvh_refit(ptr(a), ptr(b), len(a), ptr(nodes), info.bvh_nodes, ptr(recs), ptr(cn), ptr(cr),
                          ctypes.byref(step), ctypes.byref(info)))
    return info.as_dict(), nodes, recs, cn, cr, step.value


def bvh_build_morton(tris):
    """Host-only specification of a rebuild (wgt_bvh_build_morton): the tree an upload followed by
    Context.rebuild_triangles(tris) must hold, in bvh_refit's layouts: (info, nodes, leaf-ordered tris,
    cnodes, crefs, step).  The leaf target is WGT_REBUILD_LEAF's, as the rebuild's."""
    t = np.ascontiguousarray(tris, TRI_DTYPE)
    L = lib()
    info = WgtSceneInfo()
    step = ctypes.c_float(0.0)
    check(L.wgt_bvh_build_morton(ptr(t), len(t), None, 0, None, None, None, ctypes.byref(step), ctypes.byref(info)))
    nodes, recs, cn, cr = _tree_arrays(info.bvh_nodes, len(t))
    check(L.wgt_bvh_build_morton(ptr(t), len(t), ptr(nodes), info.bvh_nodes, ptr(recs), ptr(cn), ptr(cr),
                                 ctypes.byref(step), ctypes.byref(info)))
    return info.as_dict(), nodes, recs, cn, cr, step.value


def camera_param(aspect: float, spp: int, seed: int, fovy: float = 40.0, origin=(278.0, 278.0, -800.0),
                 target=(278.0, 278.0, 0.0)):
    """Camera::Update (camera.cpp:64-70) with an explicit seed instead of RandSeed(); origin and
    target default to the reference's constants."""
    cam = np.zeros(1, CAMERA_DTYPE)
    cam["origin"] = origin
    cam["target"] = target
    cam["aspect"] = np.float32(aspect)
    cam["fovy"] = np.float32(fovy)
    cam["spp"] = spp
    cam["seed"] = seed & 0xFFFFFFFF
    return cam


def _ray_soa(start, direction):
    """The ray queries' input (6 planes of n floats: start xyz, then direction xyz) and n."""
    start = np.asarray(start, np.float32).reshape(-1, 3)
    direction = np.asarray(direction, np.float32).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([start.T, direction.T], axis=0), np.float32), len(start)


def _device_hit_buffers(*fields):
    """wgt_hit_buffers of raw device addresses, in HIT_FIELDS' order (0 = field not written)."""
    return WgtHitBuffers(*(f or None for f in fields))


def _nearest_arrays(want, n):
    """Host arrays of the closest-point fields in `want` (planar: pos (3, n), uv (2, n)) and their struct."""
    bad = set(want) - set(NEAREST_FIELDS)
    if bad:
        raise ValueError(f"unknown nearest field(s) {sorted(bad)}; choose from {NEAREST_FIELDS}")
    shape = {"prim": (n,), "dist": (n,), "pos": (3, n), "uv": (2, n)}
    arr = {k: np.zeros(shape[k], np.uint32 if k == "prim" else np.float32) for k in NEAREST_FIELDS if k in want}
    return arr, WgtNearestBuffers(**{k: a.ctypes.data for k, a in arr.items()})


def _nearest_inputs(points, max_dist):
    """The closest-point queries' input: 3 planes of n floats, the limits (a scalar broadcasts) or None, n."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    n = len(points)
    lim = None if max_dist is None else np.ascontiguousarray(np.broadcast_to(np.asarray(max_dist, np.float32), (n,)))
    return np.ascontiguousarray(points.T), lim, n


def _nearest_dict(arr):
    """Vectors last: pos (n, 3), uv (n, 2)."""
    return {k: np.ascontiguousarray(a.T) if k in ("pos", "uv") else a for k, a in arr.items()}


def nearest_points_spec(tris, points, max_dist=None, first_prim=0, want=NEAREST_FIELDS):
    """The closest-point query's definition by brute force on the host (wgt_nearest_points_spec, no
    device): for each point the nearest of `tris` (TRI_DTYPE, ids first_prim + index), as
    Context.nearest_points returns it for a scene that holds these triangles."""
    tris = np.ascontiguousarray(tris, TRI_DTYPE)
    soa, lim, n = _nearest_inputs(points, max_dist)
    arr, bufs = _nearest_arrays(want, n)
    check(lib().wgt_nearest_points_spec(ptr(tris) if len(tris) else None, len(tris), first_prim, ptr(soa), ptr(lim), n,
                                        ctypes.byref(bufs)))
    return _nearest_dict(arr)


def _nearest_k_arrays(want, n, k):
    """Host arrays of the k-nearest fields in `want` (planar: prim (k, n), pos (3k, n), uv (2k, n)), their
    struct, and k as the call takes it."""
    bad = set(want) - set(NEAREST_K_FIELDS)
    if bad:
        raise ValueError(f"unknown nearest field(s) {sorted(bad)}; choose from {NEAREST_K_FIELDS}")
    kk = max(int(k), 0)
    shape = {"count": (n,), "prim": (kk, n), "dist": (kk, n), "pos": (3 * kk, n), "uv": (2 * kk, n)}
    arr = {f: np.zeros(shape[f], np.uint32 if f in ("count", "prim") else np.float32) for f in NEAREST_K_FIELDS if f in want}
    return arr, WgtNearestKBuffers(**{f: a.ctypes.data for f, a in arr.items()}), kk


def _nearest_k_dict(arr, n, k):
    """Points first, entries next, vectors last: prim and dist (n, k), pos (n, k, 3), uv (n, k, 2)."""
    out = {}
    for f, a in arr.items():
        if f == "count":
            out[f] = a
        elif f in ("prim", "dist"):
            out[f] = np.ascontiguousarray(a.T)
        else:
            out[f] = np.ascontiguousarray(a.reshape(k, 3 if f == "pos" else 2, n).transpose(2, 0, 1))
    return out


def nearest_k_points_spec(tris, points, k, max_dist=None, first_prim=0, want=NEAREST_K_FIELDS):
    """The k-nearest query's definition by brute force on the host (wgt_nearest_k_points_spec, no device):
    what Context.nearest_k_points returns for a scene that holds `tris` (TRI_DTYPE, ids first_prim + index)."""
    tris = np.ascontiguousarray(tris, TRI_DTYPE)
    soa, lim, n = _nearest_inputs(points, max_dist)
    arr, bufs, kk = _nearest_k_arrays(want, n, k)
    check(lib().wgt_nearest_k_points_spec(ptr(tris) if len(tris) else None, len(tris), first_prim, ptr(soa), ptr(lim), n,
                                          kk, ctypes.byref(bufs)))
    return _nearest_k_dict(arr, n, kk)


def _overlap_inputs(tris):
    """The overlap queries' input: (n, 3, 3) corners as nine planes of n floats (a0.x a0.y a0.z a1.x ... a2.z), n."""
    tris = np.asarray(tris, np.float32).reshape(-1, 9)
    return np.ascontiguousarray(tris.T), len(tris)


def _overlap_arrays(want, n, k):
    """Host arrays of the overlap fields in `want` (planar: prim (k, n)), their struct, and k as the call takes it."""
    bad = set(want) - set(OVERLAP_FIELDS)
    if bad:
        raise ValueError(f"unknown overlap field(s) {sorted(bad)}; choose from {OVERLAP_FIELDS}")
    kk = max(int(k), 0)
    shape = {"hit": (n,), "count": (n,), "prim": (kk, n)}
    arr = {f: np.zeros(shape[f], np.uint8 if f == "hit" else np.uint32) for f in OVERLAP_FIELDS if f in want}
    return arr, WgtOverlapBuffers(**{f: a.ctypes.data for f, a in arr.items()}), kk


def _overlap_dict(arr):
    """Queries first: hit (n,) bool, count (n,), prim (n, k)."""
    return {f: a.astype(bool) if f == "hit" else (np.ascontiguousarray(a.T) if f == "prim" else a) for f, a in arr.items()}


def overlap_triangles_spec(T, tris, k, first_prim=0, want=OVERLAP_FIELDS):
    """The overlap query's definition by brute force on the host (wgt_overlap_triangles_spec, no device): what
    Context.overlap_triangles returns for a scene that holds `T` (TRI_DTYPE, ids first_prim + index) and the
    query triangles `tris` ((n, 3, 3) corners)."""
    T = np.ascontiguousarray(T, TRI_DTYPE)
    soa, n = _overlap_inputs(tris)
    arr, bufs, kk = _overlap_arrays(want, n, k)
    check(lib().wgt_overlap_triangles_spec(ptr(T) if len(T) else None, len(T), first_prim, ptr(soa), n, kk, ctypes.byref(bufs)))
    return _overlap_dict(arr)


def _self_indices(indices, n_tris):
    """The self-intersection queries' index buffer: (n_tris, 3) labels as 3 * n_tris uint32, or None."""
    if indices is None:
        return None
    idx = np.ascontiguousarray(np.asarray(indices, np.uint32).reshape(-1))
    if len(idx) != 3 * n_tris:
        raise ValueError(f"indices hold {len(idx)} labels, the mesh has {n_tris} triangles: 3 per triangle are needed")
    return idx


def overlap_self_spec(T, indices=None, k=0, first_prim=0, want=OVERLAP_FIELDS):
    """The self-intersection query's definition by brute force on the host (wgt_overlap_self_spec, no device):
    what Context.overlap_self returns for a scene that holds `T` (TRI_DTYPE, ids first_prim + index) and the
    index buffer `indices` ((n_tris, 3) labels, or None: nothing is adjacent)."""
    T = np.ascontiguousarray(T, TRI_DTYPE)
    idx = _self_indices(indices, len(T))
    arr, bufs, kk = _overlap_arrays(want, len(T), k)
    check(lib().wgt_overlap_self_spec(ptr(T) if len(T) else None, len(T), first_prim, ptr(idx), kk, ctypes.byref(bufs)))
    return _overlap_dict(arr)


def build_id() -> str:
    """The loaded library's kernel build id (wgt_build_id: hash of the HIP sources and flags)."""
    return lib().wgt_build_id().decode()


def denoise_defaults():
    """wgt_denoise_defaults: a WgtDenoiseParams of the library's defaults."""
    p = WgtDenoiseParams()
    check(lib().wgt_denoise_defaults(ctypes.byref(p)))
    return p


def denoise_workspace_bytes(W: int, H: int) -> int:
    """Bytes of device scratch Context.denoise_async needs for a W x H image (0: a size it refuses)."""
    return int(lib().wgt_denoise_workspace_bytes(W, H))


def denoise_variance_defaults():
    """wgt_denoise_variance_defaults: a WgtDenoiseVarianceParams of the library's defaults."""
    p = WgtDenoiseVarianceParams()
    check(lib().wgt_denoise_variance_defaults(ctypes.byref(p)))
    return p


def denoise_variance_workspace_bytes(W: int, H: int) -> int:
    """Bytes of device scratch Context.denoise_variance_async needs for a W x H image (0: a size it refuses)."""
    return int(lib().wgt_denoise_variance_workspace_bytes(W, H))


def sample_plan_defaults():
    """wgt_sample_plan_defaults: a WgtSamplePlanParams of the library's defaults."""
    p = WgtSamplePlanParams()
    check(lib().wgt_sample_plan_defaults(ctypes.byref(p)))
    return p


def sample_plan_workspace_bytes(W: int, H: int) -> int:
    """Bytes of device scratch Context.sample_plan_async needs for a W x H image (0: a size it refuses)."""
    return int(lib().wgt_sample_plan_workspace_bytes(W, H))


def _host_sample_map(sample_map, W, H):
    """A (H, W) uint8 sample map as the contiguous host array the sampled calls read."""
    m = np.ascontiguousarray(sample_map, np.uint8)
    if m.shape != (H, W):
        raise ValueError(f"sample_map has shape {m.shape}, not the frame's (H, W) = ({H}, {W})")
    return m


def temporal_defaults():
    """wgt_temporal_defaults: a WgtTemporalParams of the library's defaults."""
    p = WgtTemporalParams()
    check(lib().wgt_temporal_defaults(ctypes.byref(p)))
    return p


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = lib().wgt_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


class Context:
    """A HIP device context (wgt_ctx): owns the stream and the scene in HBM."""

    def __init__(self, device: int = 0):
        self._L = lib()
        h = ctypes.c_void_p()
        check(self._L.wgt_create(device, ctypes.byref(h)))
        self.h = h
        self.device = device
        self.n_prims = 0

    def close(self):
        if getattr(self, "h", None):
            self._L.wgt_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        return check(rc, self.h)

    def upload_scene(self, lights, quads, spheres, tris=None):
        lights = np.ascontiguousarray(lights, QUAD_DTYPE)
        quads = np.ascontiguousarray(quads, QUAD_DTYPE)
        spheres = np.ascontiguousarray(spheres, SPHERE_DTYPE)
        tris = np.zeros(0, TRI_DTYPE) if tris is None else np.ascontiguousarray(tris, TRI_DTYPE)
        self._check(self._L.wgt_upload_scene(self.h, ptr(lights), len(lights), ptr(quads), len(quads),
                                             ptr(spheres), len(spheres), ptr(tris) if len(tris) else None,
                                             len(tris)))
        self.n_prims = len(lights) + len(quads) + len(tris) + len(spheres)

    def scene_info(self):
        info = WgtSceneInfo()
        self._check(self._L.wgt_scene_info_get(self.h, ctypes.byref(info)))
        return info.as_dict()

    def update_triangles(self, tris):
        """Move the uploaded scene's triangles (wgt_update_triangles): the resident BVH is refit on the
        device, not rebuilt.  Triangle i keeps its primitive id; len(tris) must be the uploaded count.
        Synchronous; every render and query afterwards equals a fresh upload's, bit for bit."""
        tris = np.ascontiguousarray(tris, TRI_DTYPE)
        self._check(self._L.wgt_update_triangles(self.h, ptr(tris), len(tris)))

    def update_triangles_device(self, d_tris, n_tris, stream=0):
        """update_triangles from device memory (wgt_update_triangles_device): d_tris is the raw device
        address of n_tris TRI_DTYPE records, 16-byte aligned.  Synchronous: the records are read after
        everything queued on `stream` (0 = the context's), and may be overwritten once it returns."""
        self._check(self._L.wgt_update_triangles_device(self.h, ctypes.c_void_p(d_tris or None), n_tris,
                                                        ctypes.c_void_p(stream or None)))

    def update_vertices_device(self, d_verts, n_verts, n_tris, d_index=0, stream=0):
        """The same from moved vertices (wgt_update_vertices_device): d_verts is the raw device address of
        n_verts x 3 float32, d_index that of n_tris x 3 uint32 vertex indices (0 = unindexed: triangle i
        uses vertices 3i .. 3i + 2, and n_verts must be 3 * n_tris).  Each triangle becomes what
        make_triangles builds from its vertices and keeps its colour and emissive flag."""
        self._check(self._L.wgt_update_vertices_device(self.h, ctypes.c_void_p(d_verts or None), n_verts,
                                                       ctypes.c_void_p(d_index or None), n_tris,
                                                       ctypes.c_void_p(stream or None)))

    def _set_triangle_count(self, n_tris):
        info = self.scene_info()
        self.n_prims = info["n_lights"] + info["n_quads"] + n_tris + info["n_spheres"]

    def rebuild_triangles(self, tris):
        """Replace the scene's triangles by `tris` (any count >= 1) and rebuild their BVH on the device
        (wgt_rebuild_triangles).  Triangle i gets primitive id n_lights + n_quads + i, so sphere ids move
        when the count changes.  Synchronous; every render and query afterwards equals a fresh upload's,
        bit for bit."""
        tris = np.ascontiguousarray(tris, TRI_DTYPE)
        self._check(self._L.wgt_rebuild_triangles(self.h, ptr(tris) if len(tris) else None, len(tris)))
        self._set_triangle_count(len(tris))

    def rebuild_triangles_device(self, d_tris, n_tris, stream=0):
        """rebuild_triangles from device memory (wgt_rebuild_triangles_device): d_tris is the raw device
        address of n_tris TRI_DTYPE records, 16-byte aligned.  Synchronous: the records are read after
        everything queued on `stream` (0 = the context's), and may be overwritten once it returns."""
        self._check(self._L.wgt_rebuild_triangles_device(self.h, ctypes.c_void_p(d_tris or None), n_tris,
                                                         ctypes.c_void_p(stream or None)))
        self._set_triangle_count(n_tris)

    def update_timing(self):
        """(host_ms, device_ms) of the last update or rebuild, of any form (wgt_update_timing)."""
        h, d = ctypes.c_float(0.0), ctypes.c_float(0.0)
        self._check(self._L.wgt_update_timing(self.h, ctypes.byref(h), ctypes.byref(d)))
        return h.value, d.value

    def bvh_read(self):
        """The resident tree (wgt_bvh_read), in bvh_refit's layouts without the info:
        (nodes, leaf-ordered tris, cnodes, crefs, step)."""
        info = self.scene_info()
        nodes, recs, cn, cr = _tree_arrays(info["bvh_nodes"], info["n_tris"])
        step = ctypes.c_float(0.0)
        self._check(self._L.wgt_bvh_read(self.h, ptr(nodes), info["bvh_nodes"], ptr(recs), ptr(cn), ptr(cr),
                                         ctypes.byref(step)))
        return nodes, recs, cn, cr, step.value

    def render_tile(self, cam, W, H, x0=0, y0=0, tw=None, th=None, want=("u8", "f32", "hit"), stats=False,
                    sample_map=None):
        """wgt_render_tile; with sample_map, a (H, W) uint8 array of per-pixel sample-grid sides over the
        whole frame, wgt_render_tile_sampled: pixel (x, y) is rendered at spp = sample_map[y, x] ** 2
        and cam's spp is ignored."""
        tw = W if tw is None else tw
        th = H if th is None else th
        u8 = np.zeros((th, tw, 4), np.uint8) if "u8" in want else None
        f32 = np.zeros((th, tw, 4), np.float32) if "f32" in want else None
        hit = np.zeros((th, tw), np.uint32) if "hit" in want else None
        st = WgtStats() if stats else None
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        if sample_map is not None:
            m = _host_sample_map(sample_map, W, H)
            self._check(self._L.wgt_render_tile_sampled(self.h, ptr(cam), W, H, x0, y0, tw, th, ptr(m), ptr(u8),
                                                        ptr(f32), ptr(hit),
                                                        ctypes.byref(st) if st is not None else None))
            return {"u8": u8, "f32": f32, "hit": hit, "stats": st.as_dict() if st is not None else None}
        self._check(self._L.wgt_render_tile(self.h, ptr(cam), W, H, x0, y0, tw, th, ptr(u8), ptr(f32), ptr(hit),
                                            ctypes.byref(st) if st is not None else None))
        return {"u8": u8, "f32": f32, "hit": hit, "stats": st.as_dict() if st is not None else None}

    def render_frames(self, cam, W, H, seeds, stats=False):
        """n whole frames in one launch (wgt_render_frames): (n, H, W, 4) uint8 (+ stats)."""
        seeds = np.ascontiguousarray(seeds, np.uint32)
        out = np.zeros((len(seeds), H, W, 4), np.uint8)
        st = WgtStats() if stats else None
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        self._check(self._L.wgt_render_frames(self.h, ptr(cam), W, H, ptr(seeds), len(seeds), ptr(out),
                                              ctypes.byref(st) if st is not None else None))
        return (out, st.as_dict()) if stats else out

    def render_tiles_async(self, cam, W, H, tw, th, d_tiles, n_tiles, d_u8=0, d_f32=0, d_hit=0, stream=0,
                           d_sample_map=0):
        """Device-pointer launch (ints are raw device addresses, 0 = NULL).  d_sample_map: the frame's
        W x H uint8 sample map on the device (wgt_render_tiles_sampled_async; cam's spp is ignored)."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        if d_sample_map:
            self._check(self._L.wgt_render_tiles_sampled_async(
                self.h, ptr(cam), W, H, tw, th, ctypes.c_void_p(d_tiles), n_tiles, ctypes.c_void_p(d_sample_map),
                ctypes.c_void_p(d_u8 or None), ctypes.c_void_p(d_f32 or None), ctypes.c_void_p(d_hit or None),
                ctypes.c_void_p(stream or None)))
            return
        self._check(self._L.wgt_render_tiles_async(self.h, ptr(cam), W, H, tw, th, ctypes.c_void_p(d_tiles),
                                                   n_tiles, ctypes.c_void_p(d_u8 or None),
                                                   ctypes.c_void_p(d_f32 or None), ctypes.c_void_p(d_hit or None),
                                                   ctypes.c_void_p(stream or None)))

    def order_info(self):
        """How the persistent kernel's launches got their queue order since the context was made
        (wgt_order_info): counts of today / refine / reuse launches and of invalidations, and the kept
        order's block count and pre-pass side (0 when none is kept)."""
        st = WgtOrderStats()
        self._check(self._L.wgt_order_info(self.h, ctypes.byref(st)))
        return st.as_dict()

    def order_read(self):
        """The kept queue order (wgt_order_read): a uint32 permutation of range(nb), empty when none is kept."""
        out = np.zeros(max(self.order_info()["nb"], 1), np.uint32)
        n = ctypes.c_uint32(0)
        self._check(self._L.wgt_order_read(self.h, ptr(out), len(out), ctypes.byref(n)))
        return out[:n.value]

    def order_reset(self):
        """Drop the kept queue order (wgt_order_reset): the next launch is the first of its view."""
        self._check(self._L.wgt_order_reset(self.h))

    def render_tiles_stats(self, cam, W, H, tw, th, d_tiles, n_tiles):
        st = WgtStats()
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        self._check(self._L.wgt_render_tiles_stats(self.h, ptr(cam), W, H, tw, th, ctypes.c_void_p(d_tiles),
                                                   n_tiles, ctypes.byref(st)))
        return st.as_dict()

    def render_tiles_profile(self, cam, W, H, tw, th, d_tiles, n_tiles):
        st = WgtStats()
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        self._check(self._L.wgt_render_tiles_profile(self.h, ptr(cam), W, H, tw, th, ctypes.c_void_p(d_tiles),
                                                     n_tiles, ctypes.byref(st)))
        return st.as_dict()

    def trace_rays(self, start, direction):
        soa, n = _ray_soa(start, direction)
        prim = np.zeros(n, np.uint32)
        dist = np.zeros(n, np.float32)
        self._check(self._L.wgt_trace_rays(self.h, ptr(soa), n, ptr(prim), ptr(dist)))
        return prim, dist

    def trace_rays_async(self, d_rays, n, d_prim, d_dist, stream=0):
        self._check(self._L.wgt_trace_rays_async(self.h, ctypes.c_void_p(d_rays), n, ctypes.c_void_p(d_prim),
                                                 ctypes.c_void_p(d_dist), ctypes.c_void_p(stream or None)))

    def occluded(self, start, direction, max_dist):
        """Any-hit query (wgt_occluded_rays): bool per ray, True iff trace_rays on it returns a
        primitive at a distance below max_dist (scene units; a scalar broadcasts)."""
        soa, n = _ray_soa(start, direction)
        lim = np.ascontiguousarray(np.broadcast_to(np.asarray(max_dist, np.float32), (n,)))
        out = np.zeros(n, np.uint8)
        self._check(self._L.wgt_occluded_rays(self.h, ptr(soa), ptr(lim), n, ptr(out)))
        return out.astype(bool)

    def occluded_async(self, d_rays, d_max_dist, n, d_out, stream=0):
        """Device-pointer launch (raw device addresses): d_out receives n bytes, 0 or 1."""
        self._check(self._L.wgt_occluded_rays_async(self.h, ctypes.c_void_p(d_rays), ctypes.c_void_p(d_max_dist), n,
                                                    ctypes.c_void_p(d_out), ctypes.c_void_p(stream or None)))

    @staticmethod
    def _hit_arrays(want, shape):
        """Host arrays of the hit-record fields in `want` (planar vectors: (3,) + shape) and their struct."""
        bad = set(want) - set(HIT_FIELDS)
        if bad:
            raise ValueError(f"unknown hit field(s) {sorted(bad)}; choose from {HIT_FIELDS}")
        dt = {"prim": np.uint32, "flags": np.uint8}
        arr = {k: np.zeros(((3,) if k in ("pos", "norm", "col") else ()) + shape, dt.get(k, np.float32))
               for k in HIT_FIELDS if k in want}
        return arr, WgtHitBuffers(**{k: a.ctypes.data for k, a in arr.items()})

    @staticmethod
    def _hit_dict(arr):
        """Vectors last: (3,) + shape -> shape + (3,)."""
        return {k: np.ascontiguousarray(np.moveaxis(a, 0, -1)) if k in ("pos", "norm", "col") else a
                for k, a in arr.items()}

    def trace_hits(self, start, direction, want=HIT_FIELDS):
        """Whole hit records (wgt_trace_hits): a dict of the fields in `want`; prim (n,) uint32 and
        dist (n,) as trace_rays, pos / norm / col (n, 3), flags (n,) uint8 (WGT_HIT_EMISSIVE |
        WGT_HIT_FRONT_FACE)."""
        soa, n = _ray_soa(start, direction)
        arr, bufs = self._hit_arrays(want, (n,))
        self._check(self._L.wgt_trace_hits(self.h, ptr(soa), n, ctypes.byref(bufs)))
        return self._hit_dict(arr)

    def trace_hits_async(self, d_rays, n, prim=0, dist=0, pos=0, norm=0, col=0, flags=0, stream=0):
        """Device-pointer launch (raw device addresses, 0 = field not written): pos / norm / col
        receive 3 planes of n floats."""
        bufs = _device_hit_buffers(prim, dist, pos, norm, col, flags)
        self._check(self._L.wgt_trace_hits_async(self.h, ctypes.c_void_p(d_rays), n, ctypes.byref(bufs),
                                                 ctypes.c_void_p(stream or None)))

    def nearest_points(self, points, max_dist=None, want=NEAREST_FIELDS):
        """Closest-point query (wgt_nearest_points): for each point the scene's nearest triangle, a dict of
        the fields in `want`: prim (n,) uint32 as trace_rays numbers triangles, dist (n,), pos (n, 3) the
        closest point, uv (n, 2) its weights of e1 and e2.  max_dist (scene units; a scalar broadcasts;
        None = no radius): a record is reported iff dist < max_dist, else prim = 0xffffffff, dist = inf,
        zeros.  Equals nearest_points_spec on the resident triangles bit for bit."""
        soa, lim, n = _nearest_inputs(points, max_dist)
        arr, bufs = _nearest_arrays(want, n)
        self._check(self._L.wgt_nearest_points(self.h, ptr(soa), ptr(lim), n, ctypes.byref(bufs)))
        return _nearest_dict(arr)

    def nearest_points_async(self, d_points, n, d_max_dist=0, prim=0, dist=0, pos=0, uv=0, stream=0):
        """Device-pointer launch (raw device addresses, 0 = NULL): d_points 3 planes of n floats, d_max_dist
        n floats or 0; pos receives 3 planes of n floats, uv 2."""
        bufs = WgtNearestBuffers(prim or None, dist or None, pos or None, uv or None)
        self._check(self._L.wgt_nearest_points_async(self.h, ctypes.c_void_p(d_points or None),
                                                     ctypes.c_void_p(d_max_dist or None), n, ctypes.byref(bufs),
                                                     ctypes.c_void_p(stream or None)))

    def nearest_points_stats(self, d_points, n, d_max_dist=0, prim=0, dist=0, pos=0, uv=0):
        """The same answers from the counting kernel (wgt_nearest_points_stats; synchronous, device
        pointers): -> (node visits, triangle tests) summed over the n points."""
        bufs = WgtNearestBuffers(prim or None, dist or None, pos or None, uv or None)
        counts = (ctypes.c_uint64 * 2)()
        self._check(self._L.wgt_nearest_points_stats(self.h, ctypes.c_void_p(d_points or None),
                                                     ctypes.c_void_p(d_max_dist or None), n, ctypes.byref(bufs), counts))
        return int(counts[0]), int(counts[1])

    def nearest_k_points(self, points, k, max_dist=None, want=NEAREST_K_FIELDS):
        """k-nearest and within-radius closest-point query (wgt_nearest_k_points): the triangles within
        max_dist of each point (scene units; a scalar broadcasts; None = no radius), a dict of the fields in
        `want`: count (n,) uint32 the number of all of them, and of the k nearest by (squared distance, prim)
        prim (n, k) uint32, dist (n, k), pos (n, k, 3) the closest points, uv (n, k, 2) their weights;
        0xffffffff, inf and zeros beyond the point's triangles.  Entry 0 is nearest_points' record.  With
        "count" wanted every triangle within the radius is visited; without it the search stops looking
        beyond the k-th distance (the same lists).  Equals nearest_k_points_spec on the resident triangles
        bit for bit."""
        soa, lim, n = _nearest_inputs(points, max_dist)
        arr, bufs, kk = _nearest_k_arrays(want, n, k)
        self._check(self._L.wgt_nearest_k_points(self.h, ptr(soa), ptr(lim), n, kk, ctypes.byref(bufs)))
        return _nearest_k_dict(arr, n, kk)

    def nearest_k_points_async(self, d_points, n, k, d_max_dist=0, count=0, prim=0, dist=0, pos=0, uv=0, stream=0):
        """Device-pointer launch (raw device addresses, 0 = NULL): d_points 3 planes of n floats, d_max_dist
        n floats or 0; count receives n uint32, prim and dist k planes of n, pos 3k planes (3 j + axis), uv 2k."""
        bufs = WgtNearestKBuffers(count or None, prim or None, dist or None, pos or None, uv or None)
        self._check(self._L.wgt_nearest_k_points_async(self.h, ctypes.c_void_p(d_points or None),
                                                       ctypes.c_void_p(d_max_dist or None), n, k, ctypes.byref(bufs),
                                                       ctypes.c_void_p(stream or None)))

    def nearest_k_points_stats(self, d_points, n, k, d_max_dist=0, count=0, prim=0, dist=0, pos=0, uv=0):
        """The same answers from the counting kernel (wgt_nearest_k_points_stats; synchronous, device
        pointers): -> (node visits, triangle tests) summed over the n points."""
        bufs = WgtNearestKBuffers(count or None, prim or None, dist or None, pos or None, uv or None)
        counts = (ctypes.c_uint64 * 2)()
        self._check(self._L.wgt_nearest_k_points_stats(self.h, ctypes.c_void_p(d_points or None),
                                                       ctypes.c_void_p(d_max_dist or None), n, k, ctypes.byref(bufs),
                                                       counts))
        return int(counts[0]), int(counts[1])

    def overlap_triangles(self, tris, k, want=OVERLAP_FIELDS):
        """Triangle overlap query (wgt_overlap_triangles): the resident triangles each of `tris` ((n, 3, 3)
        corners) cuts, a dict of the fields in `want`: hit (n,) bool whether there is one, count (n,) uint32 the
        number of all of them, prim (n, k) uint32 the k <= 32 lowest primitive ids of them, 0xffffffff beyond
        the query's triangles.  k is the list's length: at least 1 with "prim" wanted, 0 without.  Two
        triangles overlap when an edge of one crosses the other (touching counts, coplanar pairs never do);
        with "hit" alone the search ends at the first one.  Equals overlap_triangles_spec on the resident
        triangles bit for bit."""
        soa, n = _overlap_inputs(tris)
        arr, bufs, kk = _overlap_arrays(want, n, k)
        self._check(self._L.wgt_overlap_triangles(self.h, ptr(soa), n, kk, ctypes.byref(bufs)))
        return _overlap_dict(arr)

    def overlap_triangles_async(self, d_tris, n, k, hit=0, count=0, prim=0, stream=0):
        """Device-pointer launch (raw device addresses, 0 = NULL): d_tris 9 planes of n floats; hit receives n
        bytes, count n uint32, prim k planes of n uint32."""
        bufs = WgtOverlapBuffers(hit or None, count or None, prim or None)
        self._check(self._L.wgt_overlap_triangles_async(self.h, ctypes.c_void_p(d_tris or None), n, k, ctypes.byref(bufs),
                                                        ctypes.c_void_p(stream or None)))

    def overlap_triangles_stats(self, d_tris, n, k, hit=0, count=0, prim=0):
        """The same answers from the counting kernel (wgt_overlap_triangles_stats; synchronous, device
        pointers): -> (node visits, triangle tests) summed over the n queries."""
        bufs = WgtOverlapBuffers(hit or None, count or None, prim or None)
        counts = (ctypes.c_uint64 * 2)()
        self._check(self._L.wgt_overlap_triangles_stats(self.h, ctypes.c_void_p(d_tris or None), n, k, ctypes.byref(bufs),
                                                        counts))
        return int(counts[0]), int(counts[1])

    def overlap_self(self, indices=None, k=0, want=OVERLAP_FIELDS):
        """Self-intersection query (wgt_overlap_self): the resident triangles each resident triangle cuts, a dict
        of the fields in `want`, indexed by upload index: hit (n_tris,) bool, count (n_tris,) uint32 the number
        of all of them, prim (n_tris, k) uint32 the k <= 32 lowest primitive ids of them, 0xffffffff beyond.
        `indices` ((n_tris, 3) vertex labels) is the only statement of adjacency: two triangles that share a
        label never report each other; with None nothing is adjacent.  k is the list's length: at least 1 with
        "prim" wanted, 0 without.  The decision is symmetric (t in s's set iff s in t's); with "hit" alone the
        search ends at the first member.  Equals overlap_self_spec on the resident triangles bit for bit."""
        n = self.scene_info()["n_tris"]
        idx = _self_indices(indices, n)
        arr, bufs, kk = _overlap_arrays(want, n, k)
        self._check(self._L.wgt_overlap_self(self.h, ptr(idx), kk, ctypes.byref(bufs)))
        return _overlap_dict(arr)

    def overlap_self_async(self, d_indices, k, hit=0, count=0, prim=0, stream=0):
        """Device-pointer launch (raw device addresses, 0 = NULL): d_indices 3 * n_tris uint32 labels or 0; hit
        receives n_tris bytes, count n_tris uint32, prim k planes of n_tris uint32."""
        bufs = WgtOverlapBuffers(hit or None, count or None, prim or None)
        self._check(self._L.wgt_overlap_self_async(self.h, ctypes.c_void_p(d_indices or None), k, ctypes.byref(bufs),
                                                   ctypes.c_void_p(stream or None)))

    def overlap_self_stats(self, d_indices, k, hit=0, count=0, prim=0):
        """The same answers from the counting kernel (wgt_overlap_self_stats; synchronous, device pointers):
        -> (node visits, triangle tests) summed over the resident triangles."""
        bufs = WgtOverlapBuffers(hit or None, count or None, prim or None)
        counts = (ctypes.c_uint64 * 2)()
        self._check(self._L.wgt_overlap_self_stats(self.h, ctypes.c_void_p(d_indices or None), k, ctypes.byref(bufs),
                                                   counts))
        return int(counts[0]), int(counts[1])

    def self_intersections(self, indices, k=32):
        """The mesh's self-intersections as pairs: (pairs, truncated).  pairs is (m, 2) int64, the unique pairs
        (s, t) of upload indices with s < t that overlap_self(indices, k) lists, in lexicographic order;
        truncated is True when a triangle cuts more than k others, so that its list (and, if every partner's
        list is cut short too, the pairs) may be incomplete.  Python over the query: no kernel of its own."""
        r = self.overlap_self(indices, k, want=("count", "prim"))
        info = self.scene_info()
        s, j = np.nonzero(r["prim"] != 0xFFFFFFFF)
        t = r["prim"][s, j].astype(np.int64) - (info["n_lights"] + info["n_quads"])
        pairs = np.unique(np.stack([np.minimum(s, t), np.maximum(s, t)], 1), axis=0) if len(s) else np.zeros((0, 2), np.int64)
        return pairs.astype(np.int64), bool((r["count"] > k).any())

    def trace_radiance(self, start, direction, seeds=None, seed0=0, samples=1, want=RADIANCE_FIELDS):
        """Radiance query (wgt_trace_radiance): `samples` paths of the renderer's raytrace() along each
        caller ray, a dict of the fields in `want`: rgb (n, 3) the mean of max(path colour, 0), prim (n,)
        uint32 the primitive the first path's ray hits, seed (n,) uint32 the RNG state after the last
        path.  Ray i starts from seeds[i], or from seed0 + i (32-bit wrap-around) when seeds is None.
        Feeding `seed` back as `seeds` chains calls: S one-sample calls summed as col + c / f32(S) in
        fp32 equal one call with S samples.  A frame at spp = 1 is this query on render_gbuffer's rays
        from the state two rand() past each pixel's seed."""
        bad = set(want) - set(RADIANCE_FIELDS)
        if bad:
            raise ValueError(f"unknown radiance field(s) {sorted(bad)}; choose from {RADIANCE_FIELDS}")
        soa, n = _ray_soa(start, direction)
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
            if len(seeds) != n:
                raise ValueError(f"{len(seeds)} seeds for {n} rays")
        arr = {"rgb": np.zeros((3, n), np.float32), "prim": np.zeros(n, np.uint32), "seed": np.zeros(n, np.uint32)}
        arr = {k: a for k, a in arr.items() if k in want}
        bufs = WgtRadianceBuffers(ptr(arr.get("rgb")), ptr(arr.get("prim")), ptr(arr.get("seed")))
        self._check(self._L.wgt_trace_radiance(self.h, ptr(soa), ptr(seeds), seed0 & 0xFFFFFFFF, samples, n,
                                               ctypes.byref(bufs)))
        return {k: np.ascontiguousarray(a.T) if k == "rgb" else a for k, a in arr.items()}

    def trace_radiance_async(self, d_rays, n, d_seeds=0, seed0=0, samples=1, rgb=0, prim=0, seed=0, stream=0):
        """Device-pointer launch (raw device addresses, 0 = NULL): d_rays 6 planes of n floats, d_seeds n
        uint32 or 0 (then seed0 + i); rgb receives 3 planes of n floats, prim and seed n uint32."""
        bufs = WgtRadianceBuffers(rgb or None, prim or None, seed or None)
        self._check(self._L.wgt_trace_radiance_async(self.h, ctypes.c_void_p(d_rays or None),
                                                     ctypes.c_void_p(d_seeds or None), seed0 & 0xFFFFFFFF, samples, n,
                                                     ctypes.byref(bufs), ctypes.c_void_p(stream or None)))

    def trace_radiance_stats(self, d_rays, n, d_seeds=0, seed0=0, samples=1, rgb=0, prim=0, seed=0):
        """The same answers from the counting kernel (wgt_trace_radiance_stats; synchronous, device
        pointers): -> (queries, traced, samples, nan_rays) summed over the n rays, the oracle's counters."""
        bufs = WgtRadianceBuffers(rgb or None, prim or None, seed or None)
        counts = (ctypes.c_uint64 * 4)()
        self._check(self._L.wgt_trace_radiance_stats(self.h, ctypes.c_void_p(d_rays or None),
                                                     ctypes.c_void_p(d_seeds or None), seed0 & 0xFFFFFFFF, samples, n,
                                                     ctypes.byref(bufs), counts))
        return tuple(int(c) for c in counts)

    def trace_multi_hits(self, start, direction, k, max_dist=None, tris_only=False, want=MULTI_HIT_FIELDS):
        """Multi-hit query (wgt_trace_multi_hits): every primitive ray i hits below max_dist (scene units; a
        scalar broadcasts; None = no limit), a dict of the fields in `want`: count (n,) uint32 the number of
        all hits, prim (n, k) uint32 and dist (n, k) the k nearest by (dist, prim), 0xffffffff and inf
        beyond the ray's hits.  tris_only: the scene's triangles only.  With "count" wanted every hit is
        visited; without it the search stops looking beyond the k-th distance (the same prim and dist)."""
        bad = set(want) - set(MULTI_HIT_FIELDS)
        if bad:
            raise ValueError(f"unknown multi-hit field(s) {sorted(bad)}; choose from {MULTI_HIT_FIELDS}")
        soa, n = _ray_soa(start, direction)
        lim = None if max_dist is None else np.ascontiguousarray(np.broadcast_to(np.asarray(max_dist, np.float32), (n,)))
        kk = max(int(k), 0)
        arr = {"count": np.zeros(n, np.uint32), "prim": np.zeros((kk, n), np.uint32), "dist": np.zeros((kk, n), np.float32)}
        arr = {f: a for f, a in arr.items() if f in want}
        bufs = WgtMultiHitBuffers(**{f: a.ctypes.data for f, a in arr.items()})
        self._check(self._L.wgt_trace_multi_hits(self.h, ptr(soa), ptr(lim), n, kk,
                                                 WGT_MULTI_HIT_TRIS_ONLY if tris_only else 0, ctypes.byref(bufs)))
        return {f: a if f == "count" else np.ascontiguousarray(a.T) for f, a in arr.items()}

    def trace_multi_hits_async(self, d_rays, n, k, d_max_dist=0, tris_only=False, count=0, prim=0, dist=0, stream=0):
        """Device-pointer launch (raw device addresses, 0 = NULL): d_rays 6 planes of n floats, d_max_dist n
        floats or 0; count receives n uint32, prim and dist k planes of n."""
        bufs = WgtMultiHitBuffers(count or None, prim or None, dist or None)
        self._check(self._L.wgt_trace_multi_hits_async(self.h, ctypes.c_void_p(d_rays or None),
                                                       ctypes.c_void_p(d_max_dist or None), n, k,
                                                       WGT_MULTI_HIT_TRIS_ONLY if tris_only else 0, ctypes.byref(bufs),
                                                       ctypes.c_void_p(stream or None)))

    def trace_multi_hits_stats(self, d_rays, n, k, d_max_dist=0, tris_only=False, count=0, prim=0, dist=0):
        """The same answers from the counting kernel (wgt_trace_multi_hits_stats; synchronous, device
        pointers): -> (node visits, triangle tests) summed over the n rays."""
        bufs = WgtMultiHitBuffers(count or None, prim or None, dist or None)
        counts = (ctypes.c_uint64 * 2)()
        self._check(self._L.wgt_trace_multi_hits_stats(self.h, ctypes.c_void_p(d_rays or None),
                                                       ctypes.c_void_p(d_max_dist or None), n, k,
                                                       WGT_MULTI_HIT_TRIS_ONLY if tris_only else 0, ctypes.byref(bufs),
                                                       counts))
        return int(counts[0]), int(counts[1])

    def points_inside(self, points, direction=(0.5377, 0.3183, 0.7807)):
        """bool per point: inside the scene's triangle mesh, by crossing parity: one ray per point along
        `direction` through the triangles only, count & 1.  Valid for closed meshes; undefined for a point
        whose ray passes within rounding of an edge or a silhouette (a crossing counted twice or not at all)."""
        points = np.asarray(points, np.float32).reshape(-1, 3)
        d = np.broadcast_to(np.asarray(direction, np.float32), points.shape)
        return (self.trace_multi_hits(points, d, 0, tris_only=True, want=("count",))["count"] & 1).astype(bool)

    def render_gbuffer(self, cam, W, H, x0=0, y0=0, tw=None, th=None, want=HIT_FIELDS, rays=False, sample_map=None):
        """First-hit G-buffer (wgt_render_gbuffer): the hit record of sample 0's primary ray of each
        pixel of the rectangle, (th, tw) and (th, tw, 3) arrays; rays=True adds that ray as
        "origin" and "direction", (th, tw, 3) each.  sample_map: the (H, W) uint8 map of the sampled
        frame this G-buffer belongs to (wgt_render_gbuffer_sampled; cam's spp is ignored)."""
        tw = W if tw is None else tw
        th = H if th is None else th
        arr, bufs = self._hit_arrays(want, (th, tw))
        r = np.zeros((6, th, tw), np.float32) if rays else None
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        if sample_map is not None:
            m = _host_sample_map(sample_map, W, H)
            self._check(self._L.wgt_render_gbuffer_sampled(self.h, ptr(cam), W, H, x0, y0, tw, th, ptr(m),
                                                           ctypes.byref(bufs), ptr(r)))
        else:
            self._check(self._L.wgt_render_gbuffer(self.h, ptr(cam), W, H, x0, y0, tw, th, ctypes.byref(bufs),
                                                   ptr(r)))
        out = self._hit_dict(arr)
        if rays:
            out["origin"] = np.ascontiguousarray(np.moveaxis(r[:3], 0, -1))
            out["direction"] = np.ascontiguousarray(np.moveaxis(r[3:], 0, -1))
        return out

    def render_gbuffer_async(self, cam, W, H, tw, th, d_tiles, n_tiles, prim=0, dist=0, pos=0, norm=0, col=0,
                             flags=0, d_rays=0, stream=0, d_sample_map=0):
        """Tile-list G-buffer launch with device buffers (raw device addresses, 0 = NULL): n =
        n_tiles * tw * th records at render_tiles_async's pixel offsets; d_rays: 6 planes of n floats.
        d_sample_map: the sampled frame's W x H uint8 map on the device (wgt_render_gbuffer_sampled_async)."""
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        bufs = _device_hit_buffers(prim, dist, pos, norm, col, flags)
        if d_sample_map:
            self._check(self._L.wgt_render_gbuffer_sampled_async(
                self.h, ptr(cam), W, H, tw, th, ctypes.c_void_p(d_tiles), n_tiles, ctypes.c_void_p(d_sample_map),
                ctypes.byref(bufs), ctypes.c_void_p(d_rays or None), ctypes.c_void_p(stream or None)))
            return
        self._check(self._L.wgt_render_gbuffer_async(self.h, ptr(cam), W, H, tw, th, ctypes.c_void_p(d_tiles),
                                                     n_tiles, ctypes.byref(bufs), ctypes.c_void_p(d_rays or None),
                                                     ctypes.c_void_p(stream or None)))

    @staticmethod
    def _denoise_params(iterations, normal_power, sigma_pos, demodulate):
        """wgt_denoise_params: the library's defaults, with the arguments that are not None over them."""
        p = denoise_defaults()
        if iterations is not None:
            p.iterations = iterations
        if normal_power is not None:
            p.normal_power = normal_power
        if sigma_pos is not None:
            p.sigma_pos = sigma_pos
        p.flags = _lib.WGT_DENOISE_DEMODULATE if demodulate else 0
        return p

    def denoise(self, color, guides, iterations=None, normal_power=None, sigma_pos=None, demodulate=True,
                want=("f32", "u8")):
        """Edge-avoiding a-trous filter (wgt_denoise) of `color`, the (H, W, 4) float32 radiance of
        render_tile, guided by `guides`, the dict render_gbuffer returns for the same pixels (prim, pos,
        norm, col and flags are read).  None for a parameter takes the library's default (5 iterations,
        normal_power 7, sigma_pos 1.0).  Returns {"f32": (H, W, 4) float32, "u8": (H, W, 4) uint8}, None
        for an output not in `want`.  Lights, misses and non-finite pixels pass through unchanged."""
        color = np.ascontiguousarray(color, np.float32)
        if color.ndim != 3 or color.shape[2] != 4:
            raise ValueError(f"denoise: color must be (H, W, 4), got {color.shape}")
        H, W = color.shape[:2]
        missing = [k for k in ("prim", "pos", "norm", "col", "flags") if guides.get(k) is None]
        if missing:
            raise ValueError(f"denoise: guides lack {missing}")
        planar = {k: np.ascontiguousarray(np.moveaxis(np.asarray(guides[k], np.float32).reshape(H, W, 3), -1, 0))
                  for k in ("pos", "norm", "col")}
        planar["prim"] = np.ascontiguousarray(guides["prim"], np.uint32).reshape(H, W)
        planar["flags"] = np.ascontiguousarray(guides["flags"], np.uint8).reshape(H, W)
        bufs = WgtHitBuffers(**{k: a.ctypes.data for k, a in planar.items()})
        f32 = np.zeros((H, W, 4), np.float32) if "f32" in want else None
        u8 = np.zeros((H, W, 4), np.uint8) if "u8" in want else None
        p = self._denoise_params(iterations, normal_power, sigma_pos, demodulate)
        self._check(self._L.wgt_denoise(self.h, ctypes.byref(p), W, H, ptr(color), ctypes.byref(bufs), ptr(f32),
                                        ptr(u8)))
        return {"f32": f32, "u8": u8}

    def denoise_async(self, W, H, d_f32_in, d_workspace, workspace_bytes, prim=0, pos=0, norm=0, col=0, flags=0,
                      d_f32_out=0, d_u8_out=0, iterations=None, normal_power=None, sigma_pos=None, demodulate=True,
                      stream=0):
        """Device-pointer launch (wgt_denoise_async; raw device addresses, 0 = NULL): the W x H rgba32f
        image at d_f32_in, the G-buffer planes of render_gbuffer_async's single full-frame tile, a
        workspace of denoise_workspace_bytes(W, H) bytes that is the caller's, and the outputs, of
        which d_f32_out may equal d_f32_in.  Ordered on `stream` (0 = the context's)."""
        bufs = _device_hit_buffers(prim, 0, pos, norm, col, flags)
        p = self._denoise_params(iterations, normal_power, sigma_pos, demodulate)
        self._check(self._L.wgt_denoise_async(self.h, ctypes.byref(p), W, H, ctypes.c_void_p(d_f32_in or None),
                                              ctypes.byref(bufs), ctypes.c_void_p(d_workspace or None),
                                              workspace_bytes, ctypes.c_void_p(d_f32_out or None),
                                              ctypes.c_void_p(d_u8_out or None), ctypes.c_void_p(stream or None)))

    @staticmethod
    def _temporal_params(max_history, normal_min, plane_tol, match_prim):
        """wgt_temporal_params: the library's defaults, with the arguments that are not None over them."""
        p = temporal_defaults()
        if max_history is not None:
            p.max_history = max_history
        if normal_min is not None:
            p.normal_min = normal_min
        if plane_tol is not None:
            p.plane_tol = plane_tol
        p.flags = _lib.WGT_TEMPORAL_MATCH_PRIM if match_prim else 0
        return p

    @staticmethod
    def _temporal_guides(guides, H, W, what):
        """The planar host arrays wgt_temporal_accumulate reads of a render_gbuffer dict, and their struct."""
        missing = [k for k in ("prim", "pos", "norm", "flags") if guides.get(k) is None]
        if missing:
            raise ValueError(f"temporal_accumulate: {what} lack {missing}")
        planar = {k: np.ascontiguousarray(np.moveaxis(np.asarray(guides[k], np.float32).reshape(H, W, 3), -1, 0))
                  for k in ("pos", "norm")}
        planar["prim"] = np.ascontiguousarray(guides["prim"], np.uint32).reshape(H, W)
        planar["flags"] = np.ascontiguousarray(guides["flags"], np.uint8).reshape(H, W)
        return planar, WgtHitBuffers(**{k: a.ctypes.data for k, a in planar.items()})

    def temporal_accumulate(self, color, guides, cam, prev=None, guides_prev=None, cam_prev=None, max_history=None,
                            normal_min=None, plane_tol=None, match_prim=False, moments=True, want=("u8",)):
        """Temporal accumulation by reprojection (wgt_temporal_accumulate) of `color`, the (H, W, 4) float32
        radiance of render_tile, with `guides`, the dict render_gbuffer returns for the same pixels
        (prim, pos, norm and flags are read), rendered with `cam`.  prev: the dict the previous frame's
        call returned, guides_prev and cam_prev that frame's G-buffer and camera; all three None is the
        first frame.  None for a parameter takes the library's default (max_history 32, normal_min 0.9,
        plane_tol 1.0).  Returns {"f32": (H, W, 4) float32, "len": (H, W) float32, "moments": (2, H, W)
        float32 or None (moments=False), "u8": (H, W, 4) uint8 or None ("u8" not in want)}.  Lights,
        misses and non-finite pixels pass through unchanged with len 0."""
        return self._temporal_accumulate(False, None, color, guides, cam, prev, guides_prev, cam_prev, max_history,
                                         normal_min, plane_tol, match_prim, moments, want)

    def _temporal_accumulate(self, motion_form, motion, color, guides, cam, prev, guides_prev, cam_prev, max_history,
                             normal_min, plane_tol, match_prim, moments, want):
        """temporal_accumulate and temporal_accumulate_motion (motion_form: `motion` is passed on)."""
        color = np.ascontiguousarray(color, np.float32)
        if color.ndim != 3 or color.shape[2] != 4:
            raise ValueError(f"temporal_accumulate: color must be (H, W, 4), got {color.shape}")
        H, W = color.shape[:2]
        keep, bufs = self._temporal_guides(guides, H, W, "guides")
        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        out = {"f32": np.zeros((H, W, 4), np.float32), "len": np.zeros((H, W), np.float32),
               "moments": np.zeros((2, H, W), np.float32) if moments else None,
               "u8": np.zeros((H, W, 4), np.uint8) if "u8" in want else None}
        st_out = WgtTemporalState(out["f32"].ctypes.data, out["len"].ctypes.data,
                                  out["moments"].ctypes.data if moments else None)
        p_prev = p_gprev = p_cam_prev = None
        if prev is not None or guides_prev is not None or cam_prev is not None:
            # an incomplete triple reaches the library, which refuses it
            if prev is not None:
                # moments=False: a previous state's moments are not carried on
                pa = {k: np.ascontiguousarray(prev[k], np.float32)
                      if prev.get(k) is not None and (moments or k != "moments") else None
                      for k in ("f32", "len", "moments")}
                for k, size in (("f32", 4 * H * W), ("len", H * W), ("moments", 2 * H * W)):
                    if pa[k] is not None and pa[k].size != size:
                        raise ValueError(f"temporal_accumulate: prev[{k!r}] has {pa[k].size} elements, not {size}")
                st_prev = WgtTemporalState(*(pa[k].ctypes.data if pa[k] is not None else None
                                             for k in ("f32", "len", "moments")))
                p_prev = ctypes.byref(st_prev)
            if guides_prev is not None:
                keep_prev, bufs_prev = self._temporal_guides(guides_prev, H, W, "guides_prev")
                p_gprev = ctypes.byref(bufs_prev)
            if cam_prev is not None:
                cam_prev = np.ascontiguousarray(cam_prev, CAMERA_DTYPE)
                p_cam_prev = ptr(cam_prev)
        p = self._temporal_params(max_history, normal_min, plane_tol, match_prim)
        if motion_form:
            p_motion = None
            if motion is not None:
                missing = [k for k in ("pos_prev", "norm_prev") if motion.get(k) is None]
                if missing:
                    raise ValueError(f"temporal_accumulate_motion: motion lacks {missing}")
                mp = {k: np.ascontiguousarray(np.moveaxis(np.asarray(motion[k], np.float32).reshape(H, W, 3), -1, 0))
                      for k in ("pos_prev", "norm_prev")}
                mb = WgtMotionBuffers(mp["pos_prev"].ctypes.data, mp["norm_prev"].ctypes.data)
                p_motion = ctypes.byref(mb)
            self._check(self._L.wgt_temporal_accumulate_motion(self.h, ctypes.byref(p), W, H, ptr(cam), p_cam_prev,
                                                               ptr(color), ctypes.byref(bufs), p_motion, p_prev, p_gprev,
                                                               ctypes.byref(st_out), ptr(out["u8"])))
            return out
        self._check(self._L.wgt_temporal_accumulate(self.h, ctypes.byref(p), W, H, ptr(cam), p_cam_prev, ptr(color),
                                                    ctypes.byref(bufs), p_prev, p_gprev, ctypes.byref(st_out),
                                                    ptr(out["u8"])))
        return out

    def temporal_accumulate_motion(self, color, guides, cam, motion=None, prev=None, guides_prev=None, cam_prev=None,
                                   max_history=None, normal_min=None, plane_tol=None, match_prim=False, moments=True,
                                   want=("u8",)):
        """temporal_accumulate with a history that follows moved triangles (wgt_temporal_accumulate_motion):
        `motion` is the dict motion_reproject returned for `guides` ({"pos_prev", "norm_prev"}, (H, W, 3)
        each), required when prev is set and ignored on the first frame.  Everything else, the returned
        state included, is temporal_accumulate's."""
        return self._temporal_accumulate(True, motion, color, guides, cam, prev, guides_prev, cam_prev, max_history,
                                         normal_min, plane_tol, match_prim, moments, want)

    def motion_snapshot(self, stream=0):
        """Keep a copy of the resident triangles as they are now (wgt_motion_snapshot), to be taken before
        an update: motion_reproject then tells where each hit lay before it.  Returns once queued on
        `stream` (0 = the context's)."""
        self._check(self._L.wgt_motion_snapshot(self.h, ctypes.c_void_p(stream or None)))

    def motion_snapshot_read(self):
        """Diagnostic (wgt_motion_snapshot_read): the snapshot as (n_tris, 12) float32, v0, e1, e2 and the
        face normal of each triangle in original order."""
        n = self.scene_info()["n_tris"]
        out = np.zeros((n, 12), np.float32)
        self._check(self._L.wgt_motion_snapshot_read(self.h, ptr(out), n))
        return out

    def motion_reproject(self, guides):
        """Where each hit lay before the update since the last snapshot (wgt_motion_reproject).  guides: a
        dict as render_gbuffer or trace_hits returns it (prim, pos, norm and flags are read), of any
        leading shape.  Returns {"pos_prev", "norm_prev"} shaped as guides["pos"]."""
        missing = [k for k in ("prim", "pos", "norm", "flags") if guides.get(k) is None]
        if missing:
            raise ValueError(f"motion_reproject: guides lack {missing}")
        shape = np.asarray(guides["pos"]).shape
        prim = np.ascontiguousarray(guides["prim"], np.uint32).reshape(-1)
        n = prim.size
        flags = np.ascontiguousarray(guides["flags"], np.uint8).reshape(-1)
        planar = {k: np.ascontiguousarray(np.asarray(guides[k], np.float32).reshape(n, 3).T) for k in ("pos", "norm")}
        bufs = WgtHitBuffers(prim=prim.ctypes.data, pos=planar["pos"].ctypes.data, norm=planar["norm"].ctypes.data,
                             flags=flags.ctypes.data)
        out = {k: np.zeros((3, n), np.float32) for k in ("pos_prev", "norm_prev")}
        mb = WgtMotionBuffers(out["pos_prev"].ctypes.data, out["norm_prev"].ctypes.data)
        self._check(self._L.wgt_motion_reproject(self.h, n, ctypes.byref(bufs), ctypes.byref(mb)))
        return {k: np.ascontiguousarray(a.T).reshape(shape) for k, a in out.items()}

    def motion_reproject_async(self, n, guides, pos_prev, norm_prev, stream=0):
        """Device-pointer launch (wgt_motion_reproject_async; raw device addresses): guides, a dict of the
        planes' addresses (prim, pos, norm, flags) of n records; pos_prev and norm_prev receive 3 planes
        of n floats each.  Ordered on `stream` (0 = the context's)."""
        bufs = _device_hit_buffers(guides.get("prim"), 0, guides.get("pos"), guides.get("norm"), 0, guides.get("flags"))
        mb = WgtMotionBuffers(pos_prev or None, norm_prev or None)
        self._check(self._L.wgt_motion_reproject_async(self.h, n, ctypes.byref(bufs), ctypes.byref(mb),
                                                       ctypes.c_void_p(stream or None)))

    def temporal_accumulate_motion_async(self, W, H, cam, d_f32_in, guides, out, motion=None, prev=None,
                                         guides_prev=None, cam_prev=None, d_u8_out=0, max_history=None,
                                         normal_min=None, plane_tol=None, match_prim=False, stream=0):
        """temporal_accumulate_async with a history that follows moved triangles
        (wgt_temporal_accumulate_motion_async): motion, a dict {"pos_prev", "norm_prev"} of the addresses
        motion_reproject_async wrote for `guides`, required when prev is set."""
        self.temporal_accumulate_async(W, H, cam, d_f32_in, guides, out, prev, guides_prev, cam_prev, d_u8_out,
                                       max_history, normal_min, plane_tol, match_prim, stream, _motion=(motion,))

    def temporal_accumulate_async(self, W, H, cam, d_f32_in, guides, out, prev=None, guides_prev=None, cam_prev=None,
                                  d_u8_out=0, max_history=None, normal_min=None, plane_tol=None, match_prim=False,
                                  stream=0, _motion=None):
        """Device-pointer launch (wgt_temporal_accumulate_async; raw device addresses, 0 = NULL): the W x H
        rgba32f image at d_f32_in; guides and guides_prev: dicts of the G-buffer planes' addresses
        (prim, pos, norm, flags) of render_gbuffer_async's single full-frame tile; out and prev: dicts
        {"f32", "len", "moments"} of addresses, the caller's two state sets (moments 0 or absent in
        both: not kept).  prev, guides_prev and cam_prev all None is the first frame.  out["f32"] may
        equal d_f32_in.  Ordered on `stream` (0 = the context's)."""
        def state(d):
            return WgtTemporalState(*(d.get(k) or None for k in ("f32", "len", "moments")))

        def hits(d):
            return _device_hit_buffers(d.get("prim"), 0, d.get("pos"), d.get("norm"), 0, d.get("flags"))

        cam = np.ascontiguousarray(cam, CAMERA_DTYPE)
        bufs, st_out = hits(guides), state(out)
        p_prev = p_gprev = p_cam_prev = None
        if prev is not None:
            st_prev = state(prev)
            p_prev = ctypes.byref(st_prev)
        if guides_prev is not None:
            bufs_prev = hits(guides_prev)
            p_gprev = ctypes.byref(bufs_prev)
        if cam_prev is not None:
            cam_prev = np.ascontiguousarray(cam_prev, CAMERA_DTYPE)
            p_cam_prev = ptr(cam_prev)
        p = self._temporal_params(max_history, normal_min, plane_tol, match_prim)
        if _motion is not None:  # the motion form: (motion,)
            p_motion = None
            if _motion[0] is not None:
                mb = WgtMotionBuffers(_motion[0].get("pos_prev") or None, _motion[0].get("norm_prev") or None)
                p_motion = ctypes.byref(mb)
            self._check(self._L.wgt_temporal_accumulate_motion_async(
                self.h, ctypes.byref(p), W, H, ptr(cam), p_cam_prev, ctypes.c_void_p(d_f32_in or None), ctypes.byref(bufs),
                p_motion, p_prev, p_gprev, ctypes.byref(st_out), ctypes.c_void_p(d_u8_out or None),
                ctypes.c_void_p(stream or None)))
            return
        self._check(self._L.wgt_temporal_accumulate_async(self.h, ctypes.byref(p), W, H, ptr(cam), p_cam_prev,
                                                          ctypes.c_void_p(d_f32_in or None), ctypes.byref(bufs), p_prev,
                                                          p_gprev, ctypes.byref(st_out),
                                                          ctypes.c_void_p(d_u8_out or None),
                                                          ctypes.c_void_p(stream or None)))

    @staticmethod
    def _denoise_variance_params(iterations, normal_power, sigma_pos, sigma_lum, min_history, demodulate):
        """wgt_denoise_variance_params: the library's defaults, with the arguments that are not None over them."""
        p = denoise_variance_defaults()
        for name, value in (("iterations", iterations), ("normal_power", normal_power), ("sigma_pos", sigma_pos),
                            ("sigma_lum", sigma_lum), ("min_history", min_history)):
            if value is not None:
                setattr(p, name, value)
        p.flags = _lib.WGT_DENOISE_DEMODULATE if demodulate else 0
        return p

    def denoise_variance(self, state, guides, iterations=None, normal_power=None, sigma_pos=None, sigma_lum=None,
                         min_history=None, demodulate=True, want=("f32", "u8")):
        """Variance-guided a-trous filter (wgt_denoise_variance) of `state`, the dict temporal_accumulate
        returns (its "f32", "len" and "moments" are read), guided by `guides`, the dict render_gbuffer
        returns for the same pixels (prim, pos, norm, col and flags are read).  None for a parameter
        takes the library's default (5 iterations, normal_power 7, sigma_pos 1.0, sigma_lum 4.0,
        min_history 4).  Returns {"f32": (H, W, 4) float32, "u8": (H, W, 4) uint8, "var": (H, W) float32,
        the filtered variance of the demodulated luminance}, None for an output not in `want`.  Lights,
        misses, non-finite pixels and pixels without history pass through unchanged, with variance 0."""
        missing = [k for k in ("f32", "len", "moments") if state.get(k) is None]
        if missing:
            raise ValueError(f"denoise_variance: state lacks {missing}")
        color = np.ascontiguousarray(state["f32"], np.float32)
        if color.ndim != 3 or color.shape[2] != 4:
            raise ValueError(f"denoise_variance: state['f32'] must be (H, W, 4), got {color.shape}")
        H, W = color.shape[:2]
        length = np.ascontiguousarray(state["len"], np.float32)
        moments = np.ascontiguousarray(state["moments"], np.float32)
        for k, a, size in (("len", length, H * W), ("moments", moments, 2 * H * W)):
            if a.size != size:
                raise ValueError(f"denoise_variance: state[{k!r}] has {a.size} elements, not {size}")
        missing = [k for k in ("prim", "pos", "norm", "col", "flags") if guides.get(k) is None]
        if missing:
            raise ValueError(f"denoise_variance: guides lack {missing}")
        planar = {k: np.ascontiguousarray(np.moveaxis(np.asarray(guides[k], np.float32).reshape(H, W, 3), -1, 0))
                  for k in ("pos", "norm", "col")}
        planar["prim"] = np.ascontiguousarray(guides["prim"], np.uint32).reshape(H, W)
        planar["flags"] = np.ascontiguousarray(guides["flags"], np.uint8).reshape(H, W)
        bufs = WgtHitBuffers(**{k: a.ctypes.data for k, a in planar.items()})
        st = WgtTemporalState(color.ctypes.data, length.ctypes.data, moments.ctypes.data)
        f32 = np.zeros((H, W, 4), np.float32) if "f32" in want else None
        u8 = np.zeros((H, W, 4), np.uint8) if "u8" in want else None
        var = np.zeros((H, W), np.float32) if "var" in want else None
        p = self._denoise_variance_params(iterations, normal_power, sigma_pos, sigma_lum, min_history, demodulate)
        self._check(self._L.wgt_denoise_variance(self.h, ctypes.byref(p), W, H, ctypes.byref(st), ctypes.byref(bufs),
                                                 ptr(f32), ptr(u8), ptr(var)))
        return {"f32": f32, "u8": u8, "var": var}

    def denoise_variance_async(self, W, H, state, d_workspace, workspace_bytes, prim=0, pos=0, norm=0, col=0, flags=0,
                               d_f32_out=0, d_u8_out=0, d_var_out=0, iterations=None, normal_power=None,
                               sigma_pos=None, sigma_lum=None, min_history=None, demodulate=True, stream=0):
        """Device-pointer launch (wgt_denoise_variance_async; raw device addresses, 0 = NULL): `state`, a
        dict {"f32", "len", "moments"} of addresses as temporal_accumulate_async's `out`, the G-buffer
        planes of render_gbuffer_async's single full-frame tile, a workspace of
        denoise_variance_workspace_bytes(W, H) bytes that is the caller's, and the outputs, of which
        d_f32_out may equal state["f32"].  Ordered on `stream` (0 = the context's)."""
        st = WgtTemporalState(*(state.get(k) or None for k in ("f32", "len", "moments")))
        bufs = _device_hit_buffers(prim, 0, pos, norm, col, flags)
        p = self._denoise_variance_params(iterations, normal_power, sigma_pos, sigma_lum, min_history, demodulate)
        self._check(self._L.wgt_denoise_variance_async(self.h, ctypes.byref(p), W, H, ctypes.byref(st),
                                                       ctypes.byref(bufs), ctypes.c_void_p(d_workspace or None),
                                                       workspace_bytes, ctypes.c_void_p(d_f32_out or None),
                                                       ctypes.c_void_p(d_u8_out or None),
                                                       ctypes.c_void_p(d_var_out or None),
                                                       ctypes.c_void_p(stream or None)))

    @staticmethod
    def _sample_plan_params(params):
        """wgt_sample_plan_params: the library's defaults, with the keyword arguments given over them."""
        p = sample_plan_defaults()
        names = [n for n, _ in p._fields_]
        for name, value in params.items():
            if name not in names:
                raise TypeError(f"sample_plan: unknown parameter {name!r}; choose from {names}")
            if value is not None:
                setattr(p, name, value)
        return p

    def sample_plan(self, state, **params):
        """The next frame's sample map (wgt_sample_plan) from `state`, the dict temporal_accumulate
        returns (its "len" and "moments" are read).  Keyword parameters: side_min, side_max, gain,
        lum_floor, min_history, dilate, budget_spp (the library's defaults otherwise).  Returns
        {"map": (H, W) uint8, "total": int}, total = the map's sum of squares."""
        missing = [k for k in ("len", "moments") if state.get(k) is None]
        if missing:
            raise ValueError(f"sample_plan: state lacks {missing}")
        length = np.ascontiguousarray(state["len"], np.float32)
        if length.ndim != 2:
            raise ValueError(f"sample_plan: state['len'] must be (H, W), got {length.shape}")
        H, W = length.shape
        moments = np.ascontiguousarray(state["moments"], np.float32)
        if moments.size != 2 * H * W:
            raise ValueError(f"sample_plan: state['moments'] has {moments.size} elements, not {2 * H * W}")
        st = WgtTemporalState(None, length.ctypes.data, moments.ctypes.data)
        out = np.zeros((H, W), np.uint8)
        total = ctypes.c_uint64(0)
        p = self._sample_plan_params(params)
        self._check(self._L.wgt_sample_plan(self.h, ctypes.byref(p), W, H, ctypes.byref(st), ptr(out),
                                            ctypes.byref(total)))
        return {"map": out, "total": int(total.value)}

    def sample_plan_async(self, W, H, state, d_workspace, workspace_bytes, d_map_out, d_total_out=0, stream=0, **params):
        """Device-pointer launch (wgt_sample_plan_async; raw device addresses, 0 = NULL): `state`, a dict
        {"len", "moments"} of addresses as temporal_accumulate_async's `out`, a workspace of
        sample_plan_workspace_bytes(W, H) bytes that is the caller's, the W x H uint8 map and
        (optionally) its uint64 total.  Ordered on `stream` (0 = the context's)."""
        st = WgtTemporalState(None, state.get("len") or None, state.get("moments") or None)
        p = self._sample_plan_params(params)
        self._check(self._L.wgt_sample_plan_async(self.h, ctypes.byref(p), W, H, ctypes.byref(st),
                                                  ctypes.c_void_p(d_workspace or None), workspace_bytes,
                                                  ctypes.c_void_p(d_map_out or None),
                                                  ctypes.c_void_p(d_total_out or None),
                                                  ctypes.c_void_p(stream or None)))

    def stream(self) -> int:
        return self._L.wgt_stream(self.h) or 0

    def pipeline_stream(self, i: int) -> int:
        """The context's i-th pipeline stream (own hardware queue; frames issued round-robin overlap)."""
        s = self._L.wgt_pipeline_stream(self.h, i)
        if not s:
            raise WgtError(WGT_E_HIP, (self._L.wgt_last_error(self.h) or b"").decode())
        return s

    def sync(self):
        self._check(self._L.wgt_sync(self.h))

    def selftest_math(self, n: int, seed: int = 1):
        """-> dict of wgt_selftest_math's counts (include/wgt_api.h)."""
        counts = np.zeros(8, np.uint64)
        self._check(self._L.wgt_selftest_math(self.h, n, seed, counts.ctypes.data_as(ctypes.c_void_p)))
        keys = ("sqrt_tests", "sqrt_rn_bad", "div_tests", "div_rn_bad", "sqrt_fast_tests", "sqrt_fast_bad",
                "compiler_sqrt_bad", "compiler_div_bad")
        return dict(zip(keys, (int(c) for c in counts)))


def tile_grid(W: int, H: int, T: int, seed: int = 0, frame: int = 0):
    """All T x T tiles of a W x H frame, row-major (x0, y0, seed, frame)."""
    ys, xs = np.meshgrid(np.arange(0, H, T, dtype=np.uint32), np.arange(0, W, T, dtype=np.uint32), indexing="ij")
    tiles = np.zeros(xs.size, TILE_DTYPE)
    tiles["x0"] = xs.ravel()
    tiles["y0"] = ys.ravel()
    tiles["seed"] = seed & 0xFFFFFFFF
    tiles["frame"] = frame
    return tiles
