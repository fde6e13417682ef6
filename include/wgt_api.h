/*
 * wgt_api.h — C-ABI of the MI355X-native path-tracing hot path (libwgt.so).
 *
 * This is the drop-in boundary that replaces the WebGPU compute dispatch of the
 * reference (kugimasa/WebGPUTracer):
 *
 *   reference                                         replaced by
 *   ----------------------------------------------    -------------------------------
 *   Renderer::InitDevice  render.cpp:49-147           wgt_create
 *   Scene::InitBuffers    scene.cpp:161-165           wgt_upload_scene (+ BVH build)
 *     CreateQuadBuffer    scene.cpp:223-271             same 96-B quad records
 *     CreateSphereBuffer  scene.cpp:276-306             same 32-B sphere records
 *     CreateTriangleBuffer scene.cpp:170-218            same 80-B triangle records
 *   Camera::Update        camera.cpp:64-70            wgt_camera_param (48 B, same layout)
 *   OnRender compute pass render.cpp:461-491          wgt_render_tile / wgt_render_tiles_async
 *     dispatchWorkgroups  render.cpp:477-484            one HIP launch
 *   saveTexture readback  save_texture.h:10-87        rgba8 output (+ wgt_write_png)
 *   Scene::Release / OnFinish scene.cpp:41-50         wgt_destroy
 *   Error(...) / callbacks render.cpp:120-133         int status + wgt_last_error
 *   sample_hit            path_tracer.wgsl:290-310    wgt_trace_rays (closest-hit query)
 *   (none: sample_hit's dist < a limit)               wgt_occluded_rays (any-hit query)
 *   HitInfo after sample_hit path_tracer.wgsl:27-36   wgt_trace_hits (the whole hit record)
 *   (none: HitInfo of a pixel's first camera ray)     wgt_render_gbuffer (first-hit G-buffer)
 *   (none: history reprojected frame to frame)        wgt_temporal_accumulate (temporal accumulation)
 *   (none: history that follows a moved mesh)         wgt_motion_snapshot, wgt_motion_reproject,
 *                                                     wgt_temporal_accumulate_motion
 *   camera.spp, one per frame path_tracer.wgsl:23     wgt_render_tile_sampled, ..._tiles_sampled_async,
 *                                                     wgt_render_gbuffer_sampled (a side per pixel)
 *   (none: the sides planned from the variance)       wgt_sample_plan
 *   Scene::InitBuffers again, for a changed mesh      wgt_rebuild_triangles, wgt_rebuild_triangles_device
 *                                                     (a new BVH made on the device, any triangle count)
 *   (none: the triangle nearest to a point)           wgt_nearest_points (closest-point query)
 *   raytrace loop of compute_sample :386-393          wgt_trace_radiance (a path per caller ray and RNG state)
 *   (none: every surface along a ray)                 wgt_trace_multi_hits (the k nearest hits, the hit count)
 *   (none: the triangles within a radius of a point)  wgt_nearest_k_points (the k nearest, their number)
 *   (none: the triangles a triangle cuts)             wgt_overlap_triangles (whether, how many, which)
 *   (none: the triangles a mesh's own triangles cut)  wgt_overlap_self (the same, neighbours by index excluded)
 *
 * Conventions: every call returns 0 on success or a negative WGT_E_* code; the
 * message is available from wgt_last_error(ctx) (per-context, or thread-local
 * for calls without a context).  No exceptions cross the ABI.  Host arrays are
 * borrowed for the duration of the call.  "_async" entry points take device
 * pointers and a hipStream_t passed as void* (NULL = the context's stream) and
 * return immediately; everything else is synchronous.  All structs are POD,
 * little-endian, with exactly the reference GPU buffer layouts.
 */
#ifndef WGT_API_H
#define WGT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WGT_API_VERSION 2  /* 2: the 64-B and wide node forms removed (scene info fields) */

enum {
  WGT_OK = 0,
  WGT_E_INVALID = -1,  /* bad argument / shape */
  WGT_E_HIP = -2,      /* a HIP runtime call failed */
  WGT_E_NOSCENE = -3,  /* render before wgt_upload_scene */
  WGT_E_IO = -4,       /* file could not be read/written/parsed */
  WGT_E_NOMEM = -5     /* host or device allocation failed */
};

/* 96 B — path_tracer.wgsl:50-59 <-> Scene::CreateQuadBuffer scene.cpp:223-271 */
typedef struct {
  float pos[4];   /* q.xyz, 1.0 */
  float right[4]; /* right.xyz, 1.0 */
  float up[4];    /* up.xyz, 1.0 */
  float norm[4];  /* normalize(cross(right, up)).xyz, 1.0 */
  float w[3];     /* n / dot(n, n) */
  float d;        /* dot(norm, q) */
  float col[3];
  float emissive; /* 1.0 or 0.0 */
} wgt_quad;

/* 32 B — path_tracer.wgsl:61-66 <-> Scene::CreateSphereBuffer scene.cpp:276-306 */
typedef struct {
  float center[3];
  float radius;
  float col[3];
  float emissive;
} wgt_sphere;

/* 80 B — Scene::CreateTriangleBuffer scene.cpp:170-218 (tri_stride_ = 80, scene.h:45) */
typedef struct {
  float v0[4];        /* v0.xyz, 1.0 */
  float e1[4];        /* v1 - v0, 1.0 */
  float e2[4];        /* v2 - v0, 1.0 */
  float face_norm[4]; /* normalize(cross(e1, e2)), 1.0 */
  float col[3];
  float emissive;
} wgt_triangle;

/* 48 B — Camera::CameraParam camera.h:19-31 <-> path_tracer.wgsl:17-24 */
typedef struct {
  float origin[3];
  float pad0;
  float target[3];
  float pad1;
  float aspect;
  float fovy; /* degrees */
  uint32_t spp;
  uint32_t seed;
} wgt_camera_param;

/* One tile of a frame for the tile-list launch.  The camera seed is per tile so
 * one launch can cover tiles of several frames (seed = frame index). */
typedef struct {
  uint32_t x0, y0; /* tile origin in global pixel coordinates */
  uint32_t seed;   /* camera.seed for this tile's frame */
  uint32_t frame;  /* caller's frame tag (not used by the kernel) */
} wgt_tile;

/* Counters from a render (filled when a stats pointer is given; counting runs a
 * separate instrumented launch so the timed launch carries no atomics). */
typedef struct {
  uint64_t queries;      /* reference sample_hit calls (path_tracer.wgsl:266), incl. skipped */
  uint64_t traced_rays;  /* closest-hit queries actually traced (non-NaN rays) */
  uint64_t samples;      /* camera paths */
  uint64_t nan_rays;     /* queries on NaN rays (resolved without tracing) */
  uint64_t node_visits;  /* BVH nodes fetched */
  uint64_t tri_tests;    /* Moller-Trumbore tests */
  uint64_t pixels;
  /* SIMT efficiency: iterations of the per-lane path loop / BVH loop counted once
   * per wave (wave_*) and once per active lane (lane_*); lane/(64*wave) = utilisation */
  uint64_t loop_wave_iters, loop_lane_iters, trav_wave_steps, trav_lane_steps;
  /* phase-split kernel: wave cycles (s_memtime) in the service / traversal phase */
  uint64_t cyc_service, cyc_trav;
  float kernel_ms;       /* hipEvent time of the (uninstrumented) render launch of the frame */
  float trace_ms;        /* = kernel_ms (one launch traces and shades; kept for the layout) */
  float shade_ms;        /* 0 (kept for the layout) */
  uint32_t iterations;   /* launches per frame: 1 */
  /* phase-split kernel: wave cycles of the service phase by region: pixel refill +
   * writes, finalise (quad rebuild, triangle merge, spheres), shading, camera ray +
   * NaN handling, quad scan, root-node test */
  uint64_t cyc_refill, cyc_finalise, cyc_shade, cyc_camera, cyc_quads, cyc_root;
  /* persistent kernel with parked traversal state: LDS stack overflows moved to the
   * lane's global stack, and refills from it */
  uint64_t stack_spills, stack_refills;
  /* ... and traversals ended on the global stack's overflow exit (a wrong pixel; never taken:
   * the global stack holds the builder's bound, and the parity tests assert 0) */
  uint64_t stack_overflows;
  /* traversal phase by BVH level: lane visits of nodes at levels 1-2 (the root is
   * tested in the service phase), wave cycles of node steps, of the node steps whose visiting lanes
   * are all at levels 1-2 (what an LDS copy of the top levels could shorten), and of triangle steps */
  uint64_t top_node_visits, cyc_node_steps, cyc_top_steps, cyc_tri_steps;
  /* rays whose quad scan took the reference path with per-quad distances (an almost-tie in
   * distance between two quads) */
  uint64_t quad_ref_scans;
} wgt_stats;

typedef struct {
  uint32_t n_lights, n_quads, n_spheres, n_tris;
  uint32_t bvh_nodes, bvh_leaves, bvh_max_depth, bvh_max_leaf; /* the traversed (BVH4) tree */
  uint64_t device_bytes; /* scene bytes resident in HBM */
  double sah_cost;       /* of the SAH BVH2 the BVH4 is collapsed from */
  uint32_t bvh_width;    /* children per node (4) */
  uint32_t bvh_stack;    /* worst-case traversal stack entries per ray (LDS) */
  uint32_t bvh2_nodes, bvh2_depth;
  uint32_t bvh_compact;   /* 1: the tree exceeds one XCD's L2 as 128-B nodes, so the persistent
                           * kernel reads its compact form (64-B nodes + 16-B refs) by default */
  float bvh_compact_step; /* scene-wide decode step of the compact nodes (wgt_geom.h) */
  uint32_t ps_waves;      /* waves per SIMD of the persistent kernel: 6 with 3-byte stack entries
                           * when every ref of the tree fits 24 bits, else 5 */
  uint32_t ps_park;       /* 1: the persistent kernel parks its traversal state in LDS during
                           * service passes */
  uint32_t ps_stack;      /* stack entries per lane it keeps in LDS (the rest: a global stack) */
  uint32_t node_form;     /* node form of the persistent kernel for the reference camera: 0 = 128-B,
                           * 1 = 80-B compact (WGT_CNODE) */
  uint32_t ps_resident;   /* waves of the persistent grid (the device's resident capacity) */
} wgt_scene_info;

typedef struct wgt_ctx wgt_ctx;

/* ---- lifecycle ---------------------------------------------------------- */
int wgt_create(int hip_device, wgt_ctx **out);
void wgt_destroy(wgt_ctx *ctx); /* idempotent for NULL */
const char *wgt_last_error(const wgt_ctx *ctx); /* ctx may be NULL */
int wgt_version(void);
/* 16 hex digits identifying the kernel build (a hash of the HIP sources, the headers
 * they include and the compile flags): profiles key their counters by it (bench.py) */
const char *wgt_build_id(void);
int wgt_device_count(int *count);

/* ---- scene upload (replaces Scene::InitBuffers) ------------------------- */
/* n_lights >= 1 (sample_from_light reads lights[0], path_tracer.wgsl:165) and
 * n_spheres >= 1 (the reference always binds a dummy sphere, scene.cpp:31).
 * Triangles (n_tris may be 0) get a SAH BVH built on the host and uploaded as
 * SoA node/triangle arrays. */
int wgt_upload_scene(wgt_ctx *ctx, const wgt_quad *lights, uint32_t n_lights,
                     const wgt_quad *quads, uint32_t n_quads, const wgt_sphere *spheres,
                     uint32_t n_spheres, const wgt_triangle *tris, uint32_t n_tris);
int wgt_scene_info_get(const wgt_ctx *ctx, wgt_scene_info *info);
/* Host only (no device): build the BVH exactly as wgt_upload_scene does and
 * export it for inspection.  info gets the counts; nodes_out (may be NULL) gets
 * bvh_nodes x 32 floats (BVH4 layout, wgt_geom.h) if nodes_cap >= bvh_nodes;
 * tris_out (may be NULL) gets n_tris x 16 floats (leaf-ordered records).
 * Call once with NULL outputs to size them. */
int wgt_bvh_build(const wgt_triangle *tris, uint32_t n_tris, float *nodes_out, uint32_t nodes_cap,
                  float *tris_out, wgt_scene_info *info);
/* Host only: the compact form of the same tree (wgt_geom.h): cnodes_out gets
 * bvh_nodes x 16 words, crefs_out bvh_nodes x 4 child refs, step_out the decode
 * step.  Both outputs are required; nodes_cap must be >= bvh_nodes. */
int wgt_bvh_build_compact(const wgt_triangle *tris, uint32_t n_tris, uint32_t *cnodes_out,
                          int32_t *crefs_out, uint32_t nodes_cap, float *step_out);

/* ---- moving the triangles of an uploaded scene (no reference counterpart) -- */
/* Synchronous: moves the scene's triangles to tris[0..n_tris) (a HOST array; triangle i keeps its
 * primitive id, and its shading fields are taken from tris[i] too) by refitting the resident BVH
 * on the device instead of rebuilding it: the tree keeps its topology, and every box, triangle
 * record and compact code is recomputed as a build computes them.  Every render and query
 * afterwards answers exactly as after wgt_upload_scene of the same scene with these triangles,
 * bit for bit: the closest hit does not depend on the tree, whose boxes only have to be
 * conservative (only wgt_stats' visit counters differ).  The tree's quality (sah_cost, which keeps
 * the build's value) degrades as the mesh deforms; a full wgt_upload_scene restores it.
 * Order of checks: WGT_E_NOSCENE before an upload; WGT_E_INVALID for NULL, for a scene without
 * triangles and for n_tris other than the uploaded count; WGT_E_INVALID for a triangle beyond the
 * scene limits (as wgt_upload_scene), which leaves the scene exactly as it was.  Then the call
 * waits for every launch of the context, as an upload does, so launches queued before it see the
 * old triangles and launches after it the new ones.
 * A WGT_E_HIP failure during the refit itself leaves the tree undefined until the next upload.
 * Out of scope: moving quads, lights and spheres (indexed quads among them); adding or removing
 * triangles; per-vertex shading data (normals, colours, texture coordinates: a triangle is shaded
 * by its face normal and one colour); any heuristic that rebuilds the tree. */
int wgt_update_triangles(wgt_ctx *ctx, const wgt_triangle *tris, uint32_t n_tris);
/* The same update from DEVICE memory, so that a mesh a simulation, a skinning kernel or a tensor
 * library moves on the device never leaves it.  Both calls are SYNCHRONOUS calls that take device
 * pointers (unlike the _async calls, which return at once): the input is read after everything
 * queued on `stream` before the call (NULL: the context's stream, a non-blocking stream that is
 * not ordered after the legacy default stream), the call then waits for every
 * launch of the context as wgt_update_triangles does, and it returns when the refit has ended, so
 * the caller may overwrite the input at once.  The input is never written.  The result is that of
 * wgt_update_triangles(ctx, T, n_tris) bit for bit (the resident tree, the scene report, every
 * later render and query), where T is
 *   wgt_update_triangles_device: the bytes of d_tris;
 *   wgt_update_vertices_device:  T[i] = wgt_make_triangles(triangle i's three vertices, col_i,
 *     emissive_i, translation = NULL), col_i and emissive_i the values triangle i was uploaded (or
 *     last updated) with: the call carries no shading input and keeps them.  As there, a -0
 *     coordinate becomes +0, and a zero-area triangle's face normal is NaN; which NaN (its sign and
 *     payload) is unspecified and may differ from the host's.
 * Order of checks, as wgt_update_triangles: NULL context; WGT_E_NOSCENE; then WGT_E_INVALID for a
 * NULL d_tris or d_verts, for a scene without triangles, for n_tris other than the uploaded count,
 * for a misaligned pointer, and for n_verts == 0 or, without indices, n_verts != 3 * n_tris.  Then
 * a pass on the device checks every triangle against the scene limits (of the vertex form the
 * record built from its vertices; an index >= n_verts is refused too, and no vertex is loaded
 * through it): WGT_E_INVALID names the lowest-numbered such triangle in wgt_update_triangles'
 * words.  A refusal leaves the scene exactly as it was.
 * The pointers themselves are not validated: memory the device cannot read is the caller's error,
 * as for every other device-pointer entry point. */
/* d_tris: DEVICE array of n_tris wgt_triangle records, 16-byte aligned. */
int wgt_update_triangles_device(wgt_ctx *ctx, const wgt_triangle *d_tris, uint32_t n_tris, void *stream);
/* d_verts: DEVICE array of n_verts x 3 floats (4-byte aligned).
 * d_index: DEVICE array of n_tris x 3 vertex indices.
 * d_index == NULL means unindexed: triangle i uses vertices 3i, 3i+1, 3i+2,
 * and n_verts must then be 3*n_tris. */
int wgt_update_vertices_device(wgt_ctx *ctx, const float *d_verts, uint32_t n_verts,
                               const uint32_t *d_index, uint32_t n_tris, void *stream);
/* Diagnostic: the last update's time in milliseconds (of any of the three calls above), split into
 * its host part, everything before the first refit kernel (checks; the staging copy of a host
 * array; of the device forms the check pass on the device and its readback), and its device part
 * (the refit kernels and two small readbacks, by hipEvents). */
int wgt_update_timing(const wgt_ctx *ctx, float *host_ms, float *device_ms);
/* Diagnostic (synchronous): copies the resident tree back in the export layouts of wgt_bvh_build
 * (nodes_out: bvh_nodes x 32 floats, tris_out: n_tris x 16 floats) and wgt_bvh_build_compact
 * (cnodes_out: bvh_nodes x 16 words, crefs_out: bvh_nodes x 4 refs, step_out), refs as indices.
 * Any output may be NULL; nodes_cap must be >= bvh_nodes for the per-node outputs. */
int wgt_bvh_read(wgt_ctx *ctx, float *nodes_out, uint32_t nodes_cap, float *tris_out,
                 uint32_t *cnodes_out, int32_t *crefs_out, float *step_out);
/* Host only: the tree that wgt_upload_scene of built_from[0..n_tris) alone followed by
 * wgt_update_triangles to now[0..n_tris) must hold, in wgt_bvh_read's layouts (any output may be
 * NULL; info is required, its sah_cost is the build's).  now is checked as the update checks it. */
int wgt_bvh_refit(const wgt_triangle *built_from, const wgt_triangle *now, uint32_t n_tris,
                  float *nodes_out, uint32_t nodes_cap, float *tris_out, uint32_t *cnodes_out,
                  int32_t *crefs_out, float *step_out, wgt_scene_info *info);

/* ---- rebuilding the triangle BVH on the device (no reference counterpart) -- */
/* Replaces the scene's triangles by n_tris >= 1 new ones and makes a new tree for them on the
 * device.  n_tris may differ from the resident count, and a scene uploaded without triangles is
 * accepted: this is how a simulation that tears, spawns or deletes triangles, or a mesh that has
 * drifted far from the pose its tree was built for, stays on the device.  The tree is an LBVH over
 * 63-bit Morton codes emitted directly as a BVH4 of at most 10 levels (DESIGN.md §4.12;
 * wgt_bvh_build_morton below is its specification); a static scene is served better by
 * wgt_upload_scene's SAH tree.
 *   - Triangle i gets primitive id n_lights + n_quads + i, so sphere ids move when the count changes.
 *   - Shading fields come from the records, as in wgt_update_triangles_device.
 *   - Afterwards every render, sampled render, G-buffer, ray query, hit record and occlusion answer
 *     equals that of wgt_upload_scene of the same quads, lights and spheres with these triangles, bit
 *     for bit.  Only wgt_stats' visit counters and the tree fields of wgt_scene_info differ: sah_cost,
 *     bvh2_nodes and bvh2_depth are 0 (no BVH2 exists), device_bytes counts what is in use.
 *   - A rebuild drops the motion snapshot, as an upload does; a later wgt_update_* refits the
 *     rebuilt tree; wgt_update_timing also reports a rebuild (the host part is everything before the
 *     first build kernel).
 *   - WGT_REBUILD_LEAF (4, 1..8) is the leaf target L.
 * Both calls are SYNCHRONOUS, with wgt_update_triangles_device's stream rule: the input is read
 * after everything queued on `stream` (NULL: the context's), the call then waits for every launch
 * of the context, and it returns when the new tree is resident.  The input is never written.
 * Order of checks: NULL context; WGT_E_NOSCENE; then WGT_E_INVALID for a NULL pointer, for
 * n_tris == 0, for n_tris above L * 4^10 ("too many triangles for a rebuild"), for a misaligned
 * device pointer (16 bytes); then the device pass of wgt_update_triangles_device names the
 * lowest-numbered triangle beyond the scene limits in wgt_update_triangles' words.  A refusal
 * leaves the scene exactly as it was, and so does a WGT_E_HIP failure: the new tree is made in a
 * second allocation and swapped in on success (the old one is kept as the spare, so a steady stream
 * of rebuilds allocates nothing). */
/* d_tris: DEVICE array of n_tris wgt_triangle records, 16-byte aligned. */
int wgt_rebuild_triangles_device(wgt_ctx *ctx, const wgt_triangle *d_tris, uint32_t n_tris, void *stream);
/* The same from a HOST array: it is staged, then the same body runs. */
int wgt_rebuild_triangles(wgt_ctx *ctx, const wgt_triangle *tris, uint32_t n_tris);
/* Host only: the tree that wgt_upload_scene of any scene whose lights, quads and spheres lie within
 * the triangles' extent, followed by a rebuild to tris[0..n_tris) alone, must hold, in wgt_bvh_read's
 * layouts (any output may be NULL; info is required).  Call once with NULL outputs to size them,
 * as wgt_bvh_refit.  tris is checked as the rebuild checks it. */
int wgt_bvh_build_morton(const wgt_triangle *tris, uint32_t n_tris, float *nodes_out, uint32_t nodes_cap,
                         float *tris_out, uint32_t *cnodes_out, int32_t *crefs_out, float *step_out,
                         wgt_scene_info *info);

/* ---- rendering (replaces the compute pass of Renderer::OnRender) --------- */
/* Synchronous: render the rectangle [x0,x0+tw) x [y0,y0+th) of a W x H frame
 * into caller-owned HOST buffers (row-major tw x th; any may be NULL):
 * rgba8_out (4 B/px, rgba8unorm store), rgba32f_out (16 B/px, radiance before
 * quantisation), hit_id_out (primitive id of sample 0's primary ray).
 * Pixel (x, y) is computed exactly as invocation (x, y) of compute_sample
 * (path_tracer.wgsl:374-398), so any tiling reproduces the full frame. */
int wgt_render_tile(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H,
                    uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, uint8_t *rgba8_out,
                    float *rgba32f_out, uint32_t *hit_id_out, wgt_stats *stats);

/* Synchronous multi-frame render (replaces Renderer::OnCompute's frame loop,
 * render.cpp:430-449, for a static scene): n_frames whole W x H frames, frame j
 * with seed seeds[j], in ONE launch (the persistent kernel's end-of-launch drain
 * is paid once per batch).  rgba8_out: n_frames x H x W x 4 bytes, frame after
 * frame.  Frame j equals wgt_render_tile of the full frame with cam->seed =
 * seeds[j], bit for bit. */
int wgt_render_frames(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H,
                      const uint32_t *seeds, uint32_t n_frames, uint8_t *rgba8_out, wgt_stats *stats);

/* Tile-list launch with DEVICE buffers: n_tiles tiles of tw x th (d_tiles: device
 * array of wgt_tile) written compactly, tile after tile (out[(t*th + ly)*tw + lx]).
 * cam->seed is ignored (per-tile seeds).  Always asynchronous: the call returns
 * as soon as the launches are queued, ordered on `stream`; read the outputs only
 * after synchronising `stream`.  The context's launches use its scheduling
 * workspaces round-robin (4 by default, WGT_WS_SLOTS = 1..4), and a launch waits
 * on the device only for the previous launch that used the same workspace: two
 * consecutive calls on different streams may run concurrently (the next frame's
 * waves fill the CUs the previous frame's end-of-launch drain leaves idle), so the
 * caller gives such calls distinct output buffers.  wgt_upload_scene
 * and wgt_destroy wait for every launch of the context before freeing what it
 * reads.
 * Consecutive launches of one view share the pixel queue's order (see "the queue order" below): a
 * device tile list is identified by its address and n_tiles, so rewriting the tiles' origins behind
 * an unchanged pointer keeps a stale order (the frames are right, only scheduled worse) until
 * wgt_order_reset or any change of view. */
int wgt_render_tiles_async(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H,
                           uint32_t tw, uint32_t th, const wgt_tile *d_tiles, uint32_t n_tiles,
                           void *d_rgba8, float *d_rgba32f, uint32_t *d_hit_id, void *stream);
/* ---- the queue order across launches of one view (diagnostics) ------------- */
/* The persistent kernel takes its 8x8 pixel blocks most expensive first, in an order made from a
 * cheap cost pre-pass.  The order depends on the view (scene, camera, frame and tile geometry, spp,
 * tuning knobs), not on the seeds, and never changes a pixel.  The first launch of a view makes an
 * order of its own as every launch did before; the second consecutive one makes the order that is
 * kept, from a pre-pass of WGT_PQ_REFINE^2 samples per pixel; every later launch of that view reads
 * it and runs neither pre-pass nor sort, until the view or the scene changes (wgt_upload_scene, the
 * wgt_update_* and wgt_rebuild_* calls).  Views that alternate or change every frame never reuse.
 * WGT_PQ_REUSE=0 turns the reuse off.  DESIGN.md §4.2. */
typedef struct {
  uint64_t today, refine, reuse; /* launches of the persistent kernel since wgt_create, by how they
                                  * got their order: their own, made and kept, reused */
  uint64_t invalidations;        /* times a kept order was dropped by a scene change or a reset */
  uint32_t nb;                   /* 8x8 blocks of the kept order, 0 when there is none */
  uint32_t refine_side;          /* side of the pre-pass that made it (samples per pixel = side^2) */
} wgt_order_stats;
int wgt_order_info(const wgt_ctx *ctx, wgt_order_stats *out);
/* Synchronous: copies the kept order, a permutation of [0, nb), to perm_out[0..cap) and sets
 * *n_out = nb; *n_out = 0 (and nothing copied) when there is none.  WGT_E_INVALID for cap < nb. */
int wgt_order_read(wgt_ctx *ctx, uint32_t *perm_out, uint32_t cap, uint32_t *n_out);
/* Drops the kept order: the next launch counts as the first of its view.  For a caller that
 * rewrites tile origins behind an unchanged device pointer. */
int wgt_order_reset(wgt_ctx *ctx);

/* Timing pass for the same launch: uninstrumented kernels with a hipEvent pair per
 * launch; fills kernel_ms / trace_ms / shade_ms / iterations (synchronous). */
int wgt_render_tiles_profile(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H,
                             uint32_t tw, uint32_t th, const wgt_tile *d_tiles, uint32_t n_tiles,
                             wgt_stats *stats);
/* Counting pass for the same launch (instrumented kernel; synchronous). */
int wgt_render_tiles_stats(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H,
                           uint32_t tw, uint32_t th, const wgt_tile *d_tiles, uint32_t n_tiles,
                           wgt_stats *stats);

/* ---- rendering with a per-pixel sample count ------------------------------- */
/* A sample map is one uint8_t per pixel of the full W x H frame, row-major, indexed by global pixel
 * coordinates (so any tiling reproduces the frame).  Value k is the side of the pixel's sample grid:
 * pixel (x, y) is computed exactly as invocation (x, y) of compute_sample with camera.spp = k * k, and
 * a uniform map of k equals wgt_render_tile at spp = k * k bit for bit.  k = 0 gives a black pixel with
 * hit id 0xffffffff, the plain calls' spp = 0.  cam->spp is ignored (the camera is checked with spp 1);
 * cam->seed, or the per-tile seeds, act as in the plain calls.  stats->samples is the sum of k * k over
 * the rendered pixels.  Limits: sides above 255 and spp values that are not squares are not expressible;
 * the map is per frame, not per tile.  DESIGN.md §4.11.
 * Order of checks: everything the plain call checks, in its order, with spp taken as 1; then a NULL
 * map (WGT_E_INVALID "null sample map", nothing launched).  A map value cannot be out of range.
 * wgt_render_tile_sampled: wgt_render_tile with a HOST map (W x H bytes, borrowed for the call). */
int wgt_render_tile_sampled(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H,
                            uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, const uint8_t *sample_map,
                            uint8_t *rgba8_out, float *rgba32f_out, uint32_t *hit_id_out, wgt_stats *stats);
/* wgt_render_tiles_async with a DEVICE map, read by the launch in stream order: the rules for
 * ordering and workspace slots are wgt_render_tiles_async's.  With LPT ordering on (the default) the
 * cost pre-pass always runs, each pixel at min(k, WGT_PQ_LPT) per side; no result bit depends on it. */
int wgt_render_tiles_sampled_async(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H,
                                   uint32_t tw, uint32_t th, const wgt_tile *d_tiles, uint32_t n_tiles,
                                   const uint8_t *d_sample_map, void *d_rgba8, float *d_rgba32f,
                                   uint32_t *d_hit_id, void *stream);

/* ---- closest-hit queries (sample_hit, path_tracer.wgsl:290-310) ---------- */
/* Rays as SoA host arrays ox,oy,oz,dx,dy,dz (each n floats, packed in that order
 * in `rays`, i.e. rays[k*n + i]).  Writes prim id (lights, quads, triangles,
 * spheres numbered consecutively; 0xffffffff = miss) and hit distance.
 * Rays are not validated.  The answers equal the reference's arithmetic for any finite ray,
 * which outside the scene limits (coordinates within 2^40) means: a ray exactly parallel to an
 * axis (a direction component below 2^-87 in magnitude, which the triangle boxes' slab test
 * replaces by +-2^-87) misses every triangle once its origin component on that axis reaches
 * 2^41 in magnitude, because the slab offset o/d overflows; and a ray with |d| |o - c| above
 * 1.8e19 for a sphere centre c returns that sphere with a NaN distance (the discriminant is
 * inf - inf, and the reference accepts a NaN).  The same holds for wgt_trace_hits and
 * wgt_occluded_rays (a NaN distance is below no limit). */
int wgt_trace_rays(wgt_ctx *ctx, const float *rays, uint32_t n, uint32_t *prim_id, float *dist);
int wgt_trace_rays_async(wgt_ctx *ctx, const float *d_rays, uint32_t n, uint32_t *d_prim_id,
                         float *d_dist, void *stream);

/* ---- occlusion (any-hit) queries with a per-ray distance limit ----------- */
/* Rays as for wgt_trace_rays; max_dist: n floats, in scene units (the Euclidean hit
 * distance `dist` of wgt_trace_rays, not the ray parameter).  occluded[i] = 1 iff
 * wgt_trace_rays on ray i returns a primitive and dist < max_dist[i] (an IEEE f32
 * comparison: a NaN limit, a limit <= 0, a miss and a NaN ray give 0; +inf asks for
 * any hit at all), else 0.  The answer is exact; the query stops at the first such
 * primitive and culls the tree with the limit. */
int wgt_occluded_rays(wgt_ctx *ctx, const float *rays, const float *max_dist, uint32_t n, uint8_t *occluded);
int wgt_occluded_rays_async(wgt_ctx *ctx, const float *d_rays, const float *d_max_dist, uint32_t n,
                            uint8_t *d_occluded, void *stream);

/* ---- full hit records (HitInfo after sample_hit, path_tracer.wgsl:27-36) --- */
#define WGT_HIT_EMISSIVE   1u
#define WGT_HIT_FRONT_FACE 2u
/* Planar outputs for n records; any pointer may be NULL (that field is not written),
 * at least one must be set.  pos/norm/col: 3 planes of n floats, f[k*n + i].
 * HitInfo's shape and uv are not returned: shading never reads them, and shape follows
 * from the range prim lies in (lights and quads, then triangles, then spheres). */
typedef struct {
  uint32_t *prim;  /* as wgt_trace_rays */
  float *dist;     /* as wgt_trace_rays */
  float *pos;      /* HitInfo.pos  = o + t d */
  float *norm;     /* HitInfo.norm (turned against the ray) */
  float *col;      /* HitInfo.col */
  uint8_t *flags;  /* WGT_HIT_EMISSIVE | WGT_HIT_FRONT_FACE */
} wgt_hit_buffers;   /* 48 bytes */

/* Rays as for wgt_trace_rays.  Record i is the reference's HitInfo after sample_hit on
 * ray i, exact: the renderer's own functions on the same operands.  prim and dist equal
 * wgt_trace_rays on the same ray bit for bit.  A miss is hit_init's state: prim =
 * 0xffffffff, dist = kRayMax (1e20), zero vectors, flags = 0.  A ray with a NaN component
 * gives the last sphere with NaN fields, as in the renderer.  The synchronous form takes
 * a struct of host pointers, the async form a host struct of device pointers. */
int wgt_trace_hits(wgt_ctx *ctx, const float *rays, uint32_t n, const wgt_hit_buffers *out);
int wgt_trace_hits_async(wgt_ctx *ctx, const float *d_rays, uint32_t n, const wgt_hit_buffers *d_out,
                         void *stream);

/* First-hit G-buffer: the record of pixel (x, y) is the HitInfo of sample 0's primary ray
 * of that pixel, the ray whose primitive wgt_render_tile reports in hit_id_out (prim
 * equals it bit for bit).  cam->spp and cam->seed set that ray's jitter, as in the render;
 * a pixel without samples (floor(sqrt(spp)) == 0) gets the miss record.  n = tw*th records,
 * row-major.  rays_out (may be NULL) receives that ray as 6 planes of n floats, the layout
 * of wgt_trace_rays' input (zeros for a pixel without samples), so it can be fed straight
 * back into the ray queries.  Pixels of the rectangle outside the frame get prim =
 * 0xffffffff and zeros in every other field and in the ray. */
int wgt_render_gbuffer(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H,
                       uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th,
                       const wgt_hit_buffers *out, float *rays_out);
/* The tile-list form with device buffers, as wgt_render_tiles_async: n = n_tiles*tw*th
 * records at the pixel offset (t*th + ly)*tw + lx, cam->seed ignored (per-tile seeds),
 * pixels of a tile outside the frame left untouched, ordered on `stream`. */
int wgt_render_gbuffer_async(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H,
                             uint32_t tw, uint32_t th, const wgt_tile *d_tiles, uint32_t n_tiles,
                             const wgt_hit_buffers *d_out, float *d_rays, void *stream);

/* The G-buffer of a sampled frame: sample 0's jitter is -0.5 + rand / k, so it depends on the pixel's
 * side, and the record needs the frame's sample map to keep prim equal to the sampled render's
 * hit_id_out bit for bit.  A pixel with k = 0 gets the miss record and a zero ray.  Otherwise as
 * wgt_render_gbuffer and wgt_render_gbuffer_async; the map and the order of checks as
 * wgt_render_tile_sampled (HOST map) and wgt_render_tiles_sampled_async (DEVICE map): the NULL map
 * is checked last. */
int wgt_render_gbuffer_sampled(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H,
                               uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th, const uint8_t *sample_map,
                               const wgt_hit_buffers *out, float *rays_out);
int wgt_render_gbuffer_sampled_async(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H,
                                     uint32_t tw, uint32_t th, const wgt_tile *d_tiles, uint32_t n_tiles,
                                     const uint8_t *d_sample_map, const wgt_hit_buffers *d_out, float *d_rays,
                                     void *stream);

/* ---- closest-point queries (no reference counterpart; Embree's rtcPointQuery) -- */
/* Planar outputs for n records; any pointer may be NULL (that field is not written), at least one
 * must be set. */
typedef struct {
  uint32_t *prim;  /* n */
  float *dist;     /* n */
  float *pos;      /* 3 planes of n: the closest point q */
  float *uv;       /* 2 planes of n: the weights (v, w) of e1 and e2 */
} wgt_nearest_buffers;   /* 32 bytes */

/* Record i = the triangle of the scene nearest to point i (points: 3 planes of n floats, x, y, z):
 * the minimum of (d2, primitive id) over the scene's triangles, d2 the fp32 squared distance to the
 * closest point q = (v0 + v e1) + w e2 of the triangle's resident record (after an upload the
 * caller's v0, e1, e2; after wgt_update_* or a rebuild what wgt_bvh_read's tris_out returns), by the
 * seven-region test stated operation by operation in DESIGN.md §4.13; ties go to the lower id, a
 * triangle whose d2 is NaN or infinite is never the answer.  prim as wgt_trace_rays numbers triangles,
 * dist = sqrt(d2) correctly rounded.  The record is reported iff dist < max_dist[i] (an IEEE f32
 * comparison: a NaN, zero or negative limit reports nothing, +inf or a NULL max_dist anything);
 * otherwise, and for a point with a NaN or infinite component or a scene without triangles, it is the
 * miss record: prim = 0xffffffff, dist = +inf, pos = 0, uv = 0.  Only triangles are searched: no quads,
 * lights or spheres; no signed distance; one nearest triangle: the k nearest and the number within the
 * radius are wgt_nearest_k_points' answers, below.
 * The answers equal wgt_nearest_points_spec on the resident triangles bit for bit; the BVH and the
 * radius only cull (DESIGN.md §4.13 states for which triangle shapes that is proved).
 * Order of checks, each WGT_E_INVALID naming the argument, nothing launched: NULL context;
 * WGT_E_NOSCENE; n == 0 (success, nothing done); NULL points; NULL out or an out without a field.  n has
 * no limit of its own, as wgt_trace_rays' has none.  Pointers are not validated.
 * The synchronous form takes host pointers and stages through the context's scratch; the async form
 * takes device pointers and a host struct of device pointers, and follows wgt_trace_rays_async's rules:
 * ordered on `stream` (NULL = the context's) after every earlier query, update and rebuild of the
 * context, returns once queued. */
int wgt_nearest_points(wgt_ctx *ctx, const float *points, const float *max_dist, uint32_t n,
                       const wgt_nearest_buffers *out);
int wgt_nearest_points_async(wgt_ctx *ctx, const float *d_points, const float *d_max_dist, uint32_t n,
                             const wgt_nearest_buffers *d_out, void *stream);
/* Diagnostic, synchronous, device pointers: the same answers from an instrumented instantiation;
 * counts[0] = node visits, counts[1] = triangle tests, summed over the n points.  NULL counts is
 * refused last. */
int wgt_nearest_points_stats(wgt_ctx *ctx, const float *d_points, const float *d_max_dist, uint32_t n,
                             const wgt_nearest_buffers *d_out, uint64_t counts[2]);
/* Host only, no device: the definition by brute force over tris[0..n_tris) in index order, primitive
 * ids first_prim + i.  n_tris == 0 gives misses.  WGT_E_INVALID for NULL tris with n_tris > 0, NULL
 * points, a NULL or empty out (n == 0 succeeds first). */
int wgt_nearest_points_spec(const wgt_triangle *tris, uint32_t n_tris, uint32_t first_prim, const float *points,
                            const float *max_dist, uint32_t n, const wgt_nearest_buffers *out);

/* ---- k-nearest and within-radius closest-point queries ---------------------- */
#define WGT_NEAREST_MAX_K 32u
/* Planar outputs for n points; any pointer may be NULL (that field is not written), at least one must be
 * set.  prim, dist, pos and uv are the list fields: entry j of point i is at plane j (prim, dist), planes
 * 3 j + axis (pos) and 2 j + {0: v, 1: w} (uv), element i. */
typedef struct {
  uint32_t *count; /* n */
  uint32_t *prim;  /* k planes of n */
  float *dist;     /* k planes of n */
  float *pos;      /* 3k planes of n: plane (3*j + axis) */
  float *uv;       /* 2k planes of n: plane (2*j + {v,w}) */
} wgt_nearest_k_buffers; /* 40 bytes */

/* The triangles within a radius of each point: how many, and the k nearest (points and max_dist as for
 * wgt_nearest_points).  For point i = p and m = max_dist[i] (a NULL max_dist: +inf), with d2_t the fp32
 * squared distance from p to triangle t's resident record exactly as wgt_nearest_points computes it
 * (DESIGN.md §4.13): S is the set of triangles with d2_t < +inf and sqrt(d2_t) < m, the root correctly
 * rounded and the comparison IEEE f32: a NaN d2 is in no set, a NaN, zero or negative m gives the empty
 * set.  count[i] = |S|, all of it, not capped at k.  Entry j < k of the list is the j-th element of S by
 * (d2, prim) ascending (d2 compared as f32, prim as wgt_trace_rays numbers triangles): prim, dist =
 * sqrt(d2), the closest point pos and its weights uv, as wgt_nearest_points reports them; entries
 * j >= min(|S|, k) hold 0xffffffff, +inf, zeros.  A point with a NaN or infinite component, or a scene
 * without triangles, gives empty entries and count = 0.  Only triangles are searched.
 * Consequences: S is a prefix of the (d2, prim) order over all triangles with a finite d2 (the root is
 * monotone); the list for k is a prefix of the list for any larger k; entry 0 equals wgt_nearest_points'
 * record bit for bit, in all four fields, for the same point and radius; two triangles with different d2
 * that round to the same dist are ordered by d2, not by prim.
 * With count asked for, every triangle within the radius is visited; without it the search stops
 * looking beyond the k-th distance: the answers are the same.  They equal
 * wgt_nearest_k_points_spec on the resident triangles bit for bit; the BVH, the radius and the k-th
 * distance only cull (for the triangle shapes DESIGN.md §4.13 names).
 * Order of checks, each WGT_E_INVALID naming the argument, nothing launched: NULL context;
 * WGT_E_NOSCENE; n == 0 (success, nothing done); NULL points; NULL out or an out without a field; k
 * outside 1..32 when a list field is asked for (with only count asked for k is ignored); in the stats
 * form NULL counts last.  Pointers are not validated.
 * The synchronous form takes host pointers and stages through the context's scratch; the async form
 * takes device pointers and a host struct of device pointers, and follows wgt_trace_rays_async's rules:
 * ordered on `stream` (NULL = the context's) after every earlier query, update and rebuild of the
 * context, returns once queued. */
int wgt_nearest_k_points(wgt_ctx *ctx, const float *points, const float *max_dist, uint32_t n, uint32_t k,
                         const wgt_nearest_k_buffers *out);
int wgt_nearest_k_points_async(wgt_ctx *ctx, const float *d_points, const float *d_max_dist, uint32_t n, uint32_t k,
                               const wgt_nearest_k_buffers *d_out, void *stream);
/* Diagnostic, synchronous, device pointers: the same answers from an instrumented instantiation;
 * counts[0] = node visits, counts[1] = triangle tests, summed over the n points. */
int wgt_nearest_k_points_stats(wgt_ctx *ctx, const float *d_points, const float *d_max_dist, uint32_t n, uint32_t k,
                               const wgt_nearest_k_buffers *d_out, uint64_t counts[2]);
/* Host only, no device: the definition by brute force over tris[0..n_tris) in index order, primitive
 * ids first_prim + i.  n_tris == 0 gives empty records.  WGT_E_INVALID for NULL tris with n_tris > 0, NULL
 * points, a NULL or empty out, k out of range with a list field (n == 0 succeeds first). */
int wgt_nearest_k_points_spec(const wgt_triangle *tris, uint32_t n_tris, uint32_t first_prim, const float *points,
                              const float *max_dist, uint32_t n, uint32_t k, const wgt_nearest_k_buffers *out);

/* ---- triangle overlap queries: which resident triangles a triangle cuts ------ */
#define WGT_OVERLAP_MAX_K 32
/* Planar outputs for n query triangles; any pointer may be NULL (that field is not written), at least one
 * must be set.  Entry j of query i is at plane j of prim, element i. */
typedef struct {
  uint8_t *hit;    /* n: 1 when the query cuts a resident triangle, else 0 */
  uint32_t *count; /* n */
  uint32_t *prim;  /* k planes of n */
} wgt_overlap_buffers; /* 24 bytes */

/* The resident triangles each query triangle cuts.  tris: nine planes of n floats, the corners a0.x a0.y
 * a0.z a1.x a1.y a1.z a2.x a2.y a2.z (the planar convention of the points and rays).  For query i = A =
 * (a0, a1, a2) and resident triangle B = (v0, e1, e2) with its padded box [lo, hi], in
 * IEEE f32 with +, -, * only, no division and no fused operation (DESIGN.md §4.17 has every formula):
 *   segment o + t d, 0 <= t <= 1, crosses triangle (w0, f1, f2): two-sided Moller-Trumbore with the
 *     quotients cleared; with det, U, V, T its determinant and numerators and a, U', V', T' their values
 *     negated when det < 0:  a > 0, U' >= 0, V' >= 0, U' + V' <= a, 0 <= T' <= a.  A NaN or a zero
 *     determinant says no.
 *   A and B overlap iff min(a0, a1, a2) <= hi and max(a0, a1, a2) >= lo on each axis (exact; the query gets
 *     no pad) and one of six segments crosses: A's edges (a0, a1 - a0), (a1, a2 - a1), (a2, a0 - a2)
 *     against B, or B's edges (v0, e1), (v0, e2), (v0 + e1, e2 - e1) against (a0, a1 - a0, a2 - a0).
 * A query is valid iff its nine coordinates are finite and within 2^40 and every component of a1 - a0,
 * a2 - a0 and a2 - a1 is within 2^30 (the scene's own triangle limits); an invalid query, or a scene
 * without triangles, gives the empty answer.  With S the set of resident triangles that overlap A:
 * count[i] = |S|, all of it, not capped at k; hit[i] = count > 0; entry j < k of prim is the j-th lowest
 * primitive id of S (as wgt_trace_rays numbers triangles); entries j >= min(|S|, k) hold 0xffffffff.
 * Only triangles are searched: no quads, lights or spheres.
 * Consequences: the box clause removes no real intersection (the pad only enlarges B) and makes the BVH's
 * cull exact, so the answers equal wgt_overlap_triangles_spec on the resident triangles bit for bit with
 * no condition on the triangles' shapes.  Coplanar pairs are never reported (all six determinants are
 * zero); nearly coplanar pairs are decided by rounding.  A triangle wholly inside a closed mesh cuts
 * nothing: combine with an inside test.  Touching counts (the comparisons admit equality), so neighbours in
 * one mesh that share a vertex or an edge usually report each other: a self-intersection check filters
 * those by id.  The list for k is a prefix of the list for any larger k.  No intersection segment, no
 * swept (continuous) test.
 * With hit alone asked for the search ends at the first overlapping triangle; otherwise every triangle the
 * boxes allow is visited.
 * Order of checks, each WGT_E_INVALID naming the argument, nothing launched: NULL context;
 * WGT_E_NOSCENE; n == 0 (success, nothing done); NULL tris; NULL out; an out without a field; k > 32;
 * k == 0 with prim asked for; k > 0 without prim; in the stats form NULL counts last.  Pointers are not
 * validated.
 * The synchronous form takes host pointers and stages through a device allocation of the call's own; the
 * async form takes device pointers and a host struct of device pointers, and follows
 * wgt_trace_rays_async's rules: ordered on `stream` (NULL = the context's) after every earlier query,
 * update and rebuild of the context, returns once queued. */
int wgt_overlap_triangles(wgt_ctx *ctx, const float *tris, uint32_t n, uint32_t k, const wgt_overlap_buffers *out);
int wgt_overlap_triangles_async(wgt_ctx *ctx, const float *d_tris, uint32_t n, uint32_t k,
                                const wgt_overlap_buffers *d_out, void *stream);
/* Diagnostic, synchronous, device pointers: the same answers from an instrumented instantiation;
 * counts[0] = node visits, counts[1] = triangle tests, summed over the n queries. */
int wgt_overlap_triangles_stats(wgt_ctx *ctx, const float *d_tris, uint32_t n, uint32_t k,
                                const wgt_overlap_buffers *d_out, uint64_t counts[2]);
/* Host only, no device: the definition by brute force over tris[0..n_tris) in index order, primitive ids
 * first_prim + i, each triangle's padded box computed from its record; it culls nothing.  n_tris == 0
 * gives empty answers.  WGT_E_INVALID for NULL tris with n_tris > 0, then the checks above from NULL query
 * on (n == 0 succeeds first). */
int wgt_overlap_triangles_spec(const wgt_triangle *tris, uint32_t n_tris, uint32_t first_prim, const float *query,
                               uint32_t n, uint32_t k, const wgt_overlap_buffers *out);

/* ---- self-intersection queries: which resident triangles each resident triangle cuts ---- */
/* The resident mesh against itself, neighbours excluded.  The queries are the resident records; `indices` (3 *
 * n_tris labels, triangle i's at 3i .. 3i + 2, by upload index; may be NULL) is the only statement of
 * adjacency; out is a wgt_overlap_buffers sized by the scene's triangle count n_tris and indexed by upload
 * index (prim: k planes of n_tris).  For resident triangles s and t with records (v0, e1, e2) and padded boxes
 * (DESIGN.md §3.4), in IEEE f32 with +, -, * only, no division and no fused operation:
 *   corners(x) = (v0, v0 + e1, v0 + e2), each sum rounded once
 *   adjacent(s, t): with indices, any of s's three labels equals any of t's.  Labels are compared for
 *     equality only: they are never addresses and need no range.  With NULL indices nothing is adjacent.
 *   self_overlap(s, t), lo = min(s, t), hi = max(s, t): s != t, not adjacent(s, t), the two padded boxes
 *     overlap on each axis (comparisons with equality), and one of wgt_overlap_triangles' six segments
 *     crosses with corners(lo) as the query A and record hi as the resident B.
 * The lower id is always the query, so the decision is one function of the unordered pair: t is reported for
 * s iff s is reported for t, bit for bit.  With S_s the set of t that overlap s: count[s] = |S_s|, all of it,
 * not capped at k; hit[s] = count > 0; entry j < k of prim is the j-th lowest primitive id of S_s (as
 * wgt_trace_rays numbers triangles); entries j >= min(|S_s|, k) hold 0xffffffff.  For s < t not adjacent,
 * whatever wgt_overlap_triangles reports for corners(s) against t is reported here.
 * Consequences: the box clause removes no real intersection (a corner box nests in its padded box) and makes
 * the BVH's cull exact (a node box is the exact union of the padded boxes below it), so the answers equal
 * wgt_overlap_self_spec on the resident triangles bit for bit.  Limits: two triangles that share a label and
 * still cut each other (a fold through a shared vertex) are not reported; coplanar pairs are never reported;
 * only triangles are searched.  With hit alone asked for the search ends at the first member.
 * The answers follow wgt_update_* and wgt_rebuild_*; ids are upload indices throughout.
 * Order of checks, each WGT_E_INVALID naming the argument, nothing launched: NULL context; WGT_E_NOSCENE; a
 * scene without triangles (success, nothing done, as wgt_overlap_triangles with n == 0); NULL out; an out
 * without a field; k > 32; k == 0 with prim asked for; k > 0 without prim; in the stats form NULL counts
 * last.  Pointers are not validated.
 * The synchronous form takes host pointers and stages through a device allocation of the call's own; the
 * async form takes device pointers and a host struct of device pointers and follows wgt_trace_rays_async's
 * rules.  The return types stand on lines of their own: tests/test_overlap_abi.py counts every one-line
 * `int wgt_overlap_...(` as one of wgt_overlap_triangles' four forms. */
int
wgt_overlap_self(wgt_ctx *ctx, const uint32_t *indices, uint32_t k, const wgt_overlap_buffers *out);
int
wgt_overlap_self_async(wgt_ctx *ctx, const uint32_t *d_indices, uint32_t k, const wgt_overlap_buffers *d_out,
                       void *stream);
/* Diagnostic, synchronous, device pointers: the same answers from an instrumented instantiation;
 * counts[0] = node visits, counts[1] = triangle tests, summed over the n_tris lanes. */
int
wgt_overlap_self_stats(wgt_ctx *ctx, const uint32_t *d_indices, uint32_t k, const wgt_overlap_buffers *d_out,
                       uint64_t counts[2]);
/* Host only, no device: the definition by brute force over every ordered pair of tris[0..n_tris), primitive
 * ids first_prim + i, each triangle's padded box computed from its record; it culls nothing.  n_tris == 0
 * succeeds and does nothing; then WGT_E_INVALID for NULL tris, then the checks above from NULL out on. */
int
wgt_overlap_self_spec(const wgt_triangle *tris, uint32_t n_tris, uint32_t first_prim, const uint32_t *indices,
                      uint32_t k, const wgt_overlap_buffers *out);

/* ---- radiance queries (compute_sample's path loop on the caller's rays) ---- */
/* Planar outputs for n rays; any pointer may be NULL (that field is not written), at least one must
 * be set. */
typedef struct {
  float *rgb;         /* 3 planes of n: r, g, b */
  uint32_t *prim;     /* n: the primitive the first sample's ray hits (as wgt_trace_rays) */
  uint32_t *seed_out; /* n: the RNG state after the last sample */
} wgt_radiance_buffers;  /* 24 bytes */

/* How much light arrives along ray i: `samples` paths traced with the renderer's own raytrace()
 * (path_tracer.wgsl:264-288), from origin o and direction d (rays as for wgt_trace_rays: six planes of
 * n floats; d is not normalised and not validated) and RNG state s:
 *
 *   seed = s; col = (0,0,0); prim = 0xffffffff
 *   for j in 0 .. samples-1:
 *     p = Path{ray = (o, d), col = (1,1,1), end = false}
 *     for depth in 0 .. 49:
 *       p = raytrace(p, depth, &seed)
 *       if j == 0 and depth == 0: prim = that hit's primitive id
 *       if p.end: break
 *     col += max(p.col, 0) / f32(samples)            (path_tracer.wgsl:393)
 *
 * which is compute_sample with the camera ray replaced by the caller's and without the two jitter
 * draws: a frame rendered at spp = 1 is, per pixel, this query on the ray wgt_render_gbuffer exports,
 * from the state two rand() past the pixel's seed, bit for bit.  samples == 0 gives zero colour,
 * prim = 0xffffffff and the seed unchanged.  A ray with a NaN component behaves as in the renderer: it
 * hits the last sphere, and unless that sphere is emissive the state advances by 3 draws per remaining
 * bounce and the sample adds 0.  The arithmetic is the renderer's (its short divisions), exact against
 * the reference for origins within 2^40 and directions within 2^32 per component.
 * seeds == NULL: ray i starts from seed0 + i (32-bit wrap-around); else from seeds[i], and seed0 is
 * ignored.  seed_out makes calls composable: one call with S samples equals S chained one-sample calls
 * whose colours the caller sums as col = col + c_j / f32(S) in fp32, in order.
 * Order of checks, each WGT_E_INVALID naming the argument, nothing launched: NULL context;
 * WGT_E_NOSCENE; n == 0 (success, nothing done); NULL rays; NULL out or an out without a field;
 * samples above 65536; in the stats form NULL counts last.
 * The synchronous form takes host pointers and stages through the context's scratch; the async form
 * takes device pointers and a host struct of device pointers, and follows wgt_trace_rays_async's rules:
 * ordered on `stream` (NULL = the context's) after every earlier query, update and rebuild of the
 * context, returns once queued. */
int wgt_trace_radiance(wgt_ctx *ctx, const float *rays, const uint32_t *seeds, uint32_t seed0, uint32_t samples,
                       uint32_t n, const wgt_radiance_buffers *out);
int wgt_trace_radiance_async(wgt_ctx *ctx, const float *d_rays, const uint32_t *d_seeds, uint32_t seed0,
                             uint32_t samples, uint32_t n, const wgt_radiance_buffers *d_out, void *stream);
/* Diagnostic, synchronous, device pointers: the same answers from an instrumented instantiation (the
 * timed path carries no atomics); counts = sample_hit calls, those on rays without a NaN component,
 * paths started, those on NaN rays (the oracle's O_CNT_QUERIES, TRACED, SAMPLES, NAN_RAYS), summed
 * over the n rays. */
int wgt_trace_radiance_stats(wgt_ctx *ctx, const float *d_rays, const uint32_t *d_seeds, uint32_t seed0,
                             uint32_t samples, uint32_t n, const wgt_radiance_buffers *d_out, uint64_t counts[4]);

/* ---- multi-hit queries (no reference counterpart; what lies behind the first surface) ---- */
#define WGT_MULTI_HIT_TRIS_ONLY 1u /* flags: the scene's triangles only; ids unchanged */
#define WGT_MULTI_HIT_MAX_K 32u
/* Any pointer may be NULL (that field is not written), at least one must be set. */
typedef struct {
  uint32_t *count; /* n, may be NULL */
  uint32_t *prim;  /* k planes of n, may be NULL */
  float *dist;     /* k planes of n, may be NULL */
} wgt_multi_hit_buffers; /* 24 bytes */

/* The k nearest hits of each ray and the number of all its hits (rays as for wgt_trace_rays: six planes
 * of n floats).  For ray i = (o, d) and m = max_dist[i] (a NULL max_dist: +inf), lim = min(m, 1e20):
 * a primitive is HIT when the closest-hit code of wgt_trace_rays accepts it tested alone (no other
 * primitive present) at a distance dist with dist < lim, an IEEE f32 comparison: a NaN distance is
 * below nothing, a zero, negative or NaN m gives no hits.  A ray with a NaN or infinite component has
 * no hits, by definition.  A sphere gives at most the one root the reference accepts.  With S the set of
 * hit primitives: count[i] = |S|, all of it, not capped at k; prim[j*n + i] and dist[j*n + i], j < k, hold
 * the j-th element of S by (dist, prim) ascending (dist compared as f32, prim as wgt_trace_rays numbers:
 * lights, quads, triangles, spheres), and 0xffffffff and +inf for j >= min(|S|, k).
 * WGT_MULTI_HIT_TRIS_ONLY: S holds triangles only; quads, lights and spheres are not tested.  A scene
 * without triangles then answers with empty records.
 * Consequences: count > 0 equals wgt_occluded_rays with the same limit for every ray with finite
 * components for which no quad or sphere yields a NaN distance.  For a ray that wgt_trace_rays answers
 * with a non-NaN distance, dist[0*n + i] equals that distance bit for bit, and prim[0*n + i] its
 * primitive except when two triangles have different t but the same rounded dist (the closest-hit order
 * among triangles is (t, index), this one (dist, prim)).  Crossing parity (count & 1 of a tris-only
 * query) tells inside from outside of a closed mesh.
 * With count asked for, every hit below the limit is visited; without it the search stops looking
 * beyond the k-th distance: the answers are the same.
 * Order of checks, each WGT_E_INVALID naming the argument, nothing launched: NULL context;
 * WGT_E_NOSCENE; n == 0 (success, nothing done); NULL rays; NULL out or an out without a field; unknown
 * flag bits; k outside 1..32 when prim or dist is asked for (with only count asked for k is ignored); in
 * the stats form NULL counts last.
 * The synchronous form takes host pointers and stages through the context's scratch; the async form
 * takes device pointers and a host struct of device pointers, and follows wgt_trace_rays_async's rules:
 * ordered on `stream` (NULL = the context's) after every earlier query, update and rebuild of the
 * context, returns once queued. */
int wgt_trace_multi_hits(wgt_ctx *ctx, const float *rays, const float *max_dist, uint32_t n, uint32_t k,
                         uint32_t flags, const wgt_multi_hit_buffers *out);
int wgt_trace_multi_hits_async(wgt_ctx *ctx, const float *d_rays, const float *d_max_dist, uint32_t n, uint32_t k,
                               uint32_t flags, const wgt_multi_hit_buffers *d_out, void *stream);
/* Diagnostic, synchronous, device pointers: the same answers from an instrumented instantiation;
 * counts[0] = node visits, counts[1] = triangle tests, summed over the n rays. */
int wgt_trace_multi_hits_stats(wgt_ctx *ctx, const float *d_rays, const float *d_max_dist, uint32_t n, uint32_t k,
                               uint32_t flags, const wgt_multi_hit_buffers *d_out, uint64_t counts[2]);

/* ---- denoising (no reference counterpart) --------------------------------- */
/* An edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a rendered W x H image, guided
 * by the first-hit G-buffer of the same pixels and demodulated by its albedo; no colour-distance
 * weight (DESIGN.md §4.7 states the arithmetic operation by operation; tests/denoise_restatement.py
 * is the same in numpy, and the result equals it bit for bit).  A pixel is filtered when it hit a
 * primitive that is not emissive and its guides and colour are finite and within 2^100; every other
 * pixel (lights, misses, NaN) passes through bit for bit and is never averaged into a neighbour.
 * Guides whose normals are far from unit length can overflow a weight to NaN in a filtered pixel; the
 * sign and payload of such a NaN are unspecified. */
#define WGT_DENOISE_DEMODULATE 1u
typedef struct {
  uint32_t iterations;   /* 1..8 (default 5): pass i (from 0) taps at a step of 2^i pixels */
  uint32_t normal_power; /* 0..10 (default 7): the normal weight max0(n.n') is squared this many times */
  float sigma_pos;       /* finite, > 0 (default 1.0): scene units per pixel of step, along the normal */
  uint32_t flags;        /* WGT_DENOISE_DEMODULATE (default): filter colour / albedo, multiply back after */
} wgt_denoise_params;    /* 16 bytes */
int wgt_denoise_defaults(wgt_denoise_params *out);
/* Bytes of device scratch wgt_denoise_async needs for a W x H image (a multiple of 256: 64 per
 * pixel); 0 for a size it refuses. */
size_t wgt_denoise_workspace_bytes(uint32_t W, uint32_t H);
/* rgba32f_in: W x H x 4 floats, row-major, the rgba32f output of wgt_render_tile (or of one full-frame
 * tile of wgt_render_tiles_async); guides: the planar records of the same W x H pixels as
 * wgt_render_gbuffer writes them, of which prim, pos, norm, col and flags are required and dist is
 * ignored.  Outputs: rgba32f_out (alpha is the input's) and rgba8_out (the renderer's rgba8unorm
 * store of the same rgb, alpha 255); one of the two may be NULL.  params NULL = the defaults.
 * No scene is needed.  Order of checks, each WGT_E_INVALID naming the argument, nothing launched:
 * NULL context; NULL input or guides; a NULL required guide; both outputs NULL; W or H 0 or above
 * 32768, or W * H above 2^25; parameters out of range; (async) NULL workspace, one not 256-byte
 * aligned, workspace_bytes below wgt_denoise_workspace_bytes(W, H).
 * Synchronous, HOST pointers; allocates and frees its own device workspace. */
int wgt_denoise(wgt_ctx *ctx, const wgt_denoise_params *params, uint32_t W, uint32_t H, const float *rgba32f_in,
                const wgt_hit_buffers *guides, float *rgba32f_out, uint8_t *rgba8_out);
/* DEVICE pointers (d_guides: a host struct of device pointers), ordered on `stream` (NULL = the
 * context's), returns once queued.  The input and the guides are never written.  d_rgba32f_out may
 * equal d_rgba32f_in: the input is consumed into the workspace before anything is written.  The
 * workspace is the caller's and holds nothing between calls: two calls on two streams with two
 * workspaces may overlap. */
int wgt_denoise_async(wgt_ctx *ctx, const wgt_denoise_params *params, uint32_t W, uint32_t H,
                      const float *d_rgba32f_in, const wgt_hit_buffers *d_guides, void *d_workspace,
                      size_t workspace_bytes, float *d_rgba32f_out, void *d_rgba8_out, void *stream);

/* ---- temporal accumulation (no reference counterpart) ---------------------- */
/* Carries radiance from one frame to the next by reprojection, the first half of SVGF-style
 * denoising and the natural input of wgt_denoise: each pixel of the current frame projects its
 * first-hit position with both cameras, gathers the previous frame's accumulated radiance around
 * where it lay there (bilinear, four taps, a tap accepted by its normal, its distance to the pixel's
 * plane and optionally its primitive), and blends the current colour in with weight 1 / history
 * length (DESIGN.md §4.8 states the arithmetic operation by operation; tests/temporal_restatement.py
 * is the same in numpy, and the result equals it bit for bit).  The library keeps no state: the
 * caller owns the history and alternates two wgt_temporal_state sets and two G-buffers.  A pixel
 * accumulates when it hit a primitive that is not emissive and its guides and colour are finite and
 * within 2^100; every other pixel (lights, misses, NaN) passes through bit for bit with len = 0 and
 * moments = 0, and is never a tap.  Known limit of this form: it knows no per-primitive motion, so a
 * moved triangle fails the plane test and restarts its history, while a triangle sliding in its own
 * plane keeps a history that is not its own; wgt_temporal_accumulate_motion (below) follows the
 * triangles that wgt_update_triangles and its device forms move. */
#define WGT_TEMPORAL_MATCH_PRIM 1u
typedef struct {
  uint32_t max_history; /* 1..65536 (default 32): the history length is capped here; 1 = no accumulation */
  float normal_min;     /* finite, -1..1 (default 0.9): a history tap needs dot(n, n_tap) >= this */
  float plane_tol;      /* finite, >= 0 (default 1.0): ... and |dot(n, pos_tap - pos)| <= this, scene units */
  uint32_t flags;       /* WGT_TEMPORAL_MATCH_PRIM (default off): ... and the same primitive id */
} wgt_temporal_params;  /* 16 bytes */

typedef struct {
  float *rgba32f;  /* W x H x 4: the accumulated radiance (alpha: the current frame's) */
  float *len;      /* W x H: history length, 0 for a pixel that is not accumulated */
  float *moments;  /* 2 planes of W x H, may be NULL: running mean of luminance and of luminance^2 */
} wgt_temporal_state; /* 24 bytes */

int wgt_temporal_defaults(wgt_temporal_params *out);
/* rgba32f_in and guides: the current frame's radiance and planar G-buffer records, as for
 * wgt_denoise (prim, pos, norm and flags are required; dist and col are ignored); cam: the camera
 * they were rendered with.  prev, guides_prev, cam_prev: the previous call's `out`, and the previous
 * frame's G-buffer and camera; all three NULL is the first frame, in which every accumulated pixel
 * starts a history of length 1.  spp and seed of both cameras are ignored.  out: the new state;
 * moments must be NULL or not in prev and out alike.  rgba8_out (may be NULL): the renderer's
 * rgba8unorm store of out's rgb, alpha 255.  params NULL = the defaults.  No scene is needed.
 * out->rgba32f may equal rgba32f_in (a pixel reads only its own current colour), but out->rgba32f,
 * out->len and out->moments must not overlap the prev buffer of the same name: the gather reads the
 * previous frame's neighbours.  rgba32f buffers are 16-byte aligned.
 * Order of checks, each WGT_E_INVALID naming the argument, nothing launched: NULL context; NULL
 * input, camera, guides, out, out->rgba32f or out->len; a NULL required guide; prev, guides_prev and
 * cam_prev not all NULL or all set, then a NULL prev->rgba32f, prev->len or required previous guide,
 * and moments in only one of prev and out; W or H 0 or above 32768, or W * H above 2^25; parameters
 * out of range (NaN is refused); a camera that a render would refuse for reasons other than its spp;
 * an out buffer overlapping its prev buffer.  A degenerate camera (origin equal to target, or looking
 * along the up axis) is no error: no pixel finds history.
 * Synchronous, HOST pointers; stages through one device allocation of its own and frees it. */
int wgt_temporal_accumulate(wgt_ctx *ctx, const wgt_temporal_params *params, uint32_t W, uint32_t H,
                            const wgt_camera_param *cam, const wgt_camera_param *cam_prev,
                            const float *rgba32f_in, const wgt_hit_buffers *guides,
                            const wgt_temporal_state *prev, const wgt_hit_buffers *guides_prev,
                            const wgt_temporal_state *out, uint8_t *rgba8_out);
/* DEVICE pointers inside host structs (the cameras are host structs), ordered on `stream` (NULL = the
 * context's), returns once queued.  The inputs and the previous state are never written.  One pass,
 * no workspace: calls that alternate two state sets on one stream need no synchronisation between
 * them, and independent sequences on two streams may overlap. */
int wgt_temporal_accumulate_async(wgt_ctx *ctx, const wgt_temporal_params *params, uint32_t W, uint32_t H,
                                  const wgt_camera_param *cam, const wgt_camera_param *cam_prev,
                                  const float *d_rgba32f_in, const wgt_hit_buffers *d_guides,
                                  const wgt_temporal_state *d_prev, const wgt_hit_buffers *d_guides_prev,
                                  const wgt_temporal_state *d_out, void *d_rgba8_out, void *stream);

/* ---- temporal history that follows moved triangles (no reference counterpart) -- */
/* A refit never changes topology and primitive ids are stable, so a pixel that hit triangle t can ask
 * where its hit point lay on t before the update.  Per frame: wgt_motion_snapshot, then the update,
 * then the render and its G-buffer, then wgt_motion_reproject, then wgt_temporal_accumulate_motion
 * (DESIGN.md §4.10 states the arithmetic operation by operation; tests/motion_restatement.py is the
 * same in numpy, and the results equal it bit for bit).
 *
 * wgt_motion_snapshot copies the resident triangles, as they are at that point of the stream's order
 * (NULL = the context's stream), into device memory the context owns: per original triangle index 48
 * bytes (v0, e1, e2 of its leaf-ordered record and its face normal) and the leaf slot of its record,
 * 52 bytes per triangle, allocated by the first snapshot after an upload and not counted in
 * wgt_scene_info's device_bytes.  It returns once queued, ordered against every query, every
 * reproject and every update of the context.  A later snapshot replaces it; an update never touches
 * it; wgt_upload_scene and wgt_destroy drop it.  WGT_E_NOSCENE before an upload, WGT_E_INVALID for a
 * scene without triangles. */
int wgt_motion_snapshot(wgt_ctx *ctx, void *stream);
/* Diagnostic (synchronous): the snapshot as n_tris x 12 floats (v0, e1, e2, face normal) in original
 * triangle order.  WGT_E_INVALID without a snapshot or with cap_tris below the scene's n_tris. */
int wgt_motion_snapshot_read(wgt_ctx *ctx, float *out, uint32_t cap_tris);

typedef struct {
  float *pos_prev;   /* 3 planes of n floats: where the hit point lay before the update */
  float *norm_prev;  /* 3 planes of n floats: the normal it had there (turned as the record's) */
} wgt_motion_buffers; /* 16 bytes */

/* guides: n planar records as wgt_render_gbuffer or wgt_trace_hits writes them, of which prim, pos,
 * norm and flags are required (dist and col are ignored).  A record that hit a triangle which differs
 * from the snapshot (any of the nine floats of v0, e1, e2) gets its hit point's barycentric
 * coordinates on the resident triangle carried to the snapshot's triangle, and the snapshot's face
 * normal turned by WGT_HIT_FRONT_FACE; every other record (an unmoved triangle, a quad, light, sphere,
 * miss or any other id) gets pos and norm back bit for bit, and nothing is indexed by its id.  A
 * zero-area triangle on either side gives NaN or inf, which wgt_temporal_accumulate_motion reads as
 * "no history".  n is 1..2^25.  Order of checks, each WGT_E_INVALID naming the argument, nothing
 * launched: NULL context; WGT_E_NOSCENE; no snapshot since the last upload; NULL guides or a NULL
 * required guide; NULL out or a NULL plane; n out of range.  Pointers are not validated.
 * The synchronous form takes host pointers and stages through the context's scratch; the async form
 * takes host structs of device pointers, is ordered on `stream` (NULL = the context's) against the
 * snapshots and updates of the context, and returns once queued. */
int wgt_motion_reproject(wgt_ctx *ctx, uint32_t n, const wgt_hit_buffers *guides, const wgt_motion_buffers *out);
int wgt_motion_reproject_async(wgt_ctx *ctx, uint32_t n, const wgt_hit_buffers *d_guides,
                               const wgt_motion_buffers *d_out, void *stream);

/* wgt_temporal_accumulate with the history looked up where the pixel's surface point lay before the
 * update: motion holds pos_prev and norm_prev of the W x H pixels (wgt_motion_reproject of `guides`).
 * The previous camera projects pos_prev instead of pos, a pixel whose pos_prev or norm_prev is not
 * finite and within 2^100 finds no history (it starts at len = 1), and a tap is tested against
 * norm_prev and the plane through pos_prev; everything else is wgt_temporal_accumulate's, and with
 * pos_prev == pos and norm_prev == norm bitwise so is the result, bit for bit.  motion and its two
 * planes are required when prev is set (checked right after the first-frame triple) and ignored on
 * the first frame, where motion may be NULL.  Every other argument, check and rule is
 * wgt_temporal_accumulate's, the synchronous and the async form alike. */
int wgt_temporal_accumulate_motion(wgt_ctx *ctx, const wgt_temporal_params *params, uint32_t W, uint32_t H,
                                   const wgt_camera_param *cam, const wgt_camera_param *cam_prev,
                                   const float *rgba32f_in, const wgt_hit_buffers *guides,
                                   const wgt_motion_buffers *motion, const wgt_temporal_state *prev,
                                   const wgt_hit_buffers *guides_prev, const wgt_temporal_state *out,
                                   uint8_t *rgba8_out);
int wgt_temporal_accumulate_motion_async(wgt_ctx *ctx, const wgt_temporal_params *params, uint32_t W, uint32_t H,
                                         const wgt_camera_param *cam, const wgt_camera_param *cam_prev,
                                         const float *d_rgba32f_in, const wgt_hit_buffers *d_guides,
                                         const wgt_motion_buffers *d_motion, const wgt_temporal_state *d_prev,
                                         const wgt_hit_buffers *d_guides_prev, const wgt_temporal_state *d_out,
                                         void *d_rgba8_out, void *stream);

/* ---- variance-guided denoising (no reference counterpart) ------------------ */
/* The second half of SVGF-style denoising: wgt_denoise's a-trous filter with a luminance weight
 * scaled by each pixel's own variance, over the state wgt_temporal_accumulate wrote.  The variance of
 * a pixel comes from its moments (the per-frame variance m2 - m1^2, not divided by the history
 * length), or under a history shorter than min_history from a 7 x 7 spatial estimate over the
 * moments; it is filtered along with the colour, and a 3 x 3 Gaussian of it sets each pass's
 * luminance tolerance: sigma_lum standard deviations (DESIGN.md §4.9 states the arithmetic operation
 * by operation; tests/denoise_variance_restatement.py is the same in numpy, and the result equals it
 * bit for bit).  A pixel is filtered when wgt_denoise would filter it and its len is >= 1 and its
 * moments are within 2^100; every other pixel passes through bit for bit, is never a tap and has
 * variance 0.  The moments are of raw luminance: the variance is demodulated by the luminance of the
 * albedo, which is exact for a grey albedo and an approximation otherwise. */
typedef struct {
  uint32_t iterations;   /* 1..8 (default 5): pass i (from 0) taps at a step of 2^i pixels */
  uint32_t normal_power; /* 0..10 (default 7): the normal weight max0(n.n') is squared this many times */
  float sigma_pos;       /* finite, > 0 (default 1.0): scene units per pixel of step, along the normal */
  uint32_t flags;        /* WGT_DENOISE_DEMODULATE (default): filter colour / albedo, multiply back after */
  float sigma_lum;       /* finite, > 0 (default 4.0): luminance tolerance in standard deviations */
  uint32_t min_history;  /* 1..64 (default 4): a shorter history takes the spatial variance estimate */
} wgt_denoise_variance_params; /* 24 bytes */
int wgt_denoise_variance_defaults(wgt_denoise_variance_params *out);
/* Bytes of device scratch wgt_denoise_variance_async needs for a W x H image (a multiple of 256: 64
 * per pixel); 0 for a size it refuses. */
size_t wgt_denoise_variance_workspace_bytes(uint32_t W, uint32_t H);
/* state: what wgt_temporal_accumulate wrote for these W x H pixels; rgba32f, len and moments are all
 * required.  guides: as for wgt_denoise (prim, pos, norm, col and flags are required).  Outputs:
 * rgba32f_out (alpha is the state's) and rgba8_out as wgt_denoise writes them, one of the two may be
 * NULL; variance_out (may be NULL): W x H floats, the filtered variance of the demodulated luminance,
 * 0 for a pixel that passes through.  params NULL = the defaults.  No scene is needed.
 * Order of checks, each WGT_E_INVALID naming the argument, nothing launched: NULL context; NULL state
 * or guides; a NULL state->rgba32f, state->len or state->moments; a NULL required guide; both colour
 * outputs NULL; W or H 0 or above 32768, or W * H above 2^25; parameters out of range (NaN is
 * refused); (async) NULL workspace, one not 256-byte aligned, workspace_bytes below
 * wgt_denoise_variance_workspace_bytes(W, H).
 * Synchronous, HOST pointers; allocates and frees its own device workspace. */
int wgt_denoise_variance(wgt_ctx *ctx, const wgt_denoise_variance_params *params, uint32_t W, uint32_t H,
                         const wgt_temporal_state *state, const wgt_hit_buffers *guides, float *rgba32f_out,
                         uint8_t *rgba8_out, float *variance_out);
/* DEVICE pointers inside host structs, ordered on `stream` (NULL = the context's), returns once
 * queued.  The state and the guides are never written.  d_rgba32f_out may equal d_state->rgba32f:
 * the state is consumed into the workspace before anything is written.  The workspace is the
 * caller's and holds nothing between calls: two calls on two streams with two workspaces may overlap. */
int wgt_denoise_variance_async(wgt_ctx *ctx, const wgt_denoise_variance_params *params, uint32_t W, uint32_t H,
                               const wgt_temporal_state *d_state, const wgt_hit_buffers *d_guides,
                               void *d_workspace, size_t workspace_bytes, float *d_rgba32f_out, void *d_rgba8_out,
                               float *d_variance_out, void *stream);

/* ---- planning a sample map from the accumulated state (no reference counterpart) ---- */
/* The next frame's sample map from what wgt_temporal_accumulate knows about this one: a pixel whose
 * history is at least min_history long wants ceil(gain * sqrt(max0(m2 - m1^2)) / (|m1| + lum_floor))
 * sides, clamped to [side_min, side_max]; a pixel the accumulation passes through (len = 0: lights,
 * misses, NaN) wants side_min; every other pixel (a short history, moments beyond 2^100) wants
 * side_max.  The wanted sides are dilated (the maximum within `dilate` pixels in x and y, in-image
 * pixels only), and a budget caps them: with B = floor(budget_spp * W * H), the map is min(dilated, c)
 * for the largest c in [side_min, side_max] whose sum of squares is at most B (c = side_min when not
 * even that fits, so the budget can then be exceeded).  DESIGN.md §4.11 states the arithmetic
 * operation by operation; tests/sample_plan_restatement.py is the same in numpy, and the map and its
 * total equal it bit for bit.  Nothing is summed in floating point across pixels: the cap comes from
 * a 256-bin integer histogram, so the result does not depend on the order of waves. */
typedef struct {
  uint32_t side_min;    /* 0..255 (default 1): every pixel gets at least this */
  uint32_t side_max;    /* side_min..255 (default 8): ... and at most this */
  float gain;           /* finite, > 0 (default 12.0): sides per unit of relative standard deviation */
  float lum_floor;      /* finite, > 0 (default 1.0): added to |m1| before dividing */
  uint32_t min_history; /* 1..64 (default 4): a shorter history is unknown and wants side_max */
  uint32_t dilate;      /* 0..3 (default 2): radius of the max filter over the wanted sides */
  float budget_spp;     /* finite, >= 0 (default 0 = none): the map's mean of k * k may not exceed this */
} wgt_sample_plan_params; /* 28 bytes */
int wgt_sample_plan_defaults(wgt_sample_plan_params *out);
/* Bytes of device scratch wgt_sample_plan_async needs for a W x H image (a multiple of 256: one per
 * pixel and the histogram); 0 for a size it refuses. */
size_t wgt_sample_plan_workspace_bytes(uint32_t W, uint32_t H);
/* state: what wgt_temporal_accumulate wrote for these W x H pixels; len and moments are required,
 * rgba32f is not read.  map_out: W x H bytes.  total_out (may be NULL): the map's sum of k * k, the
 * paths a sampled frame with it traces.  params NULL = the defaults.  No scene is needed; the library
 * keeps no state.
 * Order of checks, each WGT_E_INVALID naming the argument, nothing launched: NULL context; NULL state;
 * a NULL state->len or state->moments; a NULL map_out; W or H 0 or above 32768, or W * H above 2^25;
 * parameters out of range, in the struct's order (NaN is refused); (async) NULL workspace, one not
 * 256-byte aligned, workspace_bytes below wgt_sample_plan_workspace_bytes(W, H).
 * Synchronous, HOST pointers; allocates and frees its own device workspace. */
int wgt_sample_plan(wgt_ctx *ctx, const wgt_sample_plan_params *params, uint32_t W, uint32_t H,
                    const wgt_temporal_state *state, uint8_t *map_out, uint64_t *total_out);
/* DEVICE pointers (the state a host struct of device pointers), ordered on `stream` (NULL = the
 * context's), returns once queued: the cap is chosen on the device and applied in a second pass, so a
 * sampled render queued behind it on the same stream reads the finished map.  The state is never
 * written.  The workspace is the caller's and holds nothing between calls.  d_total_out is 8-byte aligned. */
int wgt_sample_plan_async(wgt_ctx *ctx, const wgt_sample_plan_params *params, uint32_t W, uint32_t H,
                          const wgt_temporal_state *d_state, void *d_workspace, size_t workspace_bytes,
                          uint8_t *d_map_out, uint64_t *d_total_out, void *stream);

int wgt_sync(wgt_ctx *ctx);
/* Diagnostics: the kernels' short sqrt / division forms (wgt_math.h sqrt_rn,
 * sqrt_fast, div_rn) against correctly rounded results (the f64 operation rounded
 * to f32): sqrt_rn on all 2^32 inputs, sqrt_fast on every input of its domain,
 * div_rn on n pseudo-random operand pairs of the quad distance under the render
 * limits (accept decision and accepted bits) and on n Moller-Trumbore reciprocals
 * 1/det (bits).  counts[0..7] = sqrt tests (2^32),
 * sqrt_rn mismatches, div tests (2n), div_rn mismatches, sqrt_fast tests,
 * sqrt_fast mismatches, and the mismatches of the compiler's own f32 sqrt and
 * division on the same inputs (synchronous). */
int wgt_selftest_math(wgt_ctx *ctx, uint32_t n, uint32_t seed, uint64_t counts[8]);

/* The context's HIP stream (hipStream_t) for callers that share it. */
void *wgt_stream(wgt_ctx *ctx);
/* Stream i (0..3) of the context's pipeline streams, created on first use with a
 * full CU mask so that each has a hardware queue of its own: frames issued
 * round-robin on them overlap (wgt_render_tiles_async).  NULL on error. */
void *wgt_pipeline_stream(wgt_ctx *ctx, uint32_t i);

/* ---- host-side scene helpers (no GPU needed) ----------------------------- */
/* Scene::Scene (scene.cpp:14-36): the reference Cornell box, 1 light, 17 quads,
 * 1 dummy sphere.  Capacities in *n_*; returns counts in *n_*. */
int wgt_scene_cornell(wgt_quad *lights, uint32_t *n_lights, wgt_quad *quads, uint32_t *n_quads,
                      wgt_sphere *spheres, uint32_t *n_spheres);
/* Triangle ctor (triangle.cpp:3-16): verts = n x 9 floats (v0, v1, v2). */
int wgt_make_triangles(const float *verts, uint32_t n, const float col[3], int emissive,
                       const float translation[3], wgt_triangle *out);
/* Scene::LoadObj (scene.cpp:56-131): OBJ -> triangles (fan-triangulated faces).
 * Call with out=NULL to get the count, then with a buffer of that capacity. */
int wgt_load_obj(const char *path, const float col[3], const float translation[3], int emissive,
                 wgt_triangle *out, uint32_t *n_inout);
/* Procedural stand-in meshes for absent assets: kind 0 = "bunny"
 * (displaced closed blob, ~target tris), kind 1 = "sponza" (colonnade/arch
 * architecture, ~target tris), placed inside the Cornell box. */
int wgt_procedural_mesh(int kind, uint32_t target_tris, uint32_t seed, wgt_triangle *out,
                        uint32_t *n_inout);
int wgt_write_obj(const char *path, const wgt_triangle *tris, uint32_t n);
int wgt_write_png(const char *path, const uint8_t *rgba8, uint32_t w, uint32_t h);

#ifdef __cplusplus
}
#endif
#endif /* WGT_API_H */
