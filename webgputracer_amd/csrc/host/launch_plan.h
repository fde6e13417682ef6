// launch_plan.h — what the C-ABI (wgt_runtime.cpp) decides before it touches the device, as
// functions that call no HIP runtime function: the numeric limits of scenes and cameras, the
// frame constants and their tuning knobs, the k_render_ps form of a tree, the device layout of a
// scene, the image passes' checks and plans, and the staging layout of their synchronous forms
// (StageLayout).  The programs of tests/host_sanitize run them without a GPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#include "../wgt_denoise.h"
#include "../wgt_denoise_variance.h"
#include "../wgt_internal.h"
#include "../wgt_motion.h"
#include "../wgt_multihit.h"
#include "../wgt_nearest.h"
#include "../wgt_nearest_k.h"
#include "../wgt_overlap.h"
#include "../wgt_overlap_self.h"
#include "../wgt_radiance.h"
#include "../wgt_rebuild.h"
#include "../wgt_sample_plan.h"
#include "../wgt_temporal.h"
#include "bvh.h"

namespace wgt {

// Numeric limits under which the kernels' short division (wgt_math.h div_rn, the
// quad plane distance) is exact wherever it decides anything:
// scene coordinates and ray origins within 2^40, quad normals within 2 per
// component (or NaN: a degenerate quad), triangle edge components within 2^30 (the
// short 1/det of Moller-Trumbore), primary ray directions within 2^32
// (scattered directions are unit).  Everything else in the kernels is exact for
// any input.  Outside the limits the calls fail with WGT_E_INVALID.
// kCoordLimit (2^40) and kEdgeLimit (2^30) are in wgt_internal.h: the device check of moved
// triangles (wgt_refit.hip) applies them too.
constexpr double kPrimaryDirLimit = 4294967296.0;  // 2^32
bool finite_within(const float* v, int n, double lim);  // NaN and inf fail too
// The checks return their refusal's text, empty when fine: of a scene's primitives, and of the
// camera and frame of a render or G-buffer call (check_render_args)
std::string check_scene_limits(const wgt_quad* lq, uint32_t nlq, const wgt_sphere* sp, uint32_t ns,
                               const wgt_triangle* tr, uint32_t nt);
// ... of one triangle, which the refusal names as triangle i
std::string check_triangle_limits(const wgt_triangle& t, uint32_t i);
std::string check_frame_args(const wgt_camera_param& cam, uint32_t W, uint32_t H, uint32_t tw, uint32_t th);
// Largest |coordinate| any point of the scene's primitives can have (quad corners,
// sphere boxes, triangle vertices): hit points, i.e. secondary ray origins, lie
// within it.  The compact nodes are built for ray origins within 4x this bound,
// which holds the reference camera outside its Cornell box (BvhOptions::origin_bound).
double scene_extent(const wgt_quad* lq, uint32_t nlq, const wgt_sphere* sp, uint32_t ns, const wgt_triangle* tr,
                    uint32_t nt);

// Tuning knobs (read per launch; defaults are the measured best).
uint32_t env_u32(const char* name, uint32_t dflt);
// setup_camera_ray's frame-invariant terms (path_tracer.wgsl:239-257), same fp32
// operations as the WGSL per-invocation evaluation, and the launch's knobs
DevFrame make_frame(const wgt_camera_param& cam, uint32_t W, uint32_t H);
// ... of a launch of n_tiles tiles of tw x th pixels
DevFrame tile_frame(const wgt_camera_param& cam, uint32_t W, uint32_t H, uint32_t tw, uint32_t th, uint32_t n_tiles);

// The traversal stack of the built tree, entries per lane (DevScene::stack): + 1, the
// speculative traversal parks a second leaf on the stack (wgt_trav_ps.h)
uint32_t stack_entries(const BvhOut& bvh);
// The k_render_ps form of a scene (PsForm), under WGT_PS_WAVES, WGT_PARK and WGT_PS_CAP
PsForm ps_form_for(const BvhOut& bvh, uint32_t n_tris);
// The BVH and kernel-form fields of the scene report, of wgt_bvh_build and of an upload alike
// (a scene without triangles reports zeros)
void fill_bvh_info(const BvhOut& bvh, uint32_t n_tris, const PsForm& f, wgt_scene_info& in);
// The build with the kernels' limits and the environment's knobs (BvhOptionsFromEnv), for ray
// origins within kOriginBoundScale x `extent` (scene_extent); returns the builder's refusal
std::string build_bvh(const wgt_triangle* tris, uint32_t n_tris, double extent, BvhOut& bvh);
// wgt_bvh_build, wgt_bvh_build_compact: the tree exactly as an upload of these triangles alone builds it
std::string build_for_export(const wgt_triangle* tris, uint32_t n_tris, BvhOut& bvh);

// The refit of a built tree to moved triangles (RefitBvh) under the same origin-bound rule:
// `extent` is the scene's with the new triangles (and its unchanged quads, lights and spheres)
std::string refit_bvh(const wgt_triangle* tris, uint32_t n_tris, double extent, BvhOut& bvh);
// wgt_bvh_refit: the tree an upload of `built_from` alone followed by an update to `now` holds
std::string refit_for_export(const wgt_triangle* built_from, const wgt_triangle* now, uint32_t n_tris, BvhOut& bvh);
// The argument checks of the updates, in the calls' order after the context and the scene; each
// returns the refusal's text, empty when fine.  wgt_update_triangles: the count alone.
std::string check_update_count(uint32_t scene_tris, uint32_t n_tris);
// wgt_update_triangles_device: null, the count, then the alignment rule: 16 bytes (the kernels read
// the records as float4s).
std::string check_update_records(const void* d_tris, uint32_t scene_tris, uint32_t n_tris);
// wgt_update_vertices_device: null vertices, the count, 4-byte alignment of the vertices and of the
// indices (may be null: unindexed), then n_verts: not 0, and 3 x n_tris when unindexed.
std::string check_update_vertices(const void* d_verts, uint32_t n_verts, const void* d_index, uint32_t scene_tris,
                                  uint32_t n_tris);
// Wording the device check's refusal (RefitCheck::first_bad = i) from that one triangle read back:
// check_triangle_limits on a record; of the vertex form first check_vertex_index on the triangle's
// three indices, then check_triangle_limits on triangle_of_vertices of its gathered 9 floats (v0, e1,
// e2 as wgt_make_triangles without a translation builds them, which is what the device checked).
void triangle_of_vertices(const float* verts, wgt_triangle& t);
std::string check_vertex_index(const uint32_t index[3], uint32_t n_verts, uint32_t i);
// The triangles' term of scene_extent that the device check reduced (no triangle was refused).
double checked_extent(const RefitCheck& r);
// What the device refit (wgt_update_triangles) decides on the host.  The compact codes' bound M
// for ray origins within kOriginBoundScale x `extent`, from the refit root node alone (32 floats):
// every box of the tree nests in the root's slots exactly, so they hold the largest |coordinate|.
// This is CompactForm's M.
double compact_bound(double extent, const float* root_node);
// The nodes of each level (BvhImage::level), levels in order: level l's nodes are order[begin[l],
// begin[l + 1]).  A refit runs the levels deepest first, one launch each.  Returns a refusal when
// a level is saturated (255: the tree is deeper than levels are recorded for), empty when fine.
std::string refit_levels(const uint8_t* level, uint32_t n_nodes, std::vector<uint32_t>& order,
                         std::vector<uint32_t>& begin);

// The rebuild (wgt_rebuild_triangles and its device form).  Its argument checks after
// the context and the scene, in the calls' order, for the leaf target `leaf` (RebuildLeafFromEnv): null,
// n_tris == 0, more than rebuild_max_tris(leaf), then the alignment rule of the device records (16
// bytes; the host form passes align = false).  Each returns the refusal's text, empty when fine.
std::string check_rebuild_records(const void* tris, uint32_t n_tris, uint32_t leaf, bool align);
// The specification's tree (BuildMortonBvh) under the origin-bound rule of build_bvh, and
// wgt_bvh_build_morton: the tree an upload of any scene whose lights, quads and spheres lie within
// the triangles' extent, followed by a rebuild to these triangles, holds.
std::string morton_bvh(const wgt_triangle* tris, uint32_t n_tris, double extent, BvhOut& bvh,
                       std::vector<uint32_t>* level_count);
std::string morton_for_export(const wgt_triangle* tris, uint32_t n_tris, BvhOut& bvh);
// The nodes a rebuilt tree of n_tris triangles can have at the most: every node has two slots or
// more and every leaf a triangle or more, so there are fewer nodes than triangles.
uint32_t rebuild_node_cap(uint32_t n_tris);
// The device layout of a tree of its own allocation (a rebuild's): the five tree parts of ScenePart
// for n_nodes nodes and n_tris triangles, each 256-B aligned; returns the bytes, fills off[kPartNodes..].
size_t tree_layout(uint32_t n_tris, uint32_t n_nodes, size_t off[]);
// Points sc's five tree parts into the allocation at `base` (bind_scene's tree half).
void bind_tree(DevScene& sc, const size_t off[], const void* base);
// The build's scratch: the sort's keys and values twice, two level lists, a level's cuts, counts and
// child offsets, the centres' bounds and the reduced counts, then rocprim's temporary storage.
struct RebuildScratch {
  size_t key[2], val[2], list[2], cuts, count, offset, bounds, stats, temp, bytes;
};
RebuildScratch plan_rebuild_scratch(uint32_t n_tris, size_t temp_bytes);
// What the tree's counts decide of a scene, in one statement for an upload (pack_scene) and a rebuild:
// n_tris, n_nodes, the traversal stack (stack_entries) and the k_render_ps form (ps_form_for); the
// counts are read from bvh (its arrays may be empty).
void plan_tree_form(const BvhOut& bvh, uint32_t n_tris, DevScene& sc);
// The refit's level lists of a tree numbered breadth-first (a rebuilt one): the order is the identity,
// begin the running sum of the level counts.
std::vector<uint32_t> level_begin_of(const std::vector<uint32_t>& level_count);

// The scene's device layout, each part 256-B aligned: quads (lights first), spheres, then the
// tree: both node forms stay resident (the compact one is 63% of the 128-B one; the launch
// picks one per frame, DevFrame::cnode), the triangle and shading records, the node levels
enum ScenePart { kPartQuads, kPartSpheres, kPartNodes, kPartTris, kPartShade, kPartCNodes, kPartLevel, kSceneParts };
struct ScenePlan {
  std::vector<char> host;   // the whole allocation's bytes, padding zero
  size_t off[kSceneParts];  // of each part within it
  DevScene sc;              // every field but the pointers (bind_scene)
};
// Of inputs that passed wgt_upload_scene's checks, their tree (empty without triangles) and its DeviceImage.
ScenePlan pack_scene(const wgt_quad* lights, uint32_t n_lights, const wgt_quad* quads, uint32_t n_quads,
                     const wgt_sphere* spheres, uint32_t n_spheres, uint32_t n_tris, const BvhOut& bvh,
                     const BvhImage& image);
// Points sc's seven parts into the allocation at `base`.
void bind_scene(DevScene& sc, const size_t off[kSceneParts], const void* base);

// The denoiser (wgt_denoise, wgt_denoise_async).  Its defaults; the workspace of a
// W x H image in bytes, 0 for a size the calls refuse (DenoisePlan states the layout); and the calls'
// checks after the context, in their order, each returning the refusal's text, empty when fine:
// null input, guides and required guide fields, both outputs null, the size, the parameters (null:
// the defaults); then of the async form the workspace: null, alignment, size.
wgt_denoise_params denoise_defaults();
size_t denoise_workspace_bytes(uint32_t W, uint32_t H);
std::string check_denoise_args(const wgt_denoise_params* params, uint32_t W, uint32_t H, const void* in,
                               const wgt_hit_buffers* guides, const void* out32, const void* out8);
std::string check_denoise_workspace(const void* ws, size_t ws_bytes, uint32_t W, uint32_t H);
// Of arguments that passed the checks: the workspace layout, each pass's kz in the fp32 operations of
// the specification, and the largest step that runs LDS-tiled (WGT_DENOISE_TILED_STEP, at most 16).
DenoisePlan plan_denoise(const wgt_denoise_params& params, uint32_t W, uint32_t H);

// The variance-guided denoiser (wgt_denoise_variance, wgt_denoise_variance_async).  Its
// defaults; its workspace (wgt_denoise's size and limits); and the calls' checks after the context, in
// their order, each returning the refusal's text, empty when fine: null state or guides; a null
// state->rgba32f, state->len or state->moments; a null required guide; both colour outputs null; the
// size; the parameters (null: the defaults; NaN is refused); then of the async form the workspace:
// null, alignment, size.  No pointer is dereferenced but the structs' own.
wgt_denoise_variance_params denoise_variance_defaults();
size_t denoise_variance_workspace_bytes(uint32_t W, uint32_t H);
std::string check_denoise_variance_args(const wgt_denoise_variance_params* params, uint32_t W, uint32_t H,
                                        const wgt_temporal_state* state, const wgt_hit_buffers* guides,
                                        const void* out32, const void* out8);
std::string check_denoise_variance_workspace(const void* ws, size_t ws_bytes, uint32_t W, uint32_t H);
// Of arguments that passed the checks: the workspace layout, each pass's kz (kz[0] = 1 / sigma_pos^2)
// in the fp32 operations of the specification, min_history as a float, and the largest step that runs
// LDS-tiled (WGT_DENOISE_TILED_STEP, at most 16).
DenoiseVariancePlan plan_denoise_variance(const wgt_denoise_variance_params& params, uint32_t W, uint32_t H);

// Temporal accumulation (wgt_temporal_accumulate, wgt_temporal_accumulate_async).
// Its defaults, and the calls' checks after the context, in their order, each returning the
// refusal's text, empty when fine: null input, camera, guides, out, out->rgba32f, out->len; a null
// required guide; the first-frame triple (prev, guides_prev, cam_prev all null or all set), then
// prev's and guides_prev's required fields and moments in prev and out alike; the size (the
// denoiser's limits); the parameters (null: the defaults); the cameras (check_frame_args with spp 1);
// an out buffer overlapping the prev buffer of the same name.  No pointer is dereferenced but the
// structs' own.
wgt_temporal_params temporal_defaults();
std::string check_temporal_args(const wgt_temporal_params* params, uint32_t W, uint32_t H, const wgt_camera_param* cam,
                                const wgt_camera_param* cam_prev, const void* in, const wgt_hit_buffers* guides,
                                const wgt_temporal_state* prev, const wgt_hit_buffers* guides_prev,
                                const wgt_temporal_state* out);
// wgt_temporal_accumulate_motion's: the same checks in the same order, with the
// motion buffers' right after the first-frame triple: when there is a previous frame, a null motion,
// motion->pos_prev or motion->norm_prev; on the first frame motion is not looked at.
std::string check_temporal_motion_args(const wgt_temporal_params* params, uint32_t W, uint32_t H,
                                       const wgt_camera_param* cam, const wgt_camera_param* cam_prev, const void* in,
                                       const wgt_hit_buffers* guides, const wgt_motion_buffers* motion,
                                       const wgt_temporal_state* prev, const wgt_hit_buffers* guides_prev,
                                       const wgt_temporal_state* out);
// wgt_motion_reproject's checks after the context and the scene, in their order: no snapshot since
// the last upload; null guides or a null required guide (prim, pos, norm, flags); null out or a null
// plane; n outside 1..kMotionMaxRecords.
std::string check_motion_reproject_args(bool has_snapshot, uint32_t n, const wgt_hit_buffers* guides,
                                        const wgt_motion_buffers* out);
// Of arguments that passed the checks (cam_prev null: the first-frame form): each camera's
// projection constants in the fp32 operations of the specification, from make_frame.
TemporalCam temporal_camera(const wgt_camera_param& cam, uint32_t W, uint32_t H);
// The sampled renders and G-buffers (wgt_render_tile_sampled and the like).  Their
// checks are the plain calls' in the plain calls' order with the camera's spp taken as 1
// (sampled_camera: cam->spp is ignored), then this one: a null sample map.  A map value cannot be
// out of range: a side is one uint8_t.
wgt_camera_param sampled_camera(const wgt_camera_param& cam);
const char* check_sample_map(const void* map);
// The table of each side's constants that the sampled kernels read (SampleArgs::tab), kSampleBins
// rows of (recip_sqrt_spp, fspp, inv_fspp, 0): make_frame's own expressions for spp = k * k, so the
// bits are the host's for that spp.
void sample_constants(float (*out)[4]);

// The sample-map planner (wgt_sample_plan, wgt_sample_plan_async).  Its defaults; its
// workspace in bytes, 0 for a size the calls refuse; and the calls' checks after the context, in their
// order, each returning the refusal's text, empty when fine: null state; a null state->len or
// state->moments; a null map; the size (the denoisers' limits); the parameters (null: the defaults;
// NaN is refused) in the struct's order; then of the async form the workspace: null, alignment, size.
// No pointer is dereferenced but the structs' own.
wgt_sample_plan_params sample_plan_defaults();
size_t sample_plan_workspace_bytes(uint32_t W, uint32_t H);
std::string check_sample_plan_args(const wgt_sample_plan_params* params, uint32_t W, uint32_t H,
                                   const wgt_temporal_state* state, const void* map_out);
std::string check_sample_plan_workspace(const void* ws, size_t ws_bytes, uint32_t W, uint32_t H);
// Of arguments that passed the checks: the parameters as the kernels compare them, the budget
// B = floor(budget_spp * W * H) in double (saturated at 2^64 - 1), and the workspace layout.
SamplePlan plan_sample_plan(const wgt_sample_plan_params& params, uint32_t W, uint32_t H);
// The budget rule on a histogram of the dilated sides (what k_sp_cap computes on the device): the
// largest cap c in [side_min, side_max] whose total (sample_plan_total) is at most the budget,
// side_min when none is; side_max without a budget.  total: the map's sum of k^2 under that cap.
uint32_t sample_plan_cap(const SamplePlan& plan, const uint32_t* bins, uint64_t& total);
TemporalPlan plan_temporal(const wgt_temporal_params& params, uint32_t W, uint32_t H, const wgt_camera_param& cam,
                           const wgt_camera_param* cam_prev);

// The synchronous image passes (wgt_sample_plan, wgt_denoise, wgt_temporal_accumulate and its motion
// form, wgt_denoise_variance) stage their host buffers through one device allocation of the call's own.
// Its layout: the parts in order, each kDenoiseAlign-aligned, of `bytes` bytes (0: absent), uploaded from
// `src` before the pass and fetched to `dst` after it (null: not).  `what` words a failed upload's refusal.
struct StagePart {
  size_t bytes;
  const void* src;
  void* dst;
};
struct StageLayout {
  static constexpr int kMaxParts = 17;  // the temporal accumulation's
  const char* what = "";
  int n = 0;
  StagePart part[kMaxParts] = {};
  size_t off[kMaxParts + 1] = {};  // off[n]: the allocation's bytes
  size_t bytes() const { return off[n]; }
  // part k of the allocation at `base`; null for no bytes, which the asynchronous forms read as absent
  void* at(void* base, int k) const { return part[k].bytes ? (char*)base + off[k] : nullptr; }
};
// The four layouts, of arguments that passed the calls' checks (no pointer is dereferenced but the structs'
// own); the enums name the parts.  A pass that works in place fetches its rgba32f from the input image's part.
enum SamplePlanStage { kSpsLen, kSpsMom, kSpsMap, kSpsTotal, kSpsWs, kSpsParts };
StageLayout stage_sample_plan(uint32_t W, uint32_t H, const wgt_temporal_state& state, void* map_out, void* total_out);
enum DenoiseStage { kDnsIn, kDnsPrim, kDnsPos, kDnsNorm, kDnsCol, kDnsFlags, kDnsOut8, kDnsWs, kDnsParts };
StageLayout stage_denoise(uint32_t W, uint32_t H, const void* in, const wgt_hit_buffers& guides, void* out32, void* out8);
// prev null: the first frame (guides_prev and motion are then not looked at); motion null: the plain form
enum TemporalStage { kTpsIn, kTpsPrim, kTpsPos, kTpsNorm, kTpsFlags, kTpsPrevRgba, kTpsPrevLen, kTpsPrevMom, kTpsPPrim,
                     kTpsPPos, kTpsPNorm, kTpsPFlags, kTpsMPos, kTpsMNorm, kTpsLen, kTpsMom, kTpsOut8, kTpsParts };
static_assert(kTpsParts == StageLayout::kMaxParts, "the longest list");
StageLayout stage_temporal(uint32_t W, uint32_t H, const void* in, const wgt_hit_buffers& guides,
                           const wgt_motion_buffers* motion, const wgt_temporal_state* prev,
                           const wgt_hit_buffers* guides_prev, const wgt_temporal_state& out, void* out8);
enum DenoiseVarianceStage { kDvsIn, kDvsLen, kDvsMom, kDvsPrim, kDvsPos, kDvsNorm, kDvsCol, kDvsFlags, kDvsOut8, kDvsVar,
                            kDvsWs, kDvsParts };
StageLayout stage_denoise_variance(uint32_t W, uint32_t H, const wgt_temporal_state& state, const wgt_hit_buffers& guides,
                                   void* out32, void* out8, void* variance_out);

// The closest-point queries (wgt_nearest_points and its forms).  Their own checks
// after the context, the scene and n == 0, in the calls' order: null points; null out or an out without
// a field; n above kNearestMaxPoints, which no uint32_t is: the ray queries put no limit on n, and the
// kernel's 64-bit plane offsets need none.  Returns the refusal's text, null when fine.
constexpr uint64_t kNearestMaxPoints = 0xffffffffull;
const char* check_nearest_args(const void* points, const wgt_nearest_buffers* out, uint64_t n);
// What the synchronous form stages in the context's scratch for the fields `out` asks for: the byte
// counts of the points, the limits (0 without a radius), prim, dist, and pos | uv as one buffer with uv
// at float offset uv_at.
struct NearestStage {
  size_t points, limits, prim, dist, vec, uv_at;
};
NearestStage plan_nearest_stage(const wgt_nearest_buffers& out, bool has_radius, uint32_t n);
// wgt_nearest_points_spec: the definition by brute force (wgt_nearest.h) over tris[0..n_tris) in index
// order for the n points, ids first_prim + index; writes the fields `out` asks for.
void nearest_points_spec(const wgt_triangle* tris, uint32_t n_tris, uint32_t first_prim, const float* points,
                         const float* max_dist, uint32_t n, const wgt_nearest_buffers& out);

// The radiance queries (wgt_trace_radiance and its forms).  Their own checks after the
// context, the scene and n == 0, in the calls' order: null rays; null out or an out without a field;
// samples above kRadianceMaxSamples.  Returns the refusal's text, null when fine.
const char* check_radiance_args(const void* rays, const wgt_radiance_buffers* out, uint64_t samples);
// What the synchronous form stages in the context's scratch for the fields `out` asks for, in bytes:
// the rays, the seeds (0 without), rgb, prim and seed_out (0: not asked for).
struct RadianceStage {
  size_t rays, seeds, rgb, prim, seed_out;
};
RadianceStage plan_radiance_stage(const wgt_radiance_buffers& out, bool has_seeds, uint32_t n);
// The launch's uniform arguments and its form, from the decision the render launch takes (WGT_KERNEL,
// WGT_CNODE, the scene's ps_waves and the phase knobs of make_frame): the persistent phase-split kernel
// for a scene with triangles unless WGT_KERNEL=1, when the ray queue's 32-bit counter holds n and a
// refill of each of `resident` waves; the flat kernel otherwise.  Returns a refusal when the scene's
// launch form keeps fewer LDS stack entries than the tree needs (the parked form, WGT_PARK, which the
// radiance kernel does not have): such a launch is never queued.  Empty when fine.
std::string plan_radiance(const DevScene& sc, uint32_t seed0, uint32_t samples, uint32_t n, uint32_t resident,
                          RadianceArgs& a);

// The multi-hit queries (wgt_trace_multi_hits and its forms).  Their own checks after
// the context, the scene and n == 0, in the calls' order: null rays; null out or an out without a field;
// unknown flag bits; k outside 1..WGT_MULTI_HIT_MAX_K when prim or dist is asked for (with count alone k
// is ignored).  Returns the refusal's text, null when fine.
const char* check_multi_hit_args(const void* rays, const wgt_multi_hit_buffers* out, uint64_t k, uint64_t flags);
// What the synchronous form stages in the context's scratch for the fields `out` asks for, in bytes:
// the rays, the limits (0 without), count, and prim and dist of k planes each (0: not asked for).
struct MultiHitStage {
  size_t rays, limits, count, prim, dist;
};
MultiHitStage plan_multi_hit_stage(const wgt_multi_hit_buffers& out, bool has_limit, uint32_t n, uint32_t k);
// The launch: the count form when out.count is asked for, else the cull form; k = 0 when neither prim nor
// dist is asked for; the dynamic LDS of the scene's stack and the lists.  Returns a refusal, not a launch, when that LDS exceeds one workgroup's (or k is out of
// range, which check_multi_hit_args refuses first); empty when fine.
std::string plan_multi_hit(const DevScene& sc, const wgt_multi_hit_buffers& out, uint32_t n, uint32_t k,
                           uint32_t flags, MultiHitPlan& p);

// The k-nearest and within-radius closest-point queries (wgt_nearest_k_points and its forms; DESIGN.md
// §4.16).  Their own checks after the context, the scene and n == 0, in the calls' order: null points;
// null out or an out without a field; n above kNearestMaxPoints; k outside 1..WGT_NEAREST_MAX_K when a
// list field (prim, dist, pos, uv) is asked for (with count alone k is ignored).  Returns the refusal's
// text, null when fine.
const char* check_nearest_k_args(const void* points, const wgt_nearest_k_buffers* out, uint64_t n, uint64_t k);
// What the synchronous form stages in the context's scratch for the fields `out` asks for, in bytes: the
// points, the limits (0 without a radius), count, prim and dist of k planes each, and pos | uv as one
// buffer of 3k and 2k planes with uv at float offset uv_at (0: not asked for).
struct NearestKStage {
  size_t points, limits, count, prim, dist, vec, uv_at;
};
NearestKStage plan_nearest_k_stage(const wgt_nearest_k_buffers& out, bool has_radius, uint32_t n, uint32_t k);
// The launch: the count form when out.count is asked for, else the cull form; k = 0 when no list field is
// asked for; two list words per entry, three when pos or uv is asked for; the count form's node step sorted
// when it fills a list (WGT_NEAREST_K_SORT = 0 / 1 forces slot order / nearest first); the dynamic LDS of the scene's
// stack and the lists, sized for the call's k.  Returns a refusal, not a launch, when that LDS exceeds one
// workgroup's (or k is out of range, which check_nearest_k_args refuses first); empty when fine.
std::string plan_nearest_k(const DevScene& sc, const wgt_nearest_k_buffers& out, uint32_t n, uint32_t k,
                           NearestKPlan& p);
// wgt_nearest_k_points_spec: the definition by brute force (wgt_nearest_k.h) over tris[0..n_tris) in index
// order for the n points, ids first_prim + index; writes the fields `out` asks for.  k as plan_nearest_k
// takes it (ignored without a list field).
void nearest_k_points_spec(const wgt_triangle* tris, uint32_t n_tris, uint32_t first_prim, const float* points,
                           const float* max_dist, uint32_t n, uint32_t k, const wgt_nearest_k_buffers& out);

// The triangle overlap queries (wgt_overlap_triangles and its forms).  Their own checks
// after the context, the scene and n == 0, in the calls' order: null query triangles; null out; an out
// without a field; k above WGT_OVERLAP_MAX_K; k == 0 with prim asked for; k > 0 without prim.  Returns the
// refusal's text, null when fine.
const char* check_overlap_args(const void* query, const wgt_overlap_buffers* out, uint64_t k);
// The launch, of any arguments: those checks first (the kernel's list indices rely on them, whoever
// calls), then the form (the any form iff hit is the only field asked for), k, and the dynamic LDS of the
// scene's stack and the lists, sized for the call's k.  Returns a refusal, not a launch, when a check fails
// or that LDS exceeds one workgroup's; empty when fine.  p.lds is 0 on a refusal.
std::string plan_overlap(const DevScene& sc, const void* query, const wgt_overlap_buffers* out, uint32_t n, uint64_t k,
                         OverlapPlan& p);
// What the synchronous form stages, as the synchronous image passes do (StageLayout): the nine planes of
// the query up, the fields `out` asks for down.
enum OverlapStage { kOvsQuery, kOvsHit, kOvsCount, kOvsPrim, kOvsParts };
StageLayout stage_overlap(const float* query, const wgt_overlap_buffers& out, uint32_t n, uint32_t k);
// wgt_overlap_triangles_spec: the definition by brute force (wgt_overlap.h) over tris[0..n_tris) in index
// order for the n query triangles (nine planes of n floats), ids first_prim + index, each triangle's box
// from tri_box; it culls nothing.  Writes the fields `out` asks for; k as plan_overlap takes it.
void overlap_triangles_spec(const wgt_triangle* tris, uint32_t n_tris, uint32_t first_prim, const float* query,
                            uint32_t n, uint32_t k, const wgt_overlap_buffers& out);

// The self-intersection queries (wgt_overlap_self and its forms).  Their own checks after the
// context, the scene and a scene without triangles, in the calls' order: null out; an out without a field; k
// above WGT_OVERLAP_MAX_K; k == 0 with prim asked for; k > 0 without prim.  A null index buffer is an answer
// (nothing is adjacent), not a fault.  Returns the refusal's text, null when fine.
const char* check_overlap_self_args(const wgt_overlap_buffers* out, uint64_t k);
// The launch, of any arguments: those checks first (the kernel's list indices rely on them, whoever calls),
// then one lane per resident triangle (n = sc.n_tris: the kernel reads record i < n and writes at ids below
// n), the form (the any form iff hit is the only field asked for), k, and the dynamic LDS of the scene's
// stack and the lists (overlap_lds_bytes).  Returns a refusal, not a launch, when a check fails or that LDS
// exceeds one workgroup's; empty when fine.  p.lds is 0 on a refusal.
std::string plan_overlap_self(const DevScene& sc, const wgt_overlap_buffers* out, uint64_t k, OverlapSelfPlan& p);
// What the synchronous form stages (StageLayout): the index buffer up (no part without one), the fields `out`
// asks for down, each sized by the scene's triangle count.
enum OverlapSelfStage { kOssIndex, kOssHit, kOssCount, kOssPrim, kOssParts };
StageLayout stage_overlap_self(const uint32_t* indices, const wgt_overlap_buffers& out, uint32_t n_tris, uint32_t k);
// wgt_overlap_self_spec: the definition by brute force (wgt_overlap_self.h) over every ordered pair of
// tris[0..n_tris), ids first_prim + index, each triangle's box from tri_box; it culls nothing.  indices: 3 *
// n_tris labels or null.  Writes the fields `out` asks for; k as plan_overlap_self takes it.
void overlap_self_spec(const wgt_triangle* tris, uint32_t n_tris, uint32_t first_prim, const uint32_t* indices,
                       uint32_t k, const wgt_overlap_buffers& out);

// The pixel queue's order across launches of one view.  The LPT order of
// a launch depends on its view (scene, camera, frame and tile geometry, knobs), not on its seeds, and
// it shapes the schedule only: any permutation of [0, nb) renders the same pixels.  So the context
// computes it once per view, into one of kOrderBufs buffers of its own that later launches of the
// view read, instead of once per launch into the launch's workspace.
// The knobs, read per launch like make_frame's: WGT_PQ_REUSE (1; 0: every launch orders itself) and
// WGT_PQ_REFINE, the side of the pre-pass whose order is kept (the launch's own pre-pass runs at pq_lpt).
struct OrderKnobs {
  uint32_t reuse, refine;
};
OrderKnobs order_knobs();
// What a launch looks at, without its seeds: make_frame's frame before launch_render fills in its
// pointers, the launch's 8x8 block count, the planner's scene epoch (OrderPlanner::epoch) and the tile
// list's identity: a hash of the host tiles' origins (order_tiles_hash) or the device pointer.
struct OrderKey {
  DevFrame fr;
  uint32_t nb, refine;
  uint64_t epoch, tiles;
  uint32_t tiles_by_ptr;
};
OrderKey order_key(const DevFrame& fr, uint32_t nb, const OrderKnobs& knobs, uint64_t epoch, uint64_t tiles,
                   bool tiles_by_ptr);
bool same_view(const OrderKey& a, const OrderKey& b);
uint64_t order_tiles_hash(const wgt_tile* tiles, uint32_t n);  // x0 and y0 of each; not seed, not frame
// The launch's 8x8 block count as tile_grid computes it (0: more than the kernels' 32-bit slots hold).
uint32_t order_blocks(const DevFrame& fr);
// LPT is on for this launch (launch_render's rule for a plain launch of the persistent kernel).
bool order_lpt_on(const DevFrame& fr);
// The launch may share an order: WGT_PQ_REUSE set, no sample map (a sampled frame's costs follow its
// map, which changes per frame), a block count the kernels accept, LPT on.
bool order_eligible(const DevFrame& fr, const OrderKnobs& knobs, bool sampled, uint32_t nb);

constexpr int kOrderBufs = 2;
enum OrderMode : uint32_t {
  kOrderToday,   // pre-pass at pq_lpt and the sort into the workspace's own order: a launch on its own
  kOrderRefine,  // pre-pass at `side` and the sort into shared buffer `buf`, which the main kernel reads
  kOrderReuse    // no pre-pass, no sort: the main kernel reads shared buffer `buf`
};
struct OrderPlan {
  OrderMode mode;
  int buf;        // the shared buffer (REFINE, REUSE), else -1
  uint32_t side;  // the pre-pass's side (TODAY: pq_lpt; REUSE: 0)
};
// The planner: one per context, called once per launch of the persistent kernel, in launch order.
// It calls no HIP function: whether a workspace slot's last launch has ended is `slot_done`'s answer
// (the runtime's is hipEventQuery on the slot's event).
class OrderPlanner {
 public:
  static constexpr int kSlots = 4;  // workspace slots (wgt_ctx::kMaxWsSlots)
  // key: the launch's view.  eligible: order_eligible's answer; any other launch is TODAY and ends
  // the run of consecutive sightings.  slot: the workspace slot the launch runs on.
  // First sighting of a view: TODAY.  Second consecutive one:
  // REFINE when a shared buffer has no reader left in flight, else TODAY (and the next sighting tries
  // again).  A launch of the current view: REUSE.
  template <class SlotDone>
  OrderPlan plan(const OrderKey& key, bool eligible, int slot, SlotDone&& slot_done) {
    const uint32_t lpt = key.fr.pq_lpt;
    if (!eligible || slot < 0 || slot >= kSlots) {
      seen_ = false;
      ++n_today_;
      return OrderPlan{kOrderToday, -1, lpt};
    }
    if (cur_ >= 0 && same_view(key, cur_key_)) {
      readers_[cur_] |= 1u << slot;
      seen_ = true;
      last_ = key;
      ++n_reuse_;
      return OrderPlan{kOrderReuse, cur_, 0u};
    }
    if (seen_ && same_view(key, last_)) {
      // a buffer may be rewritten once every launch that read it has ended; the other buffer than the
      // current one first, so that a current order is dropped only when it has to be
      for (int i = 0; i < kOrderBufs; ++i) {
        const int b = cur_ >= 0 ? (cur_ + 1 + i) % kOrderBufs : i;
        uint32_t left = 0;
        for (int s = 0; s < kSlots; ++s)
          if ((readers_[b] >> s & 1u) && !slot_done(s)) left |= 1u << s;
        readers_[b] = left;
        if (left) continue;
        readers_[b] = 1u << slot;
        cur_ = b;
        cur_key_ = key;
        // within [pq_lpt, sqrt_spp - 1]: an eligible launch has sqrt_spp > pq_lpt
        cur_side_ = std::min(std::max(key.refine, lpt), key.fr.sqrt_spp - 1u);
        ++n_refine_;
        return OrderPlan{kOrderRefine, b, cur_side_};
      }
    }
    seen_ = true;
    last_ = key;
    ++n_today_;
    return OrderPlan{kOrderToday, -1, lpt};
  }
  // The scene changed (upload, refit, rebuild) or the caller asked (wgt_order_reset): no order is
  // current and the next launch is a first sighting.  The buffers' readers stay: they are launches.
  void invalidate();
  // plan() would try a REFINE for this launch (its second consecutive sighting, not the kept view):
  // the runtime makes room in the shared buffers before it plans, and only then.
  bool refine_due(const OrderKey& key, bool eligible) const;
  // The buffers were reallocated after every launch of the context had ended: no order is kept and
  // no reader is left; the scene epoch and the run of sightings stay.
  void buffers_reset();
  // The launch that plan() planned could not be queued: its order is not to be relied on.
  void launch_failed(const OrderPlan& p);
  uint64_t epoch() const { return epoch_; }
  int current() const { return cur_; }
  const OrderKey& current_key() const { return cur_key_; }
  uint32_t current_side() const { return cur_side_; }
  uint32_t readers(int buf) const { return readers_[buf]; }
  void counts(uint64_t& today, uint64_t& refine, uint64_t& reuse, uint64_t& invalidations) const;

 private:
  OrderKey last_{}, cur_key_{};
  bool seen_ = false;
  int cur_ = -1;
  uint32_t cur_side_ = 0;
  uint32_t readers_[kOrderBufs] = {};
  uint64_t epoch_ = 1;
  uint64_t n_today_ = 0, n_refine_ = 0, n_reuse_ = 0, n_invalid_ = 0;
};

}  // namespace wgt
