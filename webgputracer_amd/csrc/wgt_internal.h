// wgt_internal.h — device-side data layout shared by the kernel TU and the
// runtime TU (not part of the public ABI).
//
// HBM layout of a scene:
//   quads   : lights then quads, 96-B reference records (6 x float4) — read with
//             wave-uniform (scalar) loads, 1.7 KB for the Cornell box
//   spheres : 32-B reference records (2 x float4)
//   nodes   : BVH4 nodes, 128 B (8 x float4, one cache line), root = node 0,
//             see wgt_geom.h
//   tris    : leaf-ordered Moller-Trumbore records, 64 B (4 x float4) carrying
//             the padded triangle box, see wgt_geom.h
//   tshade  : per ORIGINAL triangle, 32 B: (face_norm.xyz, emissive), (col.xyz, 0)
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/wgt_api.h"

namespace wgt {

constexpr int kBlock = 64;        // one wave per block: 8x8 pixels
// Per-lane traversal stack in LDS, stride kBlock (conflict-free), sized per scene
// at launch (dynamic LDS) to the builder's exact worst case DevScene::stack, so it
// cannot overflow and needs no spill path.  kMaxBvhDepth bounds the SAH BVH2 the
// BVH4 is collapsed from; kStackMax bounds the builder's stack need: + 1 parking
// slot, so that LDS (160 KB per CU) admits 5 waves per SIMD (4 SIMDs per CU):
// 32 entries = 8 KB per wave.  k_render_ps stores 3-byte entries when the tree's
// refs fit them (6 KB per wave): 6 waves per SIMD at 80 VGPRs (DESIGN.md §4.2,
// DevScene::ps_waves).  kStackNarrow is the optional narrow collapse (WGT_NARROW).
constexpr int kMaxBvhDepth = 24;
constexpr int kStackMax = 31;
constexpr int kStackNarrow = 25;
// k_render_ps on scenes without triangles (no traversal, no stack): its register budget
constexpr int kPsWavesNoTris = 8;
constexpr uint32_t kStack24Nodes = 1u << 16;  // 128-B node byte offsets < 2^23
constexpr uint32_t kStack24Tris = 1u << 20;   // leaf refs ~(first << 3 | count - 1) >= -2^23
// Parked traversal state per lane (wgt_trav_ps.h Park): 1/d (3), slab offsets (3), best t,
// best index, node ref, stack top | global depth << 16, open leaf (offset | count)
constexpr uint32_t kParkWords = 11;
// The smallest LDS stack the parked kernel runs with: a node step needs 4 free entries
// above the top (3 pushes and a parked leaf), and a ray's root step, which pushes at most
// 4, must leave its top within that bound (top <= cap - 4), so a new ray never starts
// past it
constexpr uint32_t kMinPsCap = 8;

// Dynamic LDS bytes of a traversal kernel launch (k_render and the ray queries: 4-byte entries).
constexpr size_t stack_lds_bytes(uint32_t stack) { return (size_t)stack * kBlock * sizeof(int); }

// The launch form of k_render_ps for a scene (ps_form): with the frame's node form (node_form)
// it names the instantiation (ps_kernel), and it alone fixes the launch's dynamic LDS (ps_lds).
struct PsForm {
  bool tris;       // the scene has triangles (else no traversal phase, at kPsWavesNoTris)
  uint32_t waves;  // per SIMD (DevScene::ps_waves)
  bool park;       // parked traversal state (DevScene::ps_park)
  uint32_t cap;    // LDS stack entries per lane: DevScene::ps_cap when parked, else the whole stack
  // the phase-threshold defaults (DevFrame::ps_to_trav, ps_to_service), swept per wave budget
  // (profiles/sweeps/r01_sweep_compact_knobs.jsonl)
  constexpr uint32_t to_trav() const { return waves >= 6 ? 16u : 18u; }
  constexpr uint32_t to_service() const { return waves >= 6 ? 14u : 16u; }
};
// The dynamic LDS of one wave of k_render_ps, in bytes: f.cap stack entries per lane of `entry`
// bytes (3 at 6 or more waves per SIMD, Stack24: the 16-bit array, then the high bytes at `hi`;
// else 4, Stack32), then at `park` the lanes' kParkWords words when the form parks.  The launch,
// the occupancy query (ps_resident_waves) and the kernel's carve-up all read this one statement.
struct PsLds {
  uint32_t entry, hi, park, total;
};
constexpr PsLds ps_lds(const PsForm& f) {
  const uint32_t entry = f.waves >= 6 ? 3u : 4u, stack = f.cap * kBlock * entry;
  return PsLds{entry, f.cap * kBlock * 2u, stack, stack + (f.park ? kParkWords * kBlock * 4u : 0u)};
}
constexpr size_t kLdsPerCu = 160 * 1024;
static_assert(ps_lds({true, 5, false, kStackMax + 1}).total * 5 * 4 <= kLdsPerCu, "5 waves per SIMD");
static_assert(stack_lds_bytes(kStackNarrow + 1) * 6 * 4 <= kLdsPerCu, "6 waves per SIMD");
static_assert(ps_lds({true, 6, false, kStackMax + 1}).total * 6 * 4 <= kLdsPerCu, "6 waves per SIMD, 3-byte entries");
// LDS entries the parked kernel can hold at its wave budget: the stack and the parked words
// of 4 * waves one-wave workgroups per CU within kPsLdsPerCu.  Measured (profiles/r04/
// lds_sweep_*.jsonl): 24 workgroups per CU run at full speed with 6,272 B each and lose 8-20 %
// from 6,464 B on, although the occupancy API still reports 24 (and 160 KiB would hold 24 of
// 6,656 B): the usable budget lies between 24 x 6,400 and 24 x 6,656 B, so 150 KiB is taken
constexpr size_t kPsLdsPerCu = 150 * 1024;
constexpr uint32_t ps_cap_max(uint32_t waves) {
  const PsLds none = ps_lds({true, waves, true, 0});  // the parked words alone
  return (uint32_t)((kPsLdsPerCu / (4 * waves) - none.total) / (kBlock * none.entry));
}
static_assert(ps_cap_max(6) == 18, "6 waves: 18 entries of 3 B beside the 11 parked words");
static_assert(ps_cap_max(5) == 19, "5 waves: 19 entries of 4 B");

struct DevScene {
  const float4* __restrict__ quads;   // n_lights + n_quads records
  const float4* __restrict__ spheres; // n_spheres records
  const float4* __restrict__ nodes;
  const float4* __restrict__ tris;
  const float4* __restrict__ tshade;
  const float4* __restrict__ cnodes;  // the same tree as 80-B compact records (wgt_geom.h)
  // the level of each BVH4 node (root 0), by node index: read by the instrumented (STATS) passes
  // only, to split node visits and traversal-step cycles by tree level
  const uint8_t* __restrict__ node_level;
  float cstep;                        // scene-wide decode step of the compact nodes (a power of two)
  float rcstep;                       // 1 / cstep
  float cbound;                       // the compact codes hold for ray origins with |coordinate| <= cbound
  uint32_t n_lights, n_quads, n_spheres, n_tris;
  uint32_t n_nodes;
  uint32_t last_sphere_emissive;
  float light_area;  // length(cross(lights[0].right, lights[0].up)) (path_tracer.wgsl:205)
  uint32_t stack;     // traversal stack entries per lane (>= 1)
  // k_render_ps waves per SIMD: 6 (3-byte stack entries, Stack24) when every ref of
  // the tree fits 24 bits (kStack24Nodes, kStack24Tris), else 5
  uint32_t ps_waves;
  // k_render_ps with parked traversal state (ps_park = 1): the
  // LDS holds ps_cap stack entries per lane (<= stack) plus kParkWords words of the
  // lane's traversal state; entries beyond ps_cap move to a per-lane global stack
  // (DevFrame::ps_spill) in the service phase.  ps_park = 0: the whole stack in LDS.
  uint32_t ps_park, ps_cap;
};
inline PsForm ps_form(const DevScene& sc) {
  return PsForm{sc.n_tris > 0, sc.ps_waves, sc.ps_park != 0, sc.ps_park ? sc.ps_cap : sc.stack};
}

// 1 / spp when spp is a power of two (exact in fp32: end_sample multiplies), else 0
inline float pow2_recip(uint32_t spp) { return (spp != 0u && (spp & (spp - 1u)) == 0u) ? 1.0f / (float)spp : 0.0f; }

// Per-frame camera constants of setup_camera_ray (path_tracer.wgsl:239-262),
// computed once on the host with the same fp32 operations (wgt_math.h).
struct DevFrame {
  float ox, oy, oz;    // origin
  float pox, poy, poz; // pixel_origin
  float dux, duy, duz; // pixel_delta_u
  float dvx, dvy, dvz; // pixel_delta_v
  float recip_sqrt_spp;
  float fspp;          // f32(camera.spp)
  float inv_fspp;      // 1 / fspp when spp is a power of two (exact), else 0
  uint32_t sqrt_spp;
  uint32_t W, H;
  uint32_t tw, th, n_tiles;
  // kernel selection and phase-split thresholds (k_render_ps): switch from the
  // service to the traversal phase once >= ps_to_trav lanes traverse, and back
  // once <= ps_to_service lanes still traverse.
  uint32_t kernel;  // 2 = the persistent phase-split kernel (default), else the simple one
  uint32_t ps_to_trav, ps_to_service;
  // a wave with fewer live pixels leaves the traversal phase at <= live *
  // ps_svc_frac / 64 traversing lanes (if lower): a sparse wave (the end of a
  // launch) would otherwise pay a service pass for every finished ray (0 = off)
  uint32_t ps_svc_frac;
  // speculative traversal: a triangle step runs when lanes with a pending leaf
  // number >= tri_ratio % of the lanes with a node to visit
  uint32_t tri_ratio;
  // BVH node form of k_render_ps: 0 = 128-B nodes, 1 = 80-B compact records, 2 = 80-B
  // compact records when the 128-B tree exceeds kCompactNodeBytes (default) (node_form)
  uint32_t cnode;
  // persistent k_render_ps: pixel slots of the launch (64 per 8x8 block), the
  // idle lanes that trigger a refill from the pixel queue, LPT ordering (0 = off,
  // n = order from an n*n-spp cost pre-pass),
  // the queue order (queue block q renders pixel block perm[q]; NULL = identity)
  // and the pre-pass cost per pixel block (set by launch_render)
  uint32_t n_slots, pq_refill, pq_lpt;
  uint32_t pq_lpt_all;  // the pre-pass renders all 64 pixels of each block (else the 16 at even x, y)
  uint32_t pq_svc_cost;  // pre-pass work units per ray started (a service iteration ~ 7 traversal steps)
  uint32_t pq_depth;     // the pre-pass's paths end at this depth (kRayDepth: the full path)
  // sampled launches: the pre-pass, which renders min(k, pq_lpt)^2 samples of a pixel of side k,
  // scales the pixel's work by k^2 / min(k, pq_lpt)^2 (1, the default) or leaves it (0)
  uint32_t pq_lpt_weight;
  const uint32_t* perm;
  uint32_t* cost;
  // parked k_render_ps (DevScene::ps_park): the global part of the lanes' stacks, entry e
  // of the lane (wave w, lane l) at ps_spill[e * ps_spill_stride + w * 64 + l] (launch_render)
  int* ps_spill;
  uint32_t ps_spill_stride;
  // (2^32 - 1) / d for the 8x8 blocks per tile row (bx) and per tile (bx * by) of the launch
  // (launch_render, launch_gbuffer): slot_setup's divisions by them (wgt_pixel.h tile_grid, udiv_by)
  uint32_t div_bx, div_bpt;
};
// DevFrame keeps its size: the instrumented parked 5-wave kernel allocated one more VGPR when the
// kernel arguments behind the frame moved by 16 bytes, so what the sampled
// kernels need comes as a last kernel argument of its own
static_assert(sizeof(DevFrame) == 176, "the kernel arguments after the frame keep their offsets");

// The sampled launches' own kernel argument, the last one (the SM instantiations; no other kernel
// reads it): the frame's sample map, one side k per pixel of the W x H frame, row-major, and the
// context's table of each side's constants, tab[k] = (recip_sqrt_spp, fspp, inv_fspp, 0) of
// spp = k^2 (host/launch_plan.h sample_constants).  map != null selects the sampled kernels
// (launch_render, launch_gbuffer); DevFrame::sqrt_spp and its three uniform constants are then not read.
struct SampleArgs {
  const uint8_t* map;
  const float4* tab;
};

enum {
  CNT_QUERIES = 0,
  CNT_TRACED,
  CNT_SAMPLES,
  CNT_NAN,
  CNT_NODES,
  CNT_TRIS,
  CNT_PIXELS,
  CNT_LOOP_WAVE,
  CNT_LOOP_LANE,
  CNT_TRAV_WAVE,
  CNT_TRAV_LANE,
  CNT_CYC_SERVICE,  // s_memtime cycles per wave spent in each phase (instrumented pass)
  CNT_CYC_TRAV,
  CNT_CYC_REFILL,  // service-phase regions (k_render_ps, instrumented pass)
  CNT_CYC_FINALISE,
  CNT_CYC_SHADE,
  CNT_CYC_CAMERA,
  CNT_CYC_QUADS,
  CNT_CYC_ROOT,
  CNT_STACK_SPILLS,   // parked k_render_ps: LDS stack overflows moved to the global stack
  CNT_STACK_REFILLS,  // ... and refills from it
  CNT_STACK_OVERFLOWS,  // ... and traversals park_fix ended on its overflow exit (a wrong pixel)
  // traversal phase by tree level (instrumented pass): lane visits of nodes at levels 1-2 (the
  // root's children and grandchildren; the root itself is visited in the service phase), and the
  // cycles of node steps, of node steps whose every visiting lane is at levels 1-2, and of
  // triangle steps
  CNT_TOP_NODES,
  CNT_CYC_NODE_STEPS,
  CNT_CYC_TOP_STEPS,
  CNT_CYC_TRI_STEPS,
  CNT_QUAD_REF,  // rays whose quad scan fell back to the reference scan (quad_scan_fast)
  CNT_N = 29
};

// Launchers implemented in wgt_kernels.hip
// k_render_ps runs persistent: at most `resident` waves (ps_resident_waves),
// lanes pulling pixel slots from a per-launch queue in LPT order (1-spp cost
// pre-pass + k_lpt_order), all stream-ordered on `stream`.
// ws: scheduling workspace of >= render_ws_bytes(sc, fr, resident) bytes, used in stream
// order (one launch in flight per workspace): the queues, the LPT costs and order, and the
// parked kernel's global stacks.
size_t render_ws_bytes(const DevScene& sc, const DevFrame& fr, uint32_t resident);
// ws_clean_nb: in, the block count whose queues and costs the workspace's previous LPT launch left
// zero (0: unknown, a memset clears them); out, the same for this launch
// sm: the sampled frame's map and table (sm.map null: the plain kernels, at fr's uniform spp)
// order: where the queue order of an LPT launch comes from (the context plans it per view,
// host/launch_plan.h OrderPlanner); a launch without LPT ignores it.
struct OrderArgs {
  uint32_t* shared = nullptr;  // the order, nb words of the context's, that the sort writes (prepass) and the
                               // main kernel reads; null: the workspace's own (a launch on its own)
  uint32_t side = 0;           // the pre-pass's samples per pixel are side^2 (0: fr.pq_lpt)
  bool prepass = true;         // the pre-pass and the sort run; else `shared` holds an order of these nb blocks
  hipEvent_t sorted = nullptr;  // recorded on the stream right after the sort (prepass; may be null)
};
hipError_t launch_render(const DevScene& sc, const DevFrame& fr, const SampleArgs& sm, const wgt_tile* d_tiles,
                         uchar4* out8, float4* out32, uint32_t* outhit,
                         unsigned long long* counters, uint32_t resident, void* ws, size_t ws_cap,
                         hipStream_t stream, uint32_t& ws_clean_nb, const OrderArgs& order = OrderArgs{});
// The node form k_render_ps reads for this scene and frame (DevFrame::cnode): 0 = 128-B
// nodes, 1 = 80-B compact records.
int node_form(const DevScene& sc, const DevFrame& fr);
// Waves of k_render_ps resident on the whole device for this scene's LDS stack.
hipError_t ps_resident_waves(const DevScene& sc, int device, uint32_t& waves);

// Launcher implemented in wgt_selftest.hip (wgt_selftest_math)
hipError_t launch_selftest_math(uint32_t n, uint32_t seed, unsigned long long* d_counts, hipStream_t stream);

// Launcher implemented in wgt_occlusion.hip
// out[i] = ray i hits a primitive closer than max_dist[i] (k_occluded; rays as launch_trace_hits').
hipError_t launch_occluded(const DevScene& sc, const float* d_rays, const float* d_max_dist, uint32_t n,
                           uint8_t* d_out, hipStream_t stream);

// Launchers implemented in wgt_hits.hip
// Record i = the whole closest hit of ray i (k_trace_hits; d_rays: six planes of n floats, origin
// x, y, z then direction x, y, z); out: device pointers, a null field is not written.  With prim
// and dist alone this is the closest-hit query (wgt_trace_rays).
hipError_t launch_trace_hits(const DevScene& sc, const float* d_rays, uint32_t n, const wgt_hit_buffers& out,
                             hipStream_t stream);
// The record of sample 0's camera ray of every pixel of the tile list (k_gbuffer; fr as
// launch_render's), at the render's pixel offsets; d_rays (may be null) receives those rays.
// sm as launch_render's: the G-buffer of a sampled frame needs its map (sample 0's jitter depends on the side).
hipError_t launch_gbuffer(const DevScene& sc, const DevFrame& fr, const SampleArgs& sm, const wgt_tile* d_tiles,
                          const wgt_hit_buffers& out, float* d_rays, hipStream_t stream);

// Launcher implemented in wgt_nearest.hip
// Record i = the scene's triangle nearest to point i (k_nearest; d_points: three planes of n floats;
// d_max_dist may be null: no radius); out: device pointers, a null field is not written.  d_counts
// (may be null) selects the counting instantiation: += node visits, triangle tests.
hipError_t launch_nearest(const DevScene& sc, const float* d_points, const float* d_max_dist, uint32_t n,
                          const wgt_nearest_buffers& out, unsigned long long* d_counts, hipStream_t stream);

// The scene limits of coordinates and of triangle edge components (host/launch_plan.h states why),
// here because the device check of moved triangles applies them as the host's check_scene_limits does.
constexpr double kCoordLimit = 1099511627776.0;  // 2^40
constexpr double kEdgeLimit = 1073741824.0;      // 2^30: triangle edges (Moller-Trumbore's short 1/det)

// Moved triangles as vertices on the device (wgt_update_vertices_device): n_verts x 3 floats;
// triangle i uses vertices index[3i .. 3i + 2], or 3i .. 3i + 2 when index is null.
struct MovedVerts {
  const float* verts;
  uint32_t n_verts;
  const uint32_t* index;
  uint32_t n_tris;
};
// What the device check of moved triangles reduces (launch_check_tris, launch_check_verts): both
// reductions are exact, so their results do not depend on the order of waves.
struct RefitCheck {
  unsigned long long extent_bits;  // max, over the triangles within the limits, of their scene_extent term:
                                   // a non-negative double's bits, which order as the values do
  uint32_t first_bad;              // min index of a triangle beyond the limits; kNoBadTriangle: none
  uint32_t pad;
};
constexpr uint32_t kNoBadTriangle = 0xffffffffu;  // every byte 0xff: one memset over first_bad and pad

// Launchers implemented in wgt_refit.hip: the refit of the resident tree to moved triangles, in
// this order on one stream, after every launch that reads the scene has ended.  They write the
// scene's tree parts (the pointers of sc are const for every other kernel).
// The records and shading records from the n_tris moved triangles (device array, original order).
hipError_t launch_refit_tris(const DevScene& sc, const wgt_triangle* d_moved, hipStream_t stream);
// The same from moved vertices (MovedVerts): each record as wgt_make_triangles builds it from the
// triangle's three vertices; the shading records keep their colour and emissive flag.
hipError_t launch_refit_verts(const DevScene& sc, const MovedVerts& in, hipStream_t stream);
// The device pass of wgt_update_triangles_device and wgt_update_vertices_device, before any of the
// above: *d_out (extent_bits 0 and first_bad kNoBadTriangle before the launch) = the lowest-numbered triangle beyond the scene
// limits (launch_plan.h check_triangle_limits; of the vertex form also one with an index >= n_verts,
// through which nothing is loaded) and the triangles' term of scene_extent.  They read the input
// alone, so they need no order with the launches that read the scene.
hipError_t launch_check_tris(const wgt_triangle* d_moved, uint32_t n_tris, RefitCheck* d_out, hipStream_t stream);
hipError_t launch_check_verts(const MovedVerts& in, RefitCheck* d_out, hipStream_t stream);
// The boxes of the `count` nodes d_order lists, one tree level (launch_plan.h refit_levels), after
// the level below it.
hipError_t launch_refit_nodes(const DevScene& sc, const uint32_t* d_order, uint32_t count, hipStream_t stream);
// *d_max_exp (zeroed by the caller) = the scene's step exponent - kCompactMinExp for the margin G.
hipError_t launch_refit_step(const DevScene& sc, double G, uint32_t* d_max_exp, hipStream_t stream);
// The node part of every compact record for that step and margin.
hipError_t launch_refit_compact(const DevScene& sc, float step, double G, hipStream_t stream);

}  // namespace wgt
