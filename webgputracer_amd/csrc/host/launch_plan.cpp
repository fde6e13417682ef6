// launch_plan.cpp — the host arithmetic behind the C-ABI's device calls (launch_plan.h).
#include "launch_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

namespace wgt {

bool finite_within(const float* v, int n, double lim) {
  for (int i = 0; i < n; ++i)
    if (!(std::fabs((double)v[i]) <= lim)) return false;  // NaN and inf fail too
  return true;
}

std::string check_scene_limits(const wgt_quad* lq, uint32_t nlq, const wgt_sphere* sp, uint32_t ns,
                               const wgt_triangle* tr, uint32_t nt) {
  for (uint32_t i = 0; i < nlq; ++i) {
    const wgt_quad& q = lq[i];
    if (!finite_within(q.pos, 3, kCoordLimit) || !finite_within(q.right, 3, kCoordLimit) ||
        !finite_within(q.up, 3, kCoordLimit) || !finite_within(&q.d, 1, kCoordLimit * 4.0))
      return "quad " + std::to_string(i) + ": position, edges and plane offset must be finite and within 2^40";
    const bool nan_norm = q.norm[0] != q.norm[0] || q.norm[1] != q.norm[1] || q.norm[2] != q.norm[2];
    if (!nan_norm && !finite_within(q.norm, 3, 2.0))
      return "quad " + std::to_string(i) + ": normal components must be within 2 (a unit normal) or NaN";
  }
  for (uint32_t i = 0; i < ns; ++i)
    if (!finite_within(sp[i].center, 3, kCoordLimit) || !finite_within(&sp[i].radius, 1, kCoordLimit))
      return "sphere " + std::to_string(i) + ": center and radius must be finite and within 2^40";
  for (uint32_t i = 0; i < nt; ++i) {
    const std::string bad = check_triangle_limits(tr[i], i);
    if (!bad.empty()) return bad;
  }
  return "";
}

std::string check_triangle_limits(const wgt_triangle& t, uint32_t i) {
  if (!finite_within(t.v0, 3, kCoordLimit) || !finite_within(t.e1, 3, kCoordLimit) || !finite_within(t.e2, 3, kCoordLimit))
    return "triangle " + std::to_string(i) + ": vertices must be finite and within 2^40";
  // |det| <= |e1| |e2| |d| <= (sqrt(3) 2^30)^2 sqrt(3) 2^32 = 3 sqrt(3) 2^92 < 2^95 (edge components
  // within 2^30, primary-direction components within 2^32): mt_test's short 1/det is exact
  if (!finite_within(t.e1, 3, kEdgeLimit) || !finite_within(t.e2, 3, kEdgeLimit))
    return "triangle " + std::to_string(i) + ": edge components must be within 2^30";
  return "";
}

static double sq(double x) { return x * x; }

std::string check_frame_args(const wgt_camera_param& cam, uint32_t W, uint32_t H, uint32_t tw, uint32_t th) {
  if (W == 0 || H == 0) return "empty frame";
  if (tw == 0 || th == 0) return "empty tile";
  if (!(cam.aspect == cam.aspect) || !(cam.fovy == cam.fovy)) return "NaN camera parameter";
  // the kernels pack a sample's (s_i, s_j) into 16 bits each and count sqrt_spp^2
  // samples in 32 bits: u32(sqrt(f32(spp))) must stay <= 65535 (spp < 2^32 - 2^8)
  // the kernels keep a pixel's coordinates as 16-bit halves of one register (wgt_pixel.h Pixel)
  if (W > 65535u || H > 65535u) return "frame width and height must be <= 65535";
  if ((uint32_t)__builtin_sqrtf((float)cam.spp) > 65535u) return "spp too large (u32(sqrt(f32(spp))) must be <= 65535)";
  if (!finite_within(cam.origin, 3, kCoordLimit) || !finite_within(cam.target, 3, kCoordLimit))
    return "camera origin and target must be finite and within 2^40";
  // primary directions: viewport point - origin, the viewport spanning [-1/2, W+1/2] x
  // [-1/2, H+1/2] pixels around po (make_frame, setup_camera_ray)
  const DevFrame fr = make_frame(cam, W, H);
  const double po = std::sqrt(sq((double)fr.pox - fr.ox) + sq((double)fr.poy - fr.oy) + sq((double)fr.poz - fr.oz));
  const double du = std::sqrt(sq((double)fr.dux) + sq((double)fr.duy) + sq((double)fr.duz));
  const double dv = std::sqrt(sq((double)fr.dvx) + sq((double)fr.dvy) + sq((double)fr.dvz));
  if (!(po + (W + 1.0) * du + (H + 1.0) * dv <= kPrimaryDirLimit))
    return "camera: primary ray directions must be finite and within 2^32 (viewport and focal length out of range)";
  return "";
}

double scene_extent(const wgt_quad* lq, uint32_t nlq, const wgt_sphere* sp, uint32_t ns, const wgt_triangle* tr,
                    uint32_t nt) {
  double m = 0.0;
  for (uint32_t i = 0; i < nlq; ++i)
    for (int c = 0; c < 3; ++c) {
      const double p = lq[i].pos[c], r = lq[i].right[c], u = lq[i].up[c];
      m = std::max({m, std::fabs(p), std::fabs(p + r), std::fabs(p + u), std::fabs(p + r + u)});
    }
  for (uint32_t i = 0; i < ns; ++i)
    for (int c = 0; c < 3; ++c) m = std::max(m, std::fabs((double)sp[i].center[c]) + std::fabs((double)sp[i].radius));
  for (uint32_t i = 0; i < nt; ++i)
    for (int c = 0; c < 3; ++c) {
      const double v = tr[i].v0[c];
      m = std::max({m, std::fabs(v), std::fabs(v + tr[i].e1[c]), std::fabs(v + tr[i].e2[c])});
    }
  return m;
}

uint32_t env_u32(const char* name, uint32_t dflt) {
  const char* v = std::getenv(name);
  if (!v || !*v) return dflt;
  return (uint32_t)std::strtoul(v, nullptr, 10);
}

DevFrame make_frame(const wgt_camera_param& cam, uint32_t W, uint32_t H) {
  DevFrame fr{};
  const float theta = radians_w(cam.fovy);
  const f3 origin = f3{cam.origin[0], cam.origin[1], cam.origin[2]};
  const f3 end = f3{cam.target[0], cam.target[1], cam.target[2]};
  const float focal_length = length(origin - end);
  const float h = tan_w(theta * 0.5f);
  const float viewport_height = 2.0f * h * focal_length;
  const float viewport_width = viewport_height * cam.aspect;
  const f3 w = normalize(origin - end);
  const f3 u = normalize(cross(f3{0.0f, 1.0f, 0.0f}, w));
  const f3 v = cross(w, u);
  const f3 viewport_u = viewport_width * u;
  const f3 viewport_v = viewport_height * (-v);
  const f3 du = viewport_u / (float)W;
  const f3 dv = viewport_v / (float)H;
  const f3 vul = ((origin - focal_length * w) - 0.5f * viewport_u) - 0.5f * viewport_v;
  const f3 po = vul + 0.5f * (du + dv);
  fr.ox = origin.x; fr.oy = origin.y; fr.oz = origin.z;
  fr.pox = po.x; fr.poy = po.y; fr.poz = po.z;
  fr.dux = du.x; fr.duy = du.y; fr.duz = du.z;
  fr.dvx = dv.x; fr.dvy = dv.y; fr.dvz = dv.z;
  fr.recip_sqrt_spp = 1.0f / __builtin_sqrtf((float)cam.spp);
  fr.fspp = (float)cam.spp;
  fr.inv_fspp = pow2_recip(cam.spp);
  fr.sqrt_spp = (uint32_t)__builtin_sqrtf((float)cam.spp);
  fr.W = W; fr.H = H;
  fr.kernel = env_u32("WGT_KERNEL", 2);
  // swept on the persistent BVH4 kernel with compact nodes (DESIGN.md §4.2,
  // profiles/sweeps/r01_sweep_compact_knobs.jsonl)
  // 0 = by the kernel's waves per SIMD: 18/16 at 5, 16/14 at 6 (PsForm::to_trav, to_service)
  fr.ps_to_trav = env_u32("WGT_PS_TO_TRAV", 0);
  fr.ps_to_service = env_u32("WGT_PS_TO_SERVICE", 0);
  fr.ps_svc_frac = env_u32("WGT_PS_SVC_FRAC", 16);  // sweep: profiles/sweeps/r01_ps_svc_frac.jsonl
  // >= 1: with 0 a wave whose lanes all hold a node but no open leaf would take triangle steps forever
  fr.tri_ratio = std::max<uint32_t>(env_u32("WGT_TRI_RATIO", 100), 1u);
  fr.cnode = env_u32("WGT_CNODE", 1);  // compact nodes (2: only once the 128-B tree outgrows an XCD's L2)
  fr.pq_refill = env_u32("WGT_PQ_REFILL", 0);  // 0 = the default, 2 (launch_render)
  // 0: block order (A/B); n: LPT order from an n*n-spp cost pre-pass (when spp > n*n)
  fr.pq_lpt = env_u32("WGT_PQ_LPT", 1);
  fr.pq_svc_cost = env_u32("WGT_PQ_SVC_COST", 7);
  // the pre-pass's paths end at depth 6 (a cost estimate needs the path's first bounces, and
  // the full 50-bounce tail set the pre-pass's own drain): sponza +0.4%, bunny +0.7%, the frame
  // alone -0.6% against full paths, 3 rounds on one box (profiles/sweeps/r04_pq_depth.log)
  fr.pq_depth = std::min<uint32_t>(std::max<uint32_t>(env_u32("WGT_PQ_DEPTH", 6), 1u), (uint32_t)kRayDepth);
  // sampled frames: the pre-pass's cost of a pixel of side k > pq_lpt scaled to its k^2 samples
  fr.pq_lpt_weight = env_u32("WGT_PQ_LPT_WEIGHT", 1);
  fr.pq_lpt_all = env_u32("WGT_PQ_LPT_ALL", 1);  // sweep: all pixels -3% (sponza), -4% (bunny) at 256 spp
  return fr;
}

DevFrame tile_frame(const wgt_camera_param& cam, uint32_t W, uint32_t H, uint32_t tw, uint32_t th, uint32_t n_tiles) {
  DevFrame fr = make_frame(cam, W, H);
  fr.tw = tw; fr.th = th; fr.n_tiles = n_tiles;
  return fr;
}

// WGT_PQ_REFINE: swept over 1, 2 and 4, the fastest on both scenes (DESIGN.md §4.2 item 32,
// profiles/order_reuse/bench_ab.md)
OrderKnobs order_knobs() { return OrderKnobs{env_u32("WGT_PQ_REUSE", 1), env_u32("WGT_PQ_REFINE", 4)}; }

uint32_t order_blocks(const DevFrame& fr) {
  const uint64_t bx = (fr.tw + 7u) / 8u, by = (fr.th + 7u) / 8u;
  const uint64_t per_tile = bx * by;  // < 2^58
  if (per_tile > 0x3ffffffull) return 0u;
  const uint64_t nb = per_tile * fr.n_tiles;  // < 2^58
  return nb * 64u > 0xffffffffull ? 0u : (uint32_t)nb;
}

bool order_lpt_on(const DevFrame& fr) { return fr.kernel == 2 && fr.pq_lpt != 0 && fr.sqrt_spp > fr.pq_lpt; }

bool order_eligible(const DevFrame& fr, const OrderKnobs& knobs, bool sampled, uint32_t nb) {
  return knobs.reuse != 0 && !sampled && nb != 0 && order_lpt_on(fr);
}

OrderKey order_key(const DevFrame& fr, uint32_t nb, const OrderKnobs& knobs, uint64_t epoch, uint64_t tiles,
                   bool tiles_by_ptr) {
  OrderKey k{};
  k.fr = fr;
  // what launch_render fills in per launch is no part of the view
  k.fr.perm = nullptr;
  k.fr.cost = nullptr;
  k.fr.ps_spill = nullptr;
  k.fr.ps_spill_stride = k.fr.n_slots = k.fr.div_bx = k.fr.div_bpt = 0u;
  k.nb = nb;
  k.refine = knobs.refine;
  k.epoch = epoch;
  k.tiles = tiles;
  k.tiles_by_ptr = tiles_by_ptr ? 1u : 0u;
  return k;
}

bool same_view(const OrderKey& a, const OrderKey& b) {
  // the frame's 4-byte fields up to its pointers (no padding among them), by their bits: a camera
  // that differs only in the sign of a zero is another view, which costs one pre-pass
  static_assert(offsetof(DevFrame, perm) == 34 * 4, "DevFrame's scalar fields, then its pointers");
  return std::memcmp(&a.fr, &b.fr, offsetof(DevFrame, perm)) == 0 && a.nb == b.nb && a.refine == b.refine &&
         a.epoch == b.epoch && a.tiles == b.tiles && a.tiles_by_ptr == b.tiles_by_ptr;
}

uint64_t order_tiles_hash(const wgt_tile* tiles, uint32_t n) {
  uint64_t h = 0xcbf29ce484222325ull;  // FNV-1a over the origins
  for (uint32_t i = 0; i < n; ++i)
    for (const uint32_t v : {tiles[i].x0, tiles[i].y0})
      for (int b = 0; b < 4; ++b) h = (h ^ ((v >> (8 * b)) & 0xffu)) * 0x100000001b3ull;
  return h;
}

void OrderPlanner::invalidate() {
  ++epoch_;
  if (cur_ >= 0) ++n_invalid_;
  cur_ = -1;
  cur_side_ = 0;
  seen_ = false;
}

void OrderPlanner::buffers_reset() {
  // the kept order is gone with its buffer; the scene is what it was, so the epoch and the run of
  // sightings stay (the launch that made the buffers grow is the one that refines)
  if (cur_ >= 0) ++n_invalid_;
  cur_ = -1;
  cur_side_ = 0;
  for (uint32_t& r : readers_) r = 0u;
}

bool OrderPlanner::refine_due(const OrderKey& key, bool eligible) const {
  if (!eligible || (cur_ >= 0 && same_view(key, cur_key_))) return false;
  return seen_ && same_view(key, last_);
}

void OrderPlanner::launch_failed(const OrderPlan& p) {
  // a REFINE whose kernels were not queued left no order in its buffer
  if (p.mode == kOrderRefine && cur_ == p.buf) invalidate();
}

void OrderPlanner::counts(uint64_t& today, uint64_t& refine, uint64_t& reuse, uint64_t& invalidations) const {
  today = n_today_;
  refine = n_refine_;
  reuse = n_reuse_;
  invalidations = n_invalid_;
}

uint32_t stack_entries(const BvhOut& bvh) { return std::max(bvh.stack_need, 1u) + 1u; }

// Waves per SIMD: 6 with 3-byte stack entries when every ref fits them, else 5; WGT_PS_WAVES=5
// forces 5 (sweeps); without triangles the kernel without traversal at its own budget (3-byte
// entries in the launch and the occupancy query alike, ps_lds).  Parked traversal state
// (opt-in: WGT_PARK=1; it removes the service phase's scratch stores but
// measured 5 % slower, profiles/r04/): the LDS stack holds what fits beside the parked words at
// the wave budget, or the whole stack when that is smaller; WGT_PS_CAP lowers it, down to
// kMinPsCap, for tests.
PsForm ps_form_for(const BvhOut& bvh, uint32_t n_tris) {
  PsForm f{n_tris > 0, (uint32_t)kPsWavesNoTris, false, stack_entries(bvh)};
  if (!f.tris) return f;
  const bool fits24 = bvh.n_nodes < kStack24Nodes && n_tris < kStack24Tris;
  f.waves = fits24 && env_u32("WGT_PS_WAVES", 0) != 5 ? 6u : 5u;
  f.park = env_u32("WGT_PARK", 0) != 0;
  if (f.park) {
    const uint32_t c = std::min(f.cap, ps_cap_max(f.waves));
    f.cap = std::max(std::min(c, std::max(env_u32("WGT_PS_CAP", c), kMinPsCap)), kMinPsCap);
  }
  return f;
}

void fill_bvh_info(const BvhOut& bvh, uint32_t n_tris, const PsForm& f, wgt_scene_info& in) {
  in.n_tris = n_tris;
  in.bvh_nodes = bvh.n_nodes;
  in.bvh_leaves = bvh.n_leaves;
  in.bvh_max_depth = bvh.max_depth;
  in.bvh_max_leaf = bvh.max_leaf;
  in.sah_cost = bvh.sah_cost;
  in.bvh_width = f.tris ? (uint32_t)kBvhWidth : 0u;
  in.bvh_stack = f.tris ? std::max(bvh.stack_need, 1u) : 0u;
  in.bvh2_nodes = bvh.n_nodes2;
  in.bvh2_depth = bvh.depth2;
  in.bvh_compact = (size_t)bvh.n_nodes * kNode4Floats * 4 > kCompactNodeBytes ? 1u : 0u;
  in.bvh_compact_step = bvh.cstep;
  in.ps_waves = f.tris ? f.waves : 0u;
  in.ps_park = f.park;
  in.ps_stack = f.tris ? f.cap : 0u;
}

constexpr double kOriginBoundScale = 4.0;
static_assert(BvhOptions{}.max_depth == kMaxBvhDepth && BvhOptions{}.stack_limit == kStackMax, "the builder's defaults");
std::string build_bvh(const wgt_triangle* tris, uint32_t n_tris, double extent, BvhOut& bvh) {
  std::string err;
  const BvhOptions opt = BvhOptionsFromEnv(kMaxBvhDepth, kStackMax, kStackNarrow, kOriginBoundScale * extent);
  return BuildBvh(tris, n_tris, opt, bvh, err) ? "" : err;
}
std::string build_for_export(const wgt_triangle* tris, uint32_t n_tris, BvhOut& bvh) {
  return build_bvh(tris, n_tris, scene_extent(nullptr, 0, nullptr, 0, tris, n_tris), bvh);
}

std::string refit_bvh(const wgt_triangle* tris, uint32_t n_tris, double extent, BvhOut& bvh) {
  std::string err;
  return RefitBvh(bvh, tris, n_tris, kOriginBoundScale * extent, err) ? "" : err;
}
std::string refit_for_export(const wgt_triangle* built_from, const wgt_triangle* now, uint32_t n_tris, BvhOut& bvh) {
  const std::string err = build_for_export(built_from, n_tris, bvh);
  if (!err.empty()) return err;
  return refit_bvh(now, n_tris, scene_extent(nullptr, 0, nullptr, 0, now, n_tris), bvh);
}

std::string check_update_count(uint32_t scene_tris, uint32_t n_tris) {
  if (scene_tris == 0) return "the scene has no triangles to update";
  if (n_tris != scene_tris)
    return "triangle count " + std::to_string(n_tris) + " differs from the uploaded " + std::to_string(scene_tris) +
           " (an update moves triangles; upload to add or remove)";
  return "";
}

static bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

std::string check_update_records(const void* d_tris, uint32_t scene_tris, uint32_t n_tris) {
  if (!d_tris) return "null triangles";
  const std::string bad = check_update_count(scene_tris, n_tris);
  if (!bad.empty()) return bad;
  if (!aligned_to(d_tris, 16)) return "misaligned triangles: device wgt_triangle records must be 16-byte aligned";
  return "";
}

std::string check_update_vertices(const void* d_verts, uint32_t n_verts, const void* d_index, uint32_t scene_tris,
                                  uint32_t n_tris) {
  if (!d_verts) return "null vertices";
  const std::string bad = check_update_count(scene_tris, n_tris);
  if (!bad.empty()) return bad;
  if (!aligned_to(d_verts, 4) || !aligned_to(d_index, 4))
    return "misaligned vertices or indices: device floats and indices must be 4-byte aligned";
  if (n_verts == 0) return "vertex count 0";
  if (!d_index && (uint64_t)n_verts != 3ull * n_tris)
    return "vertex count " + std::to_string(n_verts) + " is not 3 x " + std::to_string(n_tris) +
           " triangles (unindexed vertices: three per triangle)";
  return "";
}

void triangle_of_vertices(const float* verts, wgt_triangle& t) {
  t = wgt_triangle{};
  for (int c = 0; c < 3; ++c) {
    const float v0 = verts[c] + 0.0f, v1 = verts[3 + c] + 0.0f, v2 = verts[6 + c] + 0.0f;
    t.v0[c] = v0;
    t.e1[c] = v1 - v0;
    t.e2[c] = v2 - v0;
  }
}

std::string check_vertex_index(const uint32_t index[3], uint32_t n_verts, uint32_t i) {
  for (int c = 0; c < 3; ++c)
    if (index[c] >= n_verts)
      return "triangle " + std::to_string(i) + ": vertex index " + std::to_string(index[c]) +
             " is not below the vertex count " + std::to_string(n_verts);
  return "";
}

std::string check_rebuild_records(const void* tris, uint32_t n_tris, uint32_t leaf, bool align) {
  if (!tris) return "null triangles";
  if (n_tris == 0) return "triangle count 0: a rebuild needs a triangle (upload a scene without triangles instead)";
  if (n_tris > rebuild_max_tris(leaf))
    return "too many triangles for a rebuild: " + std::to_string(n_tris) + " exceeds " +
           std::to_string(rebuild_max_tris(leaf)) + " (leaf target " + std::to_string(leaf) + " x 4^" +
           std::to_string(kRebuildLevels) + ")";
  if (align && !aligned_to(tris, 16)) return "misaligned triangles: device wgt_triangle records must be 16-byte aligned";
  return "";
}

std::string morton_bvh(const wgt_triangle* tris, uint32_t n_tris, double extent, BvhOut& bvh,
                       std::vector<uint32_t>* level_count) {
  std::string err;
  return BuildMortonBvh(tris, n_tris, RebuildLeafFromEnv(), kOriginBoundScale * extent, bvh, level_count, err) ? "" : err;
}
std::string morton_for_export(const wgt_triangle* tris, uint32_t n_tris, BvhOut& bvh) {
  return morton_bvh(tris, n_tris, scene_extent(nullptr, 0, nullptr, 0, tris, n_tris), bvh, nullptr);
}

uint32_t rebuild_node_cap(uint32_t n_tris) { return std::max(n_tris, 2u) - 1u; }

static size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

size_t tree_layout(uint32_t n_tris, uint32_t n_nodes, size_t off[]) {
  const size_t bytes[kSceneParts] = {0, 0, (size_t)n_nodes * kNode4Floats * 4, (size_t)n_tris * kTriRecordBytes,
                                     (size_t)n_tris * 32, (size_t)n_nodes * kCRecordFloat4s * 16, n_nodes};
  size_t total = 0;
  for (int i = kPartNodes; i < kSceneParts; ++i) {
    off[i] = total;
    total += align256(bytes[i]);
  }
  return total;
}

void bind_tree(DevScene& sc, const size_t off[], const void* base) {
  const auto at = [&](ScenePart i) { return (const float4*)((const char*)base + off[i]); };
  sc.nodes = at(kPartNodes); sc.tris = at(kPartTris); sc.tshade = at(kPartShade); sc.cnodes = at(kPartCNodes);
  sc.node_level = (const uint8_t*)at(kPartLevel);
}

RebuildScratch plan_rebuild_scratch(uint32_t n_tris, size_t temp_bytes) {
  RebuildScratch p{};
  const size_t n = n_tris, nodes = rebuild_node_cap(n_tris);  // a level holds at most every node
  size_t at = 0;
  const auto take = [&](size_t bytes) { const size_t o = at; at += align256(bytes); return o; };
  for (int i = 0; i < 2; ++i) p.key[i] = take(n * 8);
  for (int i = 0; i < 2; ++i) p.val[i] = take(n * 4);
  for (int i = 0; i < 2; ++i) p.list[i] = take(nodes * sizeof(RebuildRange));
  p.cuts = take(nodes * 16);
  p.count = take((nodes + 1) * 4);
  p.offset = take((nodes + 1) * 4);
  p.bounds = take(sizeof(RebuildBounds));
  p.stats = take(sizeof(RebuildStats));
  p.temp = take(temp_bytes);
  p.bytes = at;
  return p;
}

void plan_tree_form(const BvhOut& bvh, uint32_t n_tris, DevScene& sc) {
  const PsForm form = ps_form_for(bvh, n_tris);
  sc.n_tris = n_tris;
  sc.n_nodes = bvh.n_nodes;
  sc.stack = stack_entries(bvh);
  sc.ps_waves = form.waves; sc.ps_park = form.park; sc.ps_cap = form.cap;
}

std::vector<uint32_t> level_begin_of(const std::vector<uint32_t>& level_count) {
  std::vector<uint32_t> begin(level_count.size() + 1, 0u);
  for (size_t l = 0; l < level_count.size(); ++l) begin[l + 1] = begin[l] + level_count[l];
  return begin;
}

double checked_extent(const RefitCheck& r) {
  double m;
  static_assert(sizeof m == sizeof r.extent_bits, "a double's bits");
  std::memcpy(&m, &r.extent_bits, sizeof m);
  return m;
}

double compact_bound(double extent, const float* root_node) {
  double M = std::max(kOriginBoundScale * extent, 0x1p-60);
  for (int i = 0; i < 6 * kBvhWidth; ++i)
    if (root_node[i] != kEmptySlotCoord) M = std::max(M, 2.0 * std::fabs((double)root_node[i]));
  return M;
}

std::string refit_levels(const uint8_t* level, uint32_t n_nodes, std::vector<uint32_t>& order,
                         std::vector<uint32_t>& begin) {
  uint32_t count[256] = {};
  for (uint32_t i = 0; i < n_nodes; ++i) count[level[i]]++;
  if (count[255]) return "refit: the tree is deeper than node levels are recorded for (255)";
  uint32_t levels = 0;
  for (uint32_t l = 0; l < 255; ++l)
    if (count[l]) levels = l + 1;
  begin.assign(levels + 1, 0u);
  for (uint32_t l = 0; l < levels; ++l) begin[l + 1] = begin[l] + count[l];
  order.resize(n_nodes);
  std::vector<uint32_t> at(begin.begin(), begin.end() - 1);
  for (uint32_t i = 0; i < n_nodes; ++i) order[at[level[i]]++] = i;
  return "";
}

// the device triangle records (wgt_geom.h kTriRecordBytes): the builder's 64-B records
static_assert(kTriRecordBytes == kTriRecordFloats * 4, "device and host triangle records");
static_assert(sizeof(wgt_quad) == 96 && sizeof(wgt_sphere) == 32, "the reference's records (wgt_internal.h)");
ScenePlan pack_scene(const wgt_quad* lights, uint32_t n_lights, const wgt_quad* quads, uint32_t n_quads,
                     const wgt_sphere* spheres, uint32_t n_spheres, uint32_t n_tris, const BvhOut& bvh,
                     const BvhImage& image) {
  ScenePlan p{};
  const size_t quad_bytes = (size_t)n_lights * sizeof(wgt_quad);
  const struct { const void* src; size_t bytes; } part[kSceneParts] = {
      {nullptr, quad_bytes + (size_t)n_quads * sizeof(wgt_quad)},  // two sources, copied below
      {spheres, (size_t)n_spheres * sizeof(wgt_sphere)},
      {image.nodes.data(), image.nodes.size() * 4},
      {bvh.tris.data(), bvh.tris.size() * 4},
      {bvh.tshade.data(), bvh.tshade.size() * 4},
      {image.crecs.data(), image.crecs.size() * 4},
      {image.level.data(), image.level.size()}};
  size_t total = 0;
  for (int i = 0; i < kSceneParts; ++i) {
    p.off[i] = total;
    total += (part[i].bytes + 255) & ~size_t(255);
  }
  p.host.assign(total, 0);
  char* q = p.host.data() + p.off[kPartQuads];
  std::memcpy(q, lights, quad_bytes);
  if (n_quads) std::memcpy(q + quad_bytes, quads, (size_t)n_quads * sizeof(wgt_quad));
  for (int i = kPartSpheres; i < kSceneParts; ++i)  // a scene without triangles has empty (null) tree parts
    if (part[i].bytes) std::memcpy(p.host.data() + p.off[i], part[i].src, part[i].bytes);

  DevScene& sc = p.sc;
  sc.cstep = bvh.cstep; sc.cbound = bvh.cbound;
  sc.rcstep = 1.0f / sc.cstep;  // a power of two: exact
  sc.n_lights = n_lights; sc.n_quads = n_quads; sc.n_spheres = n_spheres;
  plan_tree_form(bvh, n_tris, sc);
  sc.last_sphere_emissive = spheres[n_spheres - 1].emissive > 0.0f ? 1u : 0u;
  const f3 lr = f3{lights[0].right[0], lights[0].right[1], lights[0].right[2]};
  const f3 lu = f3{lights[0].up[0], lights[0].up[1], lights[0].up[2]};
  sc.light_area = length(cross(lr, lu));  // path_tracer.wgsl:205
  return p;
}

void bind_scene(DevScene& sc, const size_t off[kSceneParts], const void* base) {
  const auto at = [&](ScenePart i) { return (const float4*)((const char*)base + off[i]); };
  sc.quads = at(kPartQuads); sc.spheres = at(kPartSpheres);
  sc.nodes = at(kPartNodes); sc.tris = at(kPartTris); sc.tshade = at(kPartShade); sc.cnodes = at(kPartCNodes);
  sc.node_level = (const uint8_t*)at(kPartLevel);
}

wgt_denoise_params denoise_defaults() { return wgt_denoise_params{5u, 7u, 1.0f, WGT_DENOISE_DEMODULATE}; }

static bool denoise_size_ok(uint32_t W, uint32_t H) {
  return W != 0 && H != 0 && W <= kDenoiseMaxDim && H <= kDenoiseMaxDim && (uint64_t)W * H <= kDenoiseMaxPixels;
}
static size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

size_t denoise_workspace_bytes(uint32_t W, uint32_t H) {
  if (!denoise_size_ok(W, H)) return 0;
  const size_t n = (size_t)W * H;
  return align_up(n * 32, kDenoiseAlign) + 2 * align_up(n * 16, kDenoiseAlign);
}

std::string check_denoise_args(const wgt_denoise_params* params, uint32_t W, uint32_t H, const void* in,
                               const wgt_hit_buffers* guides, const void* out32, const void* out8) {
  if (!in) return "null input image";
  if (!guides) return "null guides";
  if (!guides->prim) return "null guides.prim";
  if (!guides->pos) return "null guides.pos";
  if (!guides->norm) return "null guides.norm";
  if (!guides->col) return "null guides.col";
  if (!guides->flags) return "null guides.flags";
  if (!out32 && !out8) return "null outputs: rgba32f_out and rgba8_out are both null";
  if (!denoise_size_ok(W, H))
    return "image size " + std::to_string(W) + " x " + std::to_string(H) + ": W and H must be 1.." +
           std::to_string(kDenoiseMaxDim) + " and W * H at most " + std::to_string(kDenoiseMaxPixels);
  if (params) {
    if (params->iterations < 1 || params->iterations > kDenoiseMaxIterations)
      return "params.iterations " + std::to_string(params->iterations) + " is not in 1.." +
             std::to_string(kDenoiseMaxIterations);
    if (params->normal_power > kDenoiseMaxNormalPower)
      return "params.normal_power " + std::to_string(params->normal_power) + " is not in 0.." +
             std::to_string(kDenoiseMaxNormalPower);
    if (!(params->sigma_pos > 0.0f) || !std::isfinite(params->sigma_pos)) return "params.sigma_pos must be finite and > 0";
    if (params->flags & ~WGT_DENOISE_DEMODULATE) return "params.flags has bits other than WGT_DENOISE_DEMODULATE";
  }
  return "";
}

std::string check_denoise_workspace(const void* ws, size_t ws_bytes, uint32_t W, uint32_t H) {
  if (!ws) return "null workspace";
  if (!aligned_to(ws, kDenoiseAlign)) return "misaligned workspace: it must be 256-byte aligned";
  const size_t need = denoise_workspace_bytes(W, H);
  if (ws_bytes < need)
    return "workspace_bytes " + std::to_string(ws_bytes) + " is below the " + std::to_string(need) +
           " that wgt_denoise_workspace_bytes asks for";
  return "";
}

DenoisePlan plan_denoise(const wgt_denoise_params& params, uint32_t W, uint32_t H) {
  DenoisePlan p{};
  p.W = W; p.H = H;
  p.iterations = params.iterations;
  p.normal_power = params.normal_power;
  p.demodulate = params.flags & WGT_DENOISE_DEMODULATE;
  p.tiled_max_step = std::min(env_u32("WGT_DENOISE_TILED_STEP", kDenoiseTiledStep), kDenoiseMaxTiledStep);
  // two roundings, then an exact power of four (which may round once more among the denormals):
  // the restatement's kz0 * f32(4.0 ** -i)
  const float kz0 = 1.0f / (params.sigma_pos * params.sigma_pos);
  for (uint32_t i = 0; i < kDenoiseMaxIterations; ++i) p.kz[i] = kz0 * std::ldexp(1.0f, -2 * (int)i);
  const size_t n = (size_t)W * H;
  p.off_rec = 0;
  p.off_it0 = align_up(n * 32, kDenoiseAlign);
  p.off_it1 = p.off_it0 + align_up(n * 16, kDenoiseAlign);
  p.bytes = p.off_it1 + align_up(n * 16, kDenoiseAlign);
  return p;
}

wgt_denoise_variance_params denoise_variance_defaults() {
  return wgt_denoise_variance_params{5u, 7u, 1.0f, WGT_DENOISE_DEMODULATE, 4.0f, 4u};
}

size_t denoise_variance_workspace_bytes(uint32_t W, uint32_t H) { return denoise_workspace_bytes(W, H); }

std::string check_denoise_variance_args(const wgt_denoise_variance_params* params, uint32_t W, uint32_t H,
                                        const wgt_temporal_state* state, const wgt_hit_buffers* guides,
                                        const void* out32, const void* out8) {
  if (!state) return "null state";
  if (!guides) return "null guides";
  if (!state->rgba32f) return "null state.rgba32f";
  if (!state->len) return "null state.len";
  if (!state->moments) return "null state.moments";
  if (!guides->prim) return "null guides.prim";
  if (!guides->pos) return "null guides.pos";
  if (!guides->norm) return "null guides.norm";
  if (!guides->col) return "null guides.col";
  if (!guides->flags) return "null guides.flags";
  if (!out32 && !out8) return "null outputs: rgba32f_out and rgba8_out are both null";
  if (!denoise_size_ok(W, H))
    return "image size " + std::to_string(W) + " x " + std::to_string(H) + ": W and H must be 1.." +
           std::to_string(kDenoiseMaxDim) + " and W * H at most " + std::to_string(kDenoiseMaxPixels);
  if (params) {
    if (params->iterations < 1 || params->iterations > kDenoiseMaxIterations)
      return "params.iterations " + std::to_string(params->iterations) + " is not in 1.." +
             std::to_string(kDenoiseMaxIterations);
    if (params->normal_power > kDenoiseMaxNormalPower)
      return "params.normal_power " + std::to_string(params->normal_power) + " is not in 0.." +
             std::to_string(kDenoiseMaxNormalPower);
    if (!(params->sigma_pos > 0.0f) || !std::isfinite(params->sigma_pos)) return "params.sigma_pos must be finite and > 0";
    if (params->flags & ~WGT_DENOISE_DEMODULATE) return "params.flags has bits other than WGT_DENOISE_DEMODULATE";
    if (!(params->sigma_lum > 0.0f) || !std::isfinite(params->sigma_lum)) return "params.sigma_lum must be finite and > 0";
    if (params->min_history < 1 || params->min_history > kDenoiseVarianceMaxMinHistory)
      return "params.min_history " + std::to_string(params->min_history) + " is not in 1.." +
             std::to_string(kDenoiseVarianceMaxMinHistory);
  }
  return "";
}

std::string check_denoise_variance_workspace(const void* ws, size_t ws_bytes, uint32_t W, uint32_t H) {
  if (!ws) return "null workspace";
  if (!aligned_to(ws, kDenoiseAlign)) return "misaligned workspace: it must be 256-byte aligned";
  const size_t need = denoise_variance_workspace_bytes(W, H);
  if (ws_bytes < need)
    return "workspace_bytes " + std::to_string(ws_bytes) + " is below the " + std::to_string(need) +
           " that wgt_denoise_variance_workspace_bytes asks for";
  return "";
}

DenoiseVariancePlan plan_denoise_variance(const wgt_denoise_variance_params& params, uint32_t W, uint32_t H) {
  // the layout, the kz and the switch are the plain filter's
  const DenoisePlan d = plan_denoise(wgt_denoise_params{params.iterations, params.normal_power, params.sigma_pos, params.flags}, W, H);
  DenoiseVariancePlan p{};
  p.W = W; p.H = H;
  p.iterations = d.iterations;
  p.normal_power = d.normal_power;
  p.demodulate = d.demodulate;
  for (uint32_t i = 0; i < kDenoiseMaxIterations; ++i) p.kz[i] = d.kz[i];
  p.sigma_lum = params.sigma_lum;
  p.min_history = (float)params.min_history;
  p.tiled_max_step = d.tiled_max_step;
  p.off_rec = d.off_rec; p.off_it0 = d.off_it0; p.off_it1 = d.off_it1; p.bytes = d.bytes;
  return p;
}

wgt_temporal_params temporal_defaults() { return wgt_temporal_params{32u, 0.9f, 1.0f, 0u}; }

// [a, a + na) and [b, b + nb) share a byte (no pointer arithmetic: the addresses as integers)
static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x >= y ? x - y < nb : y - x < na;
}

static const char* null_temporal_guide(const wgt_hit_buffers& g, bool prev) {
  if (!g.prim) return prev ? "null guides_prev.prim" : "null guides.prim";
  if (!g.pos) return prev ? "null guides_prev.pos" : "null guides.pos";
  if (!g.norm) return prev ? "null guides_prev.norm" : "null guides.norm";
  if (!g.flags) return prev ? "null guides_prev.flags" : "null guides.flags";
  return nullptr;
}

// Both forms' checks: motion_form adds the motion buffers' right after the first-frame triple.
static std::string check_temporal_form(const wgt_temporal_params* params, uint32_t W, uint32_t H,
                                       const wgt_camera_param* cam, const wgt_camera_param* cam_prev, const void* in,
                                       const wgt_hit_buffers* guides, bool motion_form, const wgt_motion_buffers* motion,
                                       const wgt_temporal_state* prev, const wgt_hit_buffers* guides_prev,
                                       const wgt_temporal_state* out) {
  if (!in) return "null input image";
  if (!cam) return "null camera";
  if (!guides) return "null guides";
  if (!out) return "null out";
  if (!out->rgba32f) return "null out.rgba32f";
  if (!out->len) return "null out.len";
  if (const char* bad = null_temporal_guide(*guides, false)) return bad;
  const bool first = !prev && !guides_prev && !cam_prev;
  if (!first) {
    if (!prev || !guides_prev || !cam_prev)
      return "first-frame arguments: prev, guides_prev and cam_prev must be all null (the first frame) or all set";
    if (motion_form) {
      if (!motion) return "null motion";
      if (!motion->pos_prev) return "null motion.pos_prev";
      if (!motion->norm_prev) return "null motion.norm_prev";
    }
    if (!prev->rgba32f) return "null prev.rgba32f";
    if (!prev->len) return "null prev.len";
    if (const char* bad = null_temporal_guide(*guides_prev, true)) return bad;
    if (!prev->moments != !out->moments) return "moments must be null or set in prev and out alike";
  }
  if (!denoise_size_ok(W, H))
    return "image size " + std::to_string(W) + " x " + std::to_string(H) + ": W and H must be 1.." +
           std::to_string(kDenoiseMaxDim) + " and W * H at most " + std::to_string(kDenoiseMaxPixels);
  if (params) {
    if (params->max_history < 1 || params->max_history > kTemporalMaxHistory)
      return "params.max_history " + std::to_string(params->max_history) + " is not in 1.." +
             std::to_string(kTemporalMaxHistory);
    if (!(params->normal_min >= -1.0f && params->normal_min <= 1.0f)) return "params.normal_min must be finite and in -1..1";
    if (!(params->plane_tol >= 0.0f) || !std::isfinite(params->plane_tol)) return "params.plane_tol must be finite and >= 0";
    if (params->flags & ~WGT_TEMPORAL_MATCH_PRIM) return "params.flags has bits other than WGT_TEMPORAL_MATCH_PRIM";
  }
  // what a render of this camera would be refused for, its spp apart (the pass ignores spp and seed)
  const wgt_camera_param* cams[2] = {cam, first ? nullptr : cam_prev};
  for (int k = 0; k < 2; ++k) {
    if (!cams[k]) continue;
    wgt_camera_param c = *cams[k];
    c.spp = 1u;
    // a degenerate camera (origin equal to target, or looking along the up axis: make_frame's terms
    // are NaN, which a render refuses as out-of-range directions) is no error here: no pixel finds history
    const bool degenerate = c.aspect == c.aspect && c.fovy == c.fovy && finite_within(c.origin, 3, kCoordLimit) &&
                            finite_within(c.target, 3, kCoordLimit) && c.origin[0] == c.target[0] &&
                            c.origin[2] == c.target[2];
    const std::string bad = degenerate ? "" : check_frame_args(c, W, H, 1u, 1u);
    if (!bad.empty()) return std::string(k ? "cam_prev: " : "cam: ") + bad;
  }
  if (!first) {
    const size_t n = (size_t)W * H;
    if (ranges_overlap(out->rgba32f, n * 16, prev->rgba32f, n * 16)) return "overlap: out.rgba32f and prev.rgba32f";
    if (ranges_overlap(out->len, n * 4, prev->len, n * 4)) return "overlap: out.len and prev.len";
    if (out->moments && ranges_overlap(out->moments, n * 8, prev->moments, n * 8))
      return "overlap: out.moments and prev.moments";
  }
  return "";
}

std::string check_temporal_args(const wgt_temporal_params* params, uint32_t W, uint32_t H, const wgt_camera_param* cam,
                                const wgt_camera_param* cam_prev, const void* in, const wgt_hit_buffers* guides,
                                const wgt_temporal_state* prev, const wgt_hit_buffers* guides_prev,
                                const wgt_temporal_state* out) {
  return check_temporal_form(params, W, H, cam, cam_prev, in, guides, false, nullptr, prev, guides_prev, out);
}

std::string check_temporal_motion_args(const wgt_temporal_params* params, uint32_t W, uint32_t H,
                                       const wgt_camera_param* cam, const wgt_camera_param* cam_prev, const void* in,
                                       const wgt_hit_buffers* guides, const wgt_motion_buffers* motion,
                                       const wgt_temporal_state* prev, const wgt_hit_buffers* guides_prev,
                                       const wgt_temporal_state* out) {
  return check_temporal_form(params, W, H, cam, cam_prev, in, guides, true, motion, prev, guides_prev, out);
}

std::string check_motion_reproject_args(bool has_snapshot, uint32_t n, const wgt_hit_buffers* guides,
                                        const wgt_motion_buffers* out) {
  if (!has_snapshot) return "no motion snapshot since the last upload (wgt_motion_snapshot)";
  if (!guides) return "null guides";
  if (const char* bad = null_temporal_guide(*guides, false)) return bad;
  if (!out) return "null out";
  if (!out->pos_prev) return "null out.pos_prev";
  if (!out->norm_prev) return "null out.norm_prev";
  if (n < 1 || n > kMotionMaxRecords)
    return "n " + std::to_string(n) + " is not in 1.." + std::to_string(kMotionMaxRecords);
  return "";
}

wgt_camera_param sampled_camera(const wgt_camera_param& cam) {
  wgt_camera_param c = cam;
  c.spp = 1u;
  return c;
}

const char* check_sample_map(const void* map) { return map ? nullptr : "null sample map"; }

void sample_constants(float (*out)[4]) {
  for (uint32_t k = 0; k < kSampleBins; ++k) {
    const uint32_t spp = k * k;  // make_frame's expressions for camera.spp = k * k
    out[k][0] = 1.0f / __builtin_sqrtf((float)spp);
    out[k][1] = (float)spp;
    out[k][2] = pow2_recip(spp);
    out[k][3] = 0.0f;
  }
}

wgt_sample_plan_params sample_plan_defaults() { return wgt_sample_plan_params{1u, 8u, 12.0f, 1.0f, 4u, 2u, 0.0f}; }

size_t sample_plan_workspace_bytes(uint32_t W, uint32_t H) {
  if (!denoise_size_ok(W, H)) return 0;
  return align_up((size_t)W * H, kDenoiseAlign) + align_up((kSampleBins + 1) * sizeof(uint32_t), kDenoiseAlign);
}

std::string check_sample_plan_args(const wgt_sample_plan_params* params, uint32_t W, uint32_t H,
                                   const wgt_temporal_state* state, const void* map_out) {
  if (!state) return "null state";
  if (!state->len) return "null state.len";
  if (!state->moments) return "null state.moments";
  if (!map_out) return "null map_out";
  if (!denoise_size_ok(W, H))
    return "image size " + std::to_string(W) + " x " + std::to_string(H) + ": W and H must be 1.." +
           std::to_string(kDenoiseMaxDim) + " and W * H at most " + std::to_string(kDenoiseMaxPixels);
  if (params) {
    if (params->side_min > kSampleSideMax)
      return "params.side_min " + std::to_string(params->side_min) + " is not in 0.." + std::to_string(kSampleSideMax);
    if (params->side_max < params->side_min || params->side_max > kSampleSideMax)
      return "params.side_max " + std::to_string(params->side_max) + " is not in side_min.." + std::to_string(kSampleSideMax);
    if (!(params->gain > 0.0f) || !std::isfinite(params->gain)) return "params.gain must be finite and > 0";
    if (!(params->lum_floor > 0.0f) || !std::isfinite(params->lum_floor)) return "params.lum_floor must be finite and > 0";
    if (params->min_history < 1 || params->min_history > kSamplePlanMaxHistory)
      return "params.min_history " + std::to_string(params->min_history) + " is not in 1.." +
             std::to_string(kSamplePlanMaxHistory);
    if (params->dilate > kSamplePlanMaxDilate)
      return "params.dilate " + std::to_string(params->dilate) + " is not in 0.." + std::to_string(kSamplePlanMaxDilate);
    if (!(params->budget_spp >= 0.0f) || !std::isfinite(params->budget_spp)) return "params.budget_spp must be finite and >= 0";
  }
  return "";
}

std::string check_sample_plan_workspace(const void* ws, size_t ws_bytes, uint32_t W, uint32_t H) {
  if (!ws) return "null workspace";
  if (!aligned_to(ws, kDenoiseAlign)) return "misaligned workspace: it must be 256-byte aligned";
  const size_t need = sample_plan_workspace_bytes(W, H);
  if (ws_bytes < need)
    return "workspace_bytes " + std::to_string(ws_bytes) + " is below the " + std::to_string(need) +
           " that wgt_sample_plan_workspace_bytes asks for";
  return "";
}

SamplePlan plan_sample_plan(const wgt_sample_plan_params& params, uint32_t W, uint32_t H) {
  SamplePlan p{};
  p.W = W; p.H = H;
  p.side_min = params.side_min; p.side_max = params.side_max; p.dilate = params.dilate;
  p.side_min_f = (float)params.side_min; p.side_max_f = (float)params.side_max;
  p.gain = params.gain; p.lum_floor = params.lum_floor;
  p.min_history = (float)params.min_history;
  p.budgeted = params.budget_spp > 0.0f ? 1u : 0u;
  // a float times W * H <= 2^25 is exact in double up to its own rounding; beyond 2^64 every map fits
  const double b = std::floor((double)params.budget_spp * (double)W * (double)H);
  p.budget = b >= 18446744073709551616.0 ? ~(uint64_t)0 : (uint64_t)b;
  p.off_want = 0;
  p.off_bins = align_up((size_t)W * H, kDenoiseAlign);
  p.bytes = p.off_bins + align_up((kSampleBins + 1) * sizeof(uint32_t), kDenoiseAlign);
  return p;
}

uint32_t sample_plan_cap(const SamplePlan& p, const uint32_t* bins, uint64_t& total) {
  uint32_t c = p.side_max;
  if (p.budgeted)
    while (c > p.side_min && sample_plan_total(bins, c) > p.budget) --c;  // side_min when not even it meets the budget
  total = sample_plan_total(bins, c);
  return c;
}

TemporalCam temporal_camera(const wgt_camera_param& cam, uint32_t W, uint32_t H) {
  const DevFrame fr = make_frame(cam, W, H);
  const f3 o{fr.ox, fr.oy, fr.oz}, du{fr.dux, fr.duy, fr.duz}, dv{fr.dvx, fr.dvy, fr.dvz};
  const f3 c = f3{fr.pox, fr.poy, fr.poz} - o;
  const f3 nrm = cross(du, dv);
  const f3 iu = du / dot(du, du), iv = dv / dot(dv, dv);
  TemporalCam t{};
  t.o[0] = o.x; t.o[1] = o.y; t.o[2] = o.z;
  t.c[0] = c.x; t.c[1] = c.y; t.c[2] = c.z;
  t.nrm[0] = nrm.x; t.nrm[1] = nrm.y; t.nrm[2] = nrm.z;
  t.iu[0] = iu.x; t.iu[1] = iu.y; t.iu[2] = iu.z;
  t.iv[0] = iv.x; t.iv[1] = iv.y; t.iv[2] = iv.z;
  t.k = dot(c, nrm);
  return t;
}

TemporalPlan plan_temporal(const wgt_temporal_params& params, uint32_t W, uint32_t H, const wgt_camera_param& cam,
                           const wgt_camera_param* cam_prev) {
  TemporalPlan p{};
  p.W = W; p.H = H;
  p.first = cam_prev ? 0u : 1u;
  p.match_prim = params.flags & WGT_TEMPORAL_MATCH_PRIM;
  p.max_history = (float)params.max_history;
  p.normal_min = params.normal_min;
  p.plane_tol = params.plane_tol;
  p.cam = temporal_camera(cam, W, H);
  if (cam_prev) p.cam_prev = temporal_camera(*cam_prev, W, H);
  return p;
}

// A layout of the parts in order; a part of no bytes has no source and no destination either.
static StageLayout stage_of(const char* what, std::initializer_list<StagePart> parts) {
  StageLayout l;
  l.what = what;
  for (const StagePart& p : parts) {
    l.part[l.n] = p.bytes ? p : StagePart{};
    l.off[l.n + 1] = l.off[l.n] + align_up(p.bytes, kDenoiseAlign);
    ++l.n;
  }
  return l;
}

StageLayout stage_sample_plan(uint32_t W, uint32_t H, const wgt_temporal_state& state, void* map_out, void* total_out) {
  const size_t n = (size_t)W * H;
  // the total's 8 bytes are always there: the pass is handed a total to write, fetched or not
  return stage_of("a sample plan", {{n * 4, state.len, nullptr}, {n * 8, state.moments, nullptr}, {n, nullptr, map_out},
                                    {8, nullptr, total_out}, {sample_plan_workspace_bytes(W, H), nullptr, nullptr}});
}

StageLayout stage_denoise(uint32_t W, uint32_t H, const void* in, const wgt_hit_buffers& g, void* out32, void* out8) {
  const size_t n = (size_t)W * H;
  return stage_of("a denoiser", {{n * 16, in, out32}, {n * 4, g.prim, nullptr}, {n * 12, g.pos, nullptr},
                                 {n * 12, g.norm, nullptr}, {n * 12, g.col, nullptr}, {n, g.flags, nullptr},
                                 {out8 ? n * 4 : 0, nullptr, out8}, {denoise_workspace_bytes(W, H), nullptr, nullptr}});
}

StageLayout stage_temporal(uint32_t W, uint32_t H, const void* in, const wgt_hit_buffers& g,
                           const wgt_motion_buffers* motion, const wgt_temporal_state* prev,
                           const wgt_hit_buffers* gp, const wgt_temporal_state& out, void* out8) {
  // p, m: the pixels of the previous frame's parts and of the motion buffers' (0: absent, nothing is read)
  const size_t n = (size_t)W * H, p = prev ? n : 0, m = prev && motion ? n : 0, pm = out.moments ? p : 0;
  const wgt_temporal_state sp = p ? *prev : wgt_temporal_state{};
  const wgt_hit_buffers sg = p ? *gp : wgt_hit_buffers{};
  const wgt_motion_buffers sm = m ? *motion : wgt_motion_buffers{};
  return stage_of("a temporal accumulation",
                  {{n * 16, in, out.rgba32f}, {n * 4, g.prim, nullptr}, {n * 12, g.pos, nullptr}, {n * 12, g.norm, nullptr},
                   {n, g.flags, nullptr}, {p * 16, sp.rgba32f, nullptr}, {p * 4, sp.len, nullptr}, {pm * 8, sp.moments, nullptr},
                   {p * 4, sg.prim, nullptr}, {p * 12, sg.pos, nullptr}, {p * 12, sg.norm, nullptr}, {p, sg.flags, nullptr},
                   {m * 12, sm.pos_prev, nullptr}, {m * 12, sm.norm_prev, nullptr}, {n * 4, nullptr, out.len},
                   {out.moments ? n * 8 : 0, nullptr, out.moments}, {out8 ? n * 4 : 0, nullptr, out8}});
}

StageLayout stage_denoise_variance(uint32_t W, uint32_t H, const wgt_temporal_state& state, const wgt_hit_buffers& g,
                                   void* out32, void* out8, void* variance_out) {
  const size_t n = (size_t)W * H;
  return stage_of("a denoiser", {{n * 16, state.rgba32f, out32}, {n * 4, state.len, nullptr}, {n * 8, state.moments, nullptr},
                                 {n * 4, g.prim, nullptr}, {n * 12, g.pos, nullptr}, {n * 12, g.norm, nullptr},
                                 {n * 12, g.col, nullptr}, {n, g.flags, nullptr}, {out8 ? n * 4 : 0, nullptr, out8},
                                 {variance_out ? n * 4 : 0, nullptr, variance_out},
                                 {denoise_variance_workspace_bytes(W, H), nullptr, nullptr}});
}

const char* check_nearest_args(const void* points, const wgt_nearest_buffers* out, uint64_t n) {
  if (!points) return "null points";
  if (!out) return "null output buffers";
  if (!out->prim && !out->dist && !out->pos && !out->uv) return "no nearest field asked for";
  if (n > kNearestMaxPoints) return "too many points";
  return nullptr;
}

NearestStage plan_nearest_stage(const wgt_nearest_buffers& out, bool has_radius, uint32_t n) {
  NearestStage s{};
  const size_t N = n;
  s.points = N * 12;
  s.limits = has_radius ? N * 4 : 0;
  s.prim = out.prim ? N * 4 : 0;
  s.dist = out.dist ? N * 4 : 0;
  s.uv_at = out.pos ? 3 * N : 0;
  s.vec = (s.uv_at + (out.uv ? 2 * N : 0)) * 4;
  return s;
}

void nearest_points_spec(const wgt_triangle* tris, uint32_t n_tris, uint32_t first_prim, const float* points,
                         const float* max_dist, uint32_t n, const wgt_nearest_buffers& out) {
  const size_t N = n;
  const float inf = __builtin_inff();
  for (size_t i = 0; i < N; ++i) {
    const f3 p{points[i], points[N + i], points[2 * N + i]};
    float best = inf;
    uint32_t bi = kNoHit;
    NearestTri b{};
    for (uint32_t k = 0; k < n_tris; ++k) {
      const wgt_triangle& t = tris[k];
      const NearestTri c = nearest_on_tri(p, f3{t.v0[0], t.v0[1], t.v0[2]}, f3{t.e1[0], t.e1[1], t.e1[2]},
                                          f3{t.e2[0], t.e2[1], t.e2[2]});
      // in index order the tie rule never fires (k only grows); it is the definition all the same
      if (nearest_better(c.d2, k, best, bi)) {
        best = c.d2;
        bi = k;
        b = c;
      }
    }
    const float dist = sqrt_rn(best);
    const bool hit = nearest_reported(bi, dist, max_dist ? max_dist[i] : inf);
    if (out.prim) out.prim[i] = hit ? first_prim + bi : kNoHit;
    if (out.dist) out.dist[i] = hit ? dist : inf;
    if (out.pos) {
      out.pos[i] = hit ? b.q.x : 0.0f;
      out.pos[N + i] = hit ? b.q.y : 0.0f;
      out.pos[2 * N + i] = hit ? b.q.z : 0.0f;
    }
    if (out.uv) {
      out.uv[i] = hit ? b.v : 0.0f;
      out.uv[N + i] = hit ? b.w : 0.0f;
    }
  }
}

const char* check_radiance_args(const void* rays, const wgt_radiance_buffers* out, uint64_t samples) {
  if (!rays) return "null rays";
  if (!out) return "null output buffers";
  if (!out->rgb && !out->prim && !out->seed_out) return "no radiance field asked for";
  if (samples > kRadianceMaxSamples) return "too many samples (at most 65536)";
  return nullptr;
}

RadianceStage plan_radiance_stage(const wgt_radiance_buffers& out, bool has_seeds, uint32_t n) {
  const size_t N = n;
  return RadianceStage{N * 24, has_seeds ? N * 4 : 0, out.rgb ? N * 12 : 0, out.prim ? N * 4 : 0,
                       out.seed_out ? N * 4 : 0};
}

std::string plan_radiance(const DevScene& sc, uint32_t seed0, uint32_t samples, uint32_t n, uint32_t resident,
                          RadianceArgs& a) {
  a = RadianceArgs{};
  a.n = n; a.samples = samples; a.seed0 = seed0;
  a.fs = (float)samples;
  a.inv_fs = pow2_recip(samples);
  const PsForm form = ps_form(sc);
  a.persistent = form.tris && env_u32("WGT_KERNEL", 2) == 2 && resident != 0 &&
                 (uint64_t)n + 64ull * resident <= 0xffffffffull;
  if (!a.persistent) return "";
  if (form.cap < sc.stack)
    return "the scene's launch form keeps " + std::to_string(form.cap) + " of " + std::to_string(sc.stack) +
           " stack entries in LDS (WGT_PARK): the radiance query has no parked form";
  // node_form's rule without its camera test: the origins are the caller's rays, tested on the device
  const uint32_t cnode = env_u32("WGT_CNODE", 1);
  a.compact = cnode == 1 || (cnode >= 2 && (size_t)sc.n_nodes * kNode4Floats * 4 > kCompactNodeBytes) ? 1u : 0u;
  const uint32_t to_trav = env_u32("WGT_PS_TO_TRAV", 0), to_service = env_u32("WGT_PS_TO_SERVICE", 0);
  a.to_trav = to_trav ? to_trav : form.to_trav();
  a.to_service = to_service ? to_service : form.to_service();
  a.svc_frac = env_u32("WGT_PS_SVC_FRAC", 16);
  a.tri_ratio = std::max<uint32_t>(env_u32("WGT_TRI_RATIO", 100), 1u);
  const uint32_t refill = env_u32("WGT_PQ_REFILL", 0);
  a.refill = refill ? refill : 2u;
  return "";
}

const char* check_multi_hit_args(const void* rays, const wgt_multi_hit_buffers* out, uint64_t k, uint64_t flags) {
  if (!rays) return "null rays";
  if (!out) return "null output buffers";
  if (!out->count && !out->prim && !out->dist) return "no multi-hit field asked for";
  if (flags & ~(uint64_t)WGT_MULTI_HIT_TRIS_ONLY) return "unknown multi-hit flags";
  if ((out->prim || out->dist) && (k < 1 || k > WGT_MULTI_HIT_MAX_K)) return "k out of range (1..32)";
  return nullptr;
}

MultiHitStage plan_multi_hit_stage(const wgt_multi_hit_buffers& out, bool has_limit, uint32_t n, uint32_t k) {
  const size_t N = n, planes = (size_t)k * N * 4;
  return MultiHitStage{N * 24, has_limit ? N * 4 : 0, out.count ? N * 4 : 0, out.prim ? planes : 0,
                       out.dist ? planes : 0};
}

std::string plan_multi_hit(const DevScene& sc, const wgt_multi_hit_buffers& out, uint32_t n, uint32_t k,
                           uint32_t flags, MultiHitPlan& p) {
  p = MultiHitPlan{};
  p.n = n;
  p.k = (out.prim || out.dist) ? k : 0u;
  p.tris_only = (flags & WGT_MULTI_HIT_TRIS_ONLY) ? 1u : 0u;
  p.mode = out.count ? kMultiHitCount : kMultiHitCull;
  // the kernel's list indices rely on it, whoever calls
  if ((out.prim || out.dist) && (k < 1 || k > WGT_MULTI_HIT_MAX_K)) return "k out of range (1..32)";
  const size_t lds = multi_hit_lds_bytes(sc.stack, p.k);
  if (lds > kLdsPerWorkgroup)
    return "a stack of " + std::to_string(sc.stack) + " entries and a list of " + std::to_string(p.k) +
           " hits per lane need " + std::to_string(lds) + " bytes of LDS, above a workgroup's " +
           std::to_string(kLdsPerWorkgroup);
  p.lds = (uint32_t)lds;
  return "";
}

namespace {
bool nearest_k_lists(const wgt_nearest_k_buffers& out) { return out.prim || out.dist || out.pos || out.uv; }
}  // namespace

const char* check_nearest_k_args(const void* points, const wgt_nearest_k_buffers* out, uint64_t n, uint64_t k) {
  if (!points) return "null points";
  if (!out) return "null output buffers";
  if (!out->count && !nearest_k_lists(*out)) return "no nearest field asked for";
  if (n > kNearestMaxPoints) return "too many points";
  if (nearest_k_lists(*out) && (k < 1 || k > WGT_NEAREST_MAX_K)) return "k out of range (1..32)";
  return nullptr;
}

NearestKStage plan_nearest_k_stage(const wgt_nearest_k_buffers& out, bool has_radius, uint32_t n, uint32_t k) {
  NearestKStage s{};
  const size_t N = n, planes = (size_t)k * N;
  s.points = N * 12;
  s.limits = has_radius ? N * 4 : 0;
  s.count = out.count ? N * 4 : 0;
  s.prim = out.prim ? planes * 4 : 0;
  s.dist = out.dist ? planes * 4 : 0;
  s.uv_at = out.pos ? 3 * planes : 0;
  s.vec = (s.uv_at + (out.uv ? 2 * planes : 0)) * 4;
  return s;
}

std::string plan_nearest_k(const DevScene& sc, const wgt_nearest_k_buffers& out, uint32_t n, uint32_t k,
                           NearestKPlan& p) {
  p = NearestKPlan{};
  const bool lists = nearest_k_lists(out);
  p.n = n;
  p.k = lists ? k : 0u;
  p.words = (out.pos || out.uv) ? 3u : 2u;
  p.mode = out.count ? kNearestKCount : kNearestKCull;
  // measured: with a list the nearest-first step feeds the insertion in nearly ascending
  // order and wins by 10-17 %; the count alone is 0-4 % faster in slot order.  WGT_NEAREST_K_SORT = 0 / 1 forces one.
  const uint32_t sort = env_u32("WGT_NEAREST_K_SORT", 2);
  p.sort = (sort < 2 ? sort : (p.k > 0 ? 1u : 0u));
  // the kernel's list indices rely on both, whoever calls
  if (!out.count && !lists) return "no nearest field asked for";
  if (lists && (k < 1 || k > WGT_NEAREST_MAX_K)) return "k out of range (1..32)";
  const size_t lds = nearest_k_lds_bytes(sc.stack, p.k, p.words);
  if (lds > kNearestKLdsPerWorkgroup)
    return "a stack of " + std::to_string(sc.stack) + " entries and a list of " + std::to_string(p.k) +
           " triangles per lane need " + std::to_string(lds) + " bytes of LDS, above a workgroup's " +
           std::to_string(kNearestKLdsPerWorkgroup);
  p.lds = (uint32_t)lds;
  return "";
}

void nearest_k_points_spec(const wgt_triangle* tris, uint32_t n_tris, uint32_t first_prim, const float* points,
                           const float* max_dist, uint32_t n, uint32_t k, const wgt_nearest_k_buffers& out) {
  const size_t N = n;
  const float inf = __builtin_inff();
  if (!nearest_k_lists(out)) k = 0;
  if (k > WGT_NEAREST_MAX_K) k = WGT_NEAREST_MAX_K;  // the entry point refused it
  for (size_t i = 0; i < N; ++i) {
    const f3 p{points[i], points[N + i], points[2 * N + i]};
    const float m = max_dist ? max_dist[i] : inf;
    // the first k of S by (d2, index), kept sorted
    float d2s[WGT_NEAREST_MAX_K];
    uint32_t ids[WGT_NEAREST_MAX_K];
    uint32_t len = 0, cnt = 0;
    // a NaN or infinite point: S is empty
    const bool finite = fabs_w(p.x) + fabs_w(p.y) + fabs_w(p.z) < inf;
    for (uint32_t t = 0; finite && t < n_tris; ++t) {
      const wgt_triangle& tr = tris[t];
      const float d2 = nearest_on_tri(p, f3{tr.v0[0], tr.v0[1], tr.v0[2]}, f3{tr.e1[0], tr.e1[1], tr.e1[2]},
                                      f3{tr.e2[0], tr.e2[1], tr.e2[2]}).d2;
      if (!nearest_k_member(d2, m)) continue;
      ++cnt;
      if (k == 0) continue;
      uint32_t j = len;
      if (len == k) {
        j = k - 1;
        if (!nearest_k_less(d2, t, d2s[j], ids[j])) continue;
      } else {
        ++len;
      }
      for (; j > 0 && nearest_k_less(d2, t, d2s[j - 1], ids[j - 1]); --j) {
        d2s[j] = d2s[j - 1];
        ids[j] = ids[j - 1];
      }
      d2s[j] = d2;
      ids[j] = t;
    }
    if (out.count) out.count[i] = cnt;
    for (uint32_t j = 0; j < k; ++j) {
      const bool have = j < len;
      NearestTri c{};
      if (have) {
        const wgt_triangle& tr = tris[ids[j]];
        c = nearest_on_tri(p, f3{tr.v0[0], tr.v0[1], tr.v0[2]}, f3{tr.e1[0], tr.e1[1], tr.e1[2]},
                           f3{tr.e2[0], tr.e2[1], tr.e2[2]});
      }
      if (out.prim) out.prim[j * N + i] = have ? first_prim + ids[j] : kNoHit;
      if (out.dist) out.dist[j * N + i] = have ? sqrt_rn(d2s[j]) : inf;
      if (out.pos) {
        out.pos[(3 * j + 0) * N + i] = have ? c.q.x : 0.0f;
        out.pos[(3 * j + 1) * N + i] = have ? c.q.y : 0.0f;
        out.pos[(3 * j + 2) * N + i] = have ? c.q.z : 0.0f;
      }
      if (out.uv) {
        out.uv[(2 * j + 0) * N + i] = have ? c.v : 0.0f;
        out.uv[(2 * j + 1) * N + i] = have ? c.w : 0.0f;
      }
    }
  }
}

const char* check_overlap_args(const void* query, const wgt_overlap_buffers* out, uint64_t k) {
  if (!query) return "null query triangles";
  if (!out) return "null output buffers";
  if (!out->hit && !out->count && !out->prim) return "no overlap field asked for";
  if (k > WGT_OVERLAP_MAX_K) return "k out of range (0..32)";
  if (k == 0 && out->prim) return "prim asked for with k == 0";
  if (k > 0 && !out->prim) return "k > 0 without prim";
  return nullptr;
}

std::string plan_overlap(const DevScene& sc, const void* query, const wgt_overlap_buffers* out, uint32_t n, uint64_t k,
                         OverlapPlan& p) {
  p = OverlapPlan{};
  p.n = n;
  if (const char* bad = check_overlap_args(query, out, k)) return bad;
  p.k = (uint32_t)k;
  p.any = (out->hit && !out->count && !out->prim) ? 1u : 0u;
  const size_t lds = overlap_lds_bytes(sc.stack, p.k);
  if (lds > kOverlapLdsPerWorkgroup)
    return "a stack of " + std::to_string(sc.stack) + " entries and a list of " + std::to_string(p.k) +
           " triangles per lane need " + std::to_string(lds) + " bytes of LDS, above a workgroup's " +
           std::to_string(kOverlapLdsPerWorkgroup);
  p.lds = (uint32_t)lds;
  return "";
}

StageLayout stage_overlap(const float* query, const wgt_overlap_buffers& out, uint32_t n, uint32_t k) {
  const size_t N = n;
  return stage_of("an overlap query", {{N * 36, query, nullptr}, {out.hit ? N : 0, nullptr, out.hit},
                                       {out.count ? N * 4 : 0, nullptr, out.count},
                                       {out.prim ? N * k * 4 : 0, nullptr, out.prim}});
}

void overlap_triangles_spec(const wgt_triangle* tris, uint32_t n_tris, uint32_t first_prim, const float* query,
                            uint32_t n, uint32_t k, const wgt_overlap_buffers& out) {
  const size_t N = n;
  if (!out.prim) k = 0;
  if (k > WGT_OVERLAP_MAX_K) k = WGT_OVERLAP_MAX_K;  // the entry point refused it
  for (size_t i = 0; i < N; ++i) {
    const f3 a0{query[i], query[N + i], query[2 * N + i]};
    const f3 a1{query[3 * N + i], query[4 * N + i], query[5 * N + i]};
    const f3 a2{query[6 * N + i], query[7 * N + i], query[8 * N + i]};
    // triangles come in index order, so the first k of S are its k lowest ids
    uint32_t cnt = 0;
    const bool ok = overlap_query_ok(a0, a1, a2);
    for (uint32_t t = 0; ok && t < n_tris; ++t) {
      const wgt_triangle& tr = tris[t];
      const f3 v0{tr.v0[0], tr.v0[1], tr.v0[2]}, e1{tr.e1[0], tr.e1[1], tr.e1[2]}, e2{tr.e2[0], tr.e2[1], tr.e2[2]};
      f3 lo, hi;
      tri_box(v0, e1, e2, lo, hi);
      if (!tri_overlap(a0, a1, a2, v0, e1, e2, lo, hi)) continue;
      if (cnt < k) out.prim[cnt * N + i] = first_prim + t;
      ++cnt;
    }
    if (out.hit) out.hit[i] = cnt > 0 ? 1 : 0;
    if (out.count) out.count[i] = cnt;
    for (size_t j = cnt; j < k; ++j) out.prim[j * N + i] = kNoHit;
  }
}

const char* check_overlap_self_args(const wgt_overlap_buffers* out, uint64_t k) {
  if (!out) return "null output buffers";
  if (!out->hit && !out->count && !out->prim) return "no overlap field asked for";
  if (k > WGT_OVERLAP_MAX_K) return "k out of range (0..32)";
  if (k == 0 && out->prim) return "prim asked for with k == 0";
  if (k > 0 && !out->prim) return "k > 0 without prim";
  return nullptr;
}

std::string plan_overlap_self(const DevScene& sc, const wgt_overlap_buffers* out, uint64_t k, OverlapSelfPlan& p) {
  p = OverlapSelfPlan{};
  p.n = sc.n_tris;
  if (const char* bad = check_overlap_self_args(out, k)) return bad;
  p.k = (uint32_t)k;
  p.any = (out->hit && !out->count && !out->prim) ? 1u : 0u;
  const size_t lds = overlap_lds_bytes(sc.stack, p.k);
  if (lds > kOverlapLdsPerWorkgroup)
    return "a stack of " + std::to_string(sc.stack) + " entries and a list of " + std::to_string(p.k) +
           " triangles per lane need " + std::to_string(lds) + " bytes of LDS, above a workgroup's " +
           std::to_string(kOverlapLdsPerWorkgroup);
  p.lds = (uint32_t)lds;
  return "";
}

StageLayout stage_overlap_self(const uint32_t* indices, const wgt_overlap_buffers& out, uint32_t n_tris, uint32_t k) {
  const size_t N = n_tris;
  return stage_of("a self-intersection query", {{indices ? N * 12 : 0, indices, nullptr}, {out.hit ? N : 0, nullptr, out.hit},
                                                {out.count ? N * 4 : 0, nullptr, out.count},
                                                {out.prim ? N * k * 4 : 0, nullptr, out.prim}});
}

void overlap_self_spec(const wgt_triangle* tris, uint32_t n_tris, uint32_t first_prim, const uint32_t* indices,
                       uint32_t k, const wgt_overlap_buffers& out) {
  const size_t N = n_tris;
  if (!out.prim) k = 0;
  if (k > WGT_OVERLAP_MAX_K) k = WGT_OVERLAP_MAX_K;  // the entry point refused it
  const auto rec = [&](uint32_t x, f3& v0, f3& e1, f3& e2) {
    const wgt_triangle& tr = tris[x];
    v0 = f3{tr.v0[0], tr.v0[1], tr.v0[2]}, e1 = f3{tr.e1[0], tr.e1[1], tr.e1[2]}, e2 = f3{tr.e2[0], tr.e2[1], tr.e2[2]};
  };
  for (uint32_t s = 0; s < n_tris; ++s) {
    f3 sv0, se1, se2, slo, shi;
    rec(s, sv0, se1, se2);
    tri_box(sv0, se1, se2, slo, shi);
    // triangles come in index order, so the first k of S_s are its k lowest ids
    uint32_t cnt = 0;
    for (uint32_t t = 0; t < n_tris; ++t) {
      if (t == s) continue;
      if (indices && self_adjacent(indices[3 * (size_t)s], indices[3 * (size_t)s + 1], indices[3 * (size_t)s + 2],
                                   indices[3 * (size_t)t], indices[3 * (size_t)t + 1], indices[3 * (size_t)t + 2]))
        continue;
      f3 tv0, te1, te2, tlo, thi;
      rec(t, tv0, te1, te2);
      tri_box(tv0, te1, te2, tlo, thi);
      if (!overlap_boxes(slo, shi, tlo.x, thi.x, tlo.y, thi.y, tlo.z, thi.z)) continue;
      if (!(s < t ? self_segments(sv0, se1, se2, tv0, te1, te2) : self_segments(tv0, te1, te2, sv0, se1, se2))) continue;
      if (cnt < k) out.prim[cnt * N + s] = first_prim + t;
      ++cnt;
    }
    if (out.hit) out.hit[s] = cnt > 0 ? 1 : 0;
    if (out.count) out.count[s] = cnt;
    for (size_t j = cnt; j < k; ++j) out.prim[j * N + s] = kNoHit;
  }
}

}  // namespace wgt
