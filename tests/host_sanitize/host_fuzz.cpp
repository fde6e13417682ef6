// host_fuzz.cpp — the product's host code under AddressSanitizer + UBSan (CPU only; built and
// run by tests/test_host_sanitize.py): the BVH builder over random, degenerate and extreme
// triangle sets, every stack budget and both collapses, with the device image of every tree it
// builds, the OBJ parser over valid, malformed and random
// text, the procedural meshes, the host C-ABI entry points (Cornell scene, triangle
// packing, OBJ and PNG writers), and the planning layer of the device calls (launch_plan.h: the
// numeric limits, the frame constants and knobs, the kernel form, the scene's device layout).
// Exits non-zero on a failed invariant; the sanitizers abort on the first finding.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../../include/wgt_api.h"
#include "../../webgputracer_amd/csrc/host/bvh.h"
#include "../../webgputracer_amd/csrc/host/launch_plan.h"
#include "../../webgputracer_amd/csrc/host/obj_loader.h"
#include "../../webgputracer_amd/csrc/host/procedural.h"

// wgt_runtime.cpp's entry points, which need the HIP runtime (Scene::InitBuffers references
// them; nothing here calls them)
namespace wgt {
void set_thread_error(const std::string&) {}
}
extern "C" const char* wgt_last_error(const wgt_ctx*) { return ""; }
extern "C" int wgt_upload_scene(wgt_ctx*, const wgt_quad*, uint32_t, const wgt_quad*, uint32_t, const wgt_sphere*,
                                uint32_t, const wgt_triangle*, uint32_t) {
  return WGT_E_INVALID;
}

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                          \
    }                                                                    \
  } while (0)

static std::vector<wgt_triangle> pack(const std::vector<float>& v) {  // 9 floats per triangle
  const uint32_t n = (uint32_t)(v.size() / 9);
  std::vector<wgt_triangle> t(n);
  const float col[3] = {0.5f, 0.5f, 0.5f};
  CHECK(wgt_make_triangles(v.data(), n, col, 0, nullptr, t.data()) == WGT_OK);
  return t;
}

// The device image of a built tree (wgt::DeviceImage), checked completely: the 128-B nodes and the
// 80-B compact records are the builder's with internal refs as byte offsets, and a node's level is
// its parent's + 1, saturating at 255.
static void check_image(const wgt::BvhOut& out) {
  const wgt::BvhImage im = wgt::DeviceImage(out);
  const bool sized = im.nodes.size() == out.nodes.size() && im.crecs.size() == (size_t)out.n_nodes * 20 &&
                     im.level.size() == out.n_nodes;
  CHECK(sized);
  if (!sized) return;
  CHECK(im.level[0] == 0);
  for (size_t i = 0; i < out.n_nodes; ++i) {
    const auto a = wgt::Node4(out.nodes, i), b = wgt::Node4(im.nodes, i);
    for (int s = 0; s < 4; ++s) {
      for (int c = 0; c < 3; ++c)
        CHECK(std::memcmp(&a.lo(c, s), &b.lo(c, s), 4) == 0 && std::memcmp(&a.hi(c, s), &b.hi(c, s), 4) == 0);
      CHECK(std::memcmp(&a.pad(s), &b.pad(s), 4) == 0);
      const int32_t r = a.ref(s), cr = out.crefs[i * 4 + s];
      CHECK(b.ref(s) == (r >= 0 ? r * 128 : r));
      int32_t rec;
      std::memcpy(&rec, &im.crecs[i * 20 + 16 + s], 4);
      CHECK(rec == (cr >= 0 ? cr * 80 : cr));
      if (r >= 0 && (size_t)r < out.n_nodes) CHECK(im.level[r] == std::min(255, im.level[i] + 1));
    }
    CHECK(std::memcmp(&im.crecs[i * 20], &out.cnodes[i * 16], 64) == 0);
  }
}

// Returns whether the build succeeded (its output checked).  `opt` carries the builder's tuning;
// the limits are set here.
static bool build(const std::vector<wgt_triangle>& t, uint32_t stack_limit, uint32_t narrow, wgt::BvhOptions opt = {}) {
  wgt::BvhOut out;
  std::string err;
  opt.max_depth = 24;
  opt.stack_limit = stack_limit;
  opt.narrow_limit = narrow;
  opt.narrow_ratio = 1.03;
  opt.origin_bound = 1e4;
  const bool ok = wgt::BuildBvh(t.data(), (uint32_t)t.size(), opt, out, err);
  if (!ok) {  // a refusal must say why
    CHECK(!err.empty());
    return false;
  }
  CHECK(out.n_nodes >= 1);
  CHECK(out.nodes.size() == (size_t)out.n_nodes * 32);
  CHECK(out.tris.size() == t.size() * 16);
  CHECK(out.stack_need <= 3u * 24u);
  CHECK(out.max_leaf >= 1 && out.max_leaf <= 8);
  // every triangle index appears once in the leaf-ordered records
  std::vector<int> seen(t.size(), 0);
  for (size_t i = 0; i < t.size(); ++i) {
    uint32_t idx;
    std::memcpy(&idx, &out.tris[i * 16 + 3], 4);
    CHECK(idx < t.size());
    if (idx < t.size()) ++seen[idx];
  }
  for (int s : seen) CHECK(s == 1);
  // the compact form: one record and 4 refs per node
  CHECK(out.cnodes.size() == (size_t)out.n_nodes * 16 && out.crefs.size() == (size_t)out.n_nodes * 4);
  check_image(out);
  return true;
}

static std::vector<float> soup(std::mt19937& g, uint32_t n, float spread, float size) {
  std::uniform_real_distribution<float> u(0.0f, spread);
  std::normal_distribution<float> e(0.0f, size);
  std::vector<float> v;
  for (uint32_t i = 0; i < n; ++i) {
    const float x = u(g), y = u(g), z = u(g);
    const float p[9] = {x, y, z, x + e(g), y + e(g), z + e(g), x + e(g), y + e(g), z + e(g)};
    v.insert(v.end(), p, p + 9);
  }
  return v;
}

static void fuzz_bvh() {
  std::mt19937 g(7);
  const uint32_t sizes[] = {1, 2, 3, 7, 8, 9, 17, 33, 257, 1000, 5000};
  for (uint32_t n : sizes) {
    for (uint32_t lim : {31u, 24u, 20u, 16u}) build(pack(soup(g, n, 500.0f, 20.0f)), lim, 0);
    build(pack(soup(g, n, 500.0f, 20.0f)), 31, 25);
  }
  // coincident triangles (no SAH split exists), zero-area ones, one plane, one line of centroids
  std::vector<float> same, flat, plane, line;
  for (uint32_t i = 0; i < 300; ++i) {
    const float a[9] = {0, 0, 0, 10, 0, 0, 0, 10, 0};
    same.insert(same.end(), a, a + 9);
    const float f = (float)i;
    const float b[9] = {f, f, f, f, f, f, f, f, f};  // a point
    flat.insert(flat.end(), b, b + 9);
    const float c[9] = {f, 0, 5, f + 1, 0, 5, f, 1, 5};
    plane.insert(plane.end(), c, c + 9);
    const float d[9] = {0, 0, f, 1, 0, f, 0, 1, f};
    line.insert(line.end(), d, d + 9);
  }
  for (auto* v : {&same, &flat, &plane, &line}) build(pack(*v), 31, 0);
  // extreme magnitudes within the scene limits (coordinates up to 2^40, edges up to 2^30)
  for (float s : {1e-30f, 1e-10f, 1.0f, 1e6f, 1e11f}) {
    std::vector<float> v = soup(g, 500, 1.0f, 0.01f);
    for (float& x : v) x *= s;
    build(pack(v), 31, 0);
  }
  // the collapses the defaults do not reach: the greedy one, and the optimal one merging BVH2
  // subtrees into leaves (a node weight of 2 makes merges pay)
  wgt::BvhOptions greedy, merge;
  greedy.collapse = wgt::BvhOptions::kGreedy;
  merge.dp_leaf = 8;
  merge.dp_node = 2.0;
  for (const wgt::BvhOptions& opt : {greedy, merge})
    for (uint32_t n : sizes) {
      for (uint32_t lim : {31u, 24u, 20u, 16u}) build(pack(soup(g, n, 500.0f, 20.0f)), lim, 0, opt);
      build(pack(soup(g, n, 500.0f, 20.0f)), 31, 25, opt);
    }
}

static void fuzz_obj() {
  std::vector<wgt::Vertex> vs;
  std::string err, warn;
  const char* texts[] = {
      "", "\n\n", "# only a comment\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n",
      "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0.5 0.5\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1 4/1/1\n",
      "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -3 -2 -1\n", "v 0 0 0\nf 1 2 3\n", "f 1 2 3\n", "v 1 2\nf 1 1 1\n",
      "v a b c\nf 1 2 3\n", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1/ 2// 3/x/\n", "v 0 0 0\nf 0 0 0\n",
      "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 4294967296 1 2\n", "v 1e39 -1e39 nan\nv 0 0 0\nv 1 1 1\nf 1 2 3\n",
      "v 0 0 0\r\nv 1 0 0\r\nv 0 1 0\r\nf 1 2 3\r\n", "g a\no b\nusemtl m\ns off\nmtllib x.mtl\n",
      "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2\n", "vt\nvn\nv\nf\n"};
  for (const char* t : texts) {
    vs.clear();
    (void)wgt::obj::ParseTriangulated(t, vs, err, warn);
    CHECK(vs.size() % 3 == 0);
  }
  std::mt19937 g(11);
  const char* tok[] = {"v", "vt", "vn", "f", "g", "o", "#", "1", "-1", "2/3", "4//5", "/", "//", "0.5", "-2.5e3",
                       "nan", "inf", "x", " ", "\t", "7/8/9", "-0", "99999999999", "\\"};
  for (int it = 0; it < 3000; ++it) {
    std::string s;
    const int lines = (int)(g() % 20);
    for (int l = 0; l < lines; ++l) {
      const int nt = (int)(g() % 6);
      for (int k = 0; k < nt; ++k) {
        s += tok[g() % (sizeof(tok) / sizeof(tok[0]))];
        s += ' ';
      }
      s += (g() % 7) ? "\n" : "\r\n";
    }
    vs.clear();
    (void)wgt::obj::ParseTriangulated(s, vs, err, warn);
    CHECK(vs.size() % 3 == 0);
  }
}

static void host_api() {
  wgt_quad l[8], q[64];
  wgt_sphere sp[8];
  uint32_t nl = 8, nq = 64, ns = 8;
  CHECK(wgt_scene_cornell(l, &nl, q, &nq, sp, &ns) == WGT_OK);
  uint32_t z = 0;
  CHECK(wgt_scene_cornell(l, &z, q, &nq, sp, &ns) == WGT_E_INVALID);  // capacity too small
  for (int kind = 0; kind < 2; ++kind) {
    uint32_t n = 0;
    CHECK(wgt_procedural_mesh(kind, kind ? 20000 : 5000, 1, nullptr, &n) == WGT_OK);
    std::vector<wgt_triangle> t(n);
    CHECK(wgt_procedural_mesh(kind, kind ? 20000 : 5000, 1, t.data(), &n) == WGT_OK);
    CHECK(build(t, 31, 0));  // the Cornell-box meshes build
    const char* path = "/tmp/wgt_host_fuzz.obj";
    CHECK(wgt_write_obj(path, t.data(), n) == WGT_OK);
    const float col[3] = {0.2f, 0.4f, 0.6f};
    uint32_t m = 0;
    CHECK(wgt_load_obj(path, col, nullptr, 0, nullptr, &m) == WGT_OK);
    CHECK(m == n);
    std::vector<wgt_triangle> r(m);
    CHECK(wgt_load_obj(path, col, nullptr, 0, r.data(), &m) == WGT_OK);
    uint32_t small = m ? m - 1 : 0;
    if (m) CHECK(wgt_load_obj(path, col, nullptr, 0, r.data(), &small) == WGT_E_INVALID);
    std::remove(path);
  }
  CHECK(wgt_procedural_mesh(2, 10, 1, nullptr, &nl) == WGT_E_INVALID);
  for (uint32_t w : {1u, 3u, 64u}) {
    std::vector<uint8_t> px((size_t)w * 5 * 4, 0x5a);
    CHECK(wgt_write_png("/tmp/wgt_host_fuzz.png", px.data(), w, 5) == WGT_OK);
  }
  std::remove("/tmp/wgt_host_fuzz.png");
  CHECK(wgt_write_png("/tmp/wgt_host_fuzz.png", nullptr, 1, 1) == WGT_E_INVALID);
  uint32_t n = 0;
  const float col[3] = {1, 1, 1};
  CHECK(wgt_load_obj("/nonexistent/wgt.obj", col, nullptr, 0, nullptr, &n) == WGT_E_IO);
}

// ---- the planning layer (launch_plan.h) ----

static bool starts(const std::string& msg, const char* prefix) { return msg.rfind(prefix, 0) == 0; }
static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static const char* const kKnobs[] = {"WGT_KERNEL", "WGT_PS_TO_TRAV", "WGT_PS_TO_SERVICE", "WGT_PS_SVC_FRAC",
                                     "WGT_TRI_RATIO", "WGT_CNODE", "WGT_PQ_REFILL", "WGT_PQ_LPT", "WGT_PQ_SVC_COST",
                                     "WGT_PQ_DEPTH", "WGT_PQ_LPT_ALL", "WGT_PS_WAVES", "WGT_PARK", "WGT_PS_CAP"};
static void clear_knobs() {
  for (const char* k : kKnobs) unsetenv(k);
}

struct Cornell {
  wgt_quad l[8], q[64];
  wgt_sphere sp[8];
  uint32_t nl = 8, nq = 64, ns = 8;
  Cornell() { CHECK(wgt_scene_cornell(l, &nl, q, &nq, sp, &ns) == WGT_OK); }
};
static std::vector<wgt_triangle> mesh500() {
  uint32_t n = 0;
  CHECK(wgt_procedural_mesh(0, 500, 1, nullptr, &n) == WGT_OK);
  std::vector<wgt_triangle> t(n);
  CHECK(wgt_procedural_mesh(0, 500, 1, t.data(), &n) == WGT_OK);
  return t;
}
// the reference camera (camera.cpp:64-70), origin and target scaled by s
static wgt_camera_param camera(float aspect, uint32_t spp, float s = 1.0f) {
  return wgt_camera_param{{278.0f * s, 278.0f * s, -800.0f * s}, 0.0f, {278.0f * s, 278.0f * s, 0.0f}, 0.0f,
                          aspect, 40.0f, spp, 0u};
}

// The limits of tests/test_gpu_numerics.py (test_render_limits_fail_cleanly,
// test_spp_beyond_sample_index_range_rejected) and their boundaries, refusals by message prefix.
static void plan_limits() {
  const Cornell c;
  const std::vector<wgt_triangle> mesh = mesh500();
  const auto quads = [&](const wgt_quad& q) { return wgt::check_scene_limits(&q, 1, nullptr, 0, nullptr, 0); };
  const auto tris = [&](const std::vector<wgt_triangle>& t) {
    return wgt::check_scene_limits(nullptr, 0, nullptr, 0, t.data(), (uint32_t)t.size());
  };
  const char* const quad_coord = "quad 0: position, edges and plane offset must be finite and within 2^40";
  CHECK(wgt::check_scene_limits(c.l, c.nl, c.sp, c.ns, mesh.data(), (uint32_t)mesh.size()).empty());
  CHECK(wgt::check_scene_limits(c.q, c.nq, nullptr, 0, nullptr, 0).empty());
  wgt_quad q = c.q[3];
  q.pos[1] = 0x1p40f;  // exactly 2^40
  CHECK(quads(q).empty());
  q.pos[1] = std::nextafter(0x1p40f, INFINITY);
  CHECK(starts(quads(q), quad_coord));
  q = c.q[3];
  q.pos[0] = NAN;
  CHECK(starts(quads(q), quad_coord));
  q = c.q[3];
  q.d = -0x1p42f;  // the plane offset: up to 2^42
  CHECK(quads(q).empty());
  q.d = std::nextafter(0x1p42f, INFINITY);
  CHECK(starts(quads(q), quad_coord));
  q = c.q[3];
  q.norm[1] = 2.0f;
  CHECK(quads(q).empty());
  q.norm[1] = 3.0f;
  CHECK(starts(quads(q), "quad 0: normal components must be within 2 (a unit normal) or NaN"));
  q.norm[0] = q.norm[1] = q.norm[2] = NAN;  // a degenerate quad
  CHECK(quads(q).empty());
  wgt_sphere s = c.sp[0];
  s.radius = INFINITY;
  CHECK(starts(wgt::check_scene_limits(nullptr, 0, &s, 1, nullptr, 0),
               "sphere 0: center and radius must be finite and within 2^40"));
  std::vector<wgt_triangle> t = mesh;
  t[7].v0[1] = INFINITY;
  CHECK(starts(tris(t), "triangle 7: vertices must be finite and within 2^40"));
  t = mesh;
  t[3].e2[2] = 0x1p30f;
  CHECK(tris(t).empty());
  t[3].e2[2] = 0x1p31f;
  CHECK(starts(tris(t), "triangle 3: edge components must be within 2^30"));

  const auto frame = [](const wgt_camera_param& cam, uint32_t W, uint32_t H) {
    return wgt::check_frame_args(cam, W, H, 8, 4);
  };
  CHECK(frame(camera(1.0f, 1), 8, 8).empty());
  CHECK(wgt::check_frame_args(camera(1.0f, 1), 0, 8, 8, 8) == "empty frame");
  CHECK(wgt::check_frame_args(camera(1.0f, 1), 8, 8, 8, 0) == "empty tile");
  wgt_camera_param cam = camera(1.0f, 1);
  cam.origin[0] = NAN;
  CHECK(starts(frame(cam, 8, 8), "camera origin and target must be finite and within 2^40"));
  CHECK(starts(frame(camera(NAN, 1), 8, 8), "NaN camera parameter"));
  CHECK(starts(frame(camera(1.0f, 1), 65536, 4), "frame width and height must be <= 65535"));
  CHECK(frame(camera(1.0f, 1), 65535, 4).empty());
  for (uint32_t spp : {0xFFFFFFFFu, 0xFFFFFF80u})
    CHECK(starts(frame(camera(1.0f, spp), 8, 8), "spp too large (u32(sqrt(f32(spp))) must be <= 65535)"));
  CHECK(starts(frame(camera(1.0f, 1, 0x1p24f), 8, 8), "camera: primary ray directions must be finite and within 2^32"));
  CHECK(frame(camera(1.0f, 1, 0x1p20f), 8, 8).empty());
}

// make_frame: the reference camera's frame, and the knobs' defaults and clamps.
static void plan_frame() {
  clear_knobs();
  const wgt::DevFrame fr = wgt::make_frame(camera(16.0f / 9.0f, 4), 48, 27);
  // origin, pixel_origin, pixel_delta_u, pixel_delta_v, recip_sqrt_spp, fspp, inv_fspp, then sqrt_spp: make_frame of
  // commit 545344f41999e1fc858e5f5cf0031f04c4872bf1 (wgt_runtime.cpp, the library's flags), printed by a program
  const uint32_t want[15] = {0x438b0000u, 0x438b0000u, 0xc4480000u, 0x4444372eu, 0x440b9914u, 0x00000000u,
                             0xc1ac8c80u, 0x00000000u, 0x00000000u, 0x80000000u, 0xc1ac8c80u, 0x80000000u,
                             0x3f000000u, 0x40800000u, 0x3e800000u};
  const float got[15] = {fr.ox,  fr.oy,  fr.oz,  fr.pox, fr.poy, fr.poz,         fr.dux,  fr.duy,
                         fr.duz, fr.dvx, fr.dvy, fr.dvz, fr.recip_sqrt_spp, fr.fspp, fr.inv_fspp};
  for (int i = 0; i < 15; ++i) CHECK(bits(got[i]) == want[i]);
  CHECK(fr.sqrt_spp == 2u && fr.W == 48u && fr.H == 27u);
  CHECK(fr.kernel == 2u && fr.ps_svc_frac == 16u && fr.tri_ratio == 100u && fr.cnode == 1u && fr.pq_lpt == 1u &&
        fr.pq_svc_cost == 7u && fr.pq_depth == 6u && fr.pq_lpt_all == 1u);
  CHECK(fr.ps_to_trav == 0u && fr.ps_to_service == 0u && fr.pq_refill == 0u);
  const wgt::DevFrame tf = wgt::tile_frame(camera(16.0f / 9.0f, 4), 48, 27, 16, 8, 3);
  CHECK(tf.tw == 16u && tf.th == 8u && tf.n_tiles == 3u && bits(tf.pox) == want[3]);
  const auto with = [](const char* knob, const char* value) {
    setenv(knob, value, 1);
    const wgt::DevFrame f = wgt::make_frame(camera(1.0f, 1), 8, 8);
    unsetenv(knob);
    return f;
  };
  CHECK(with("WGT_TRI_RATIO", "0").tri_ratio == 1u);
  CHECK(with("WGT_PQ_DEPTH", "0").pq_depth == 1u);
  CHECK(with("WGT_PQ_DEPTH", "999").pq_depth == (uint32_t)wgt::kRayDepth);
  CHECK(with("WGT_KERNEL", "").kernel == 2u && with("WGT_KERNEL", "1").kernel == 1u);
}

// ps_form_for and fill_bvh_info on trees whose counts are set by hand.
static void plan_form() {
  clear_knobs();
  const auto form = [](uint32_t n_nodes, uint32_t n_tris, uint32_t stack_need) {
    wgt::BvhOut b;
    b.n_nodes = n_nodes;
    b.stack_need = stack_need;
    return wgt::ps_form_for(b, n_tris);
  };
  CHECK(form(100, 1000, 9).waves == 6u && form((1u << 16) - 1, (1u << 20) - 1, 9).waves == 6u);
  CHECK(form(1u << 16, 1000, 9).waves == 5u && form(100, 1u << 20, 9).waves == 5u);
  wgt::PsForm f = form(100, 1000, 9);
  CHECK(f.tris && !f.park && f.cap == 10u);
  CHECK(form(100, 1000, 0).cap == 2u);  // stack_entries: max(stack_need, 1) + 1
  setenv("WGT_PS_WAVES", "5", 1);
  CHECK(form(100, 1000, 9).waves == 5u);
  unsetenv("WGT_PS_WAVES");
  wgt::BvhOut none;
  f = wgt::ps_form_for(none, 0);
  CHECK(!f.tris && f.waves == (uint32_t)wgt::kPsWavesNoTris && !f.park);
  wgt_scene_info in;
  std::memset(&in, 0xff, sizeof in);
  wgt::fill_bvh_info(none, 0, f, in);
  CHECK(in.n_tris == 0 && in.bvh_nodes == 0 && in.bvh_width == 0 && in.bvh_stack == 0 && in.ps_waves == 0 &&
        in.ps_park == 0 && in.ps_stack == 0 && in.bvh_compact == 0);
  setenv("WGT_PARK", "1", 1);
  for (uint32_t need : {1u, 2u, 9u, 17u, 18u, 30u})
    for (uint32_t nodes : {100u, 1u << 16}) {
      f = form(nodes, 1000, need);
      const uint32_t whole = std::max(need, 1u) + 1u, room = wgt::ps_cap_max(f.waves);
      CHECK(f.park && f.cap >= wgt::kMinPsCap && f.cap <= std::max(room, wgt::kMinPsCap));
      CHECK(f.cap == std::max(std::min(whole, room), wgt::kMinPsCap));
    }
  setenv("WGT_PS_CAP", "3", 1);
  CHECK(form(100, 1000, 30).cap == 8u);
  setenv("WGT_PS_CAP", "12", 1);
  CHECK(form(100, 1000, 30).cap == 12u);
  setenv("WGT_PS_CAP", "99", 1);
  CHECK(form(100, 1000, 30).cap == wgt::ps_cap_max(6));
  clear_knobs();
}

// pack_scene and bind_scene: the layout, the image's bytes and the DevScene of an upload.
static void check_pack(const Cornell& c, const std::vector<wgt_triangle>& tris) {
  const uint32_t nt = (uint32_t)tris.size();
  wgt::BvhOut bvh;
  if (nt) {
    const double ext = std::max(wgt::scene_extent(c.l, c.nl, c.sp, c.ns, tris.data(), nt),
                                wgt::scene_extent(c.q, c.nq, nullptr, 0, nullptr, 0));
    CHECK(wgt::build_bvh(tris.data(), nt, ext, bvh).empty());
  }
  const wgt::BvhImage im = wgt::DeviceImage(bvh);
  const wgt::ScenePlan p = wgt::pack_scene(c.l, c.nl, c.q, c.nq, c.sp, c.ns, nt, bvh, im);
  std::vector<char> lq((size_t)(c.nl + c.nq) * sizeof(wgt_quad));  // lights, then quads
  std::memcpy(lq.data(), c.l, c.nl * sizeof(wgt_quad));
  std::memcpy(lq.data() + c.nl * sizeof(wgt_quad), c.q, c.nq * sizeof(wgt_quad));
  const struct { const void* src; size_t bytes; } part[wgt::kSceneParts] = {
      {lq.data(), lq.size()},           {c.sp, c.ns * sizeof(wgt_sphere)},    {im.nodes.data(), im.nodes.size() * 4},
      {bvh.tris.data(), bvh.tris.size() * 4}, {bvh.tshade.data(), bvh.tshade.size() * 4},
      {im.crecs.data(), im.crecs.size() * 4}, {im.level.data(), im.level.size()}};
  std::vector<char> covered(p.host.size(), 0);
  size_t end = 0;
  for (int i = 0; i < wgt::kSceneParts; ++i) {
    CHECK(p.off[i] % 256 == 0 && p.off[i] >= end && p.off[i] + part[i].bytes <= p.host.size());
    if (p.off[i] + part[i].bytes > p.host.size()) return;
    end = p.off[i] + part[i].bytes;
    if (part[i].bytes) CHECK(std::memcmp(p.host.data() + p.off[i], part[i].src, part[i].bytes) == 0);
    std::fill(covered.begin() + p.off[i], covered.begin() + end, 1);
  }
  CHECK(nt ? part[wgt::kPartNodes].bytes > 0 && part[wgt::kPartLevel].bytes == bvh.n_nodes
           : part[wgt::kPartNodes].bytes + part[wgt::kPartTris].bytes + part[wgt::kPartLevel].bytes == 0);
  for (size_t i = 0; i < p.host.size(); ++i)
    if (!covered[i]) CHECK(p.host[i] == 0);  // padding

  wgt::DevScene sc = p.sc;
  CHECK(!sc.quads && !sc.spheres && !sc.nodes && !sc.tris && !sc.tshade && !sc.cnodes && !sc.node_level);
  std::vector<char> dev(p.host.size() + 1);  // stands for the device allocation
  wgt::bind_scene(sc, p.off, dev.data());
  const void* const bound[wgt::kSceneParts] = {sc.quads, sc.spheres, sc.nodes, sc.tris,
                                               sc.tshade, sc.cnodes, sc.node_level};
  for (int i = 0; i < wgt::kSceneParts; ++i) CHECK(bound[i] == dev.data() + p.off[i]);
  CHECK(sc.n_lights == c.nl && sc.n_quads == c.nq && sc.n_spheres == c.ns && sc.n_tris == nt &&
        sc.n_nodes == bvh.n_nodes);
  CHECK(bits(sc.cstep) == bits(bvh.cstep) && bits(sc.cbound) == bits(bvh.cbound) && sc.rcstep == 1.0f / sc.cstep);
  CHECK(sc.last_sphere_emissive == (c.sp[c.ns - 1].emissive > 0.0f ? 1u : 0u));
  // the reference light (scene.cpp:17): 130 x 105, axis-aligned
  CHECK(sc.light_area == 13650.0f);
  CHECK(sc.stack == std::max(bvh.stack_need, 1u) + 1u);
  const wgt::PsForm f = wgt::ps_form_for(bvh, nt), g = wgt::ps_form(sc);
  CHECK(sc.ps_waves == f.waves && sc.ps_park == (f.park ? 1u : 0u) && sc.ps_cap == f.cap);
  CHECK(g.tris == f.tris && g.waves == f.waves && g.park == f.park && g.cap == f.cap);
  CHECK(sc.ps_waves == (nt ? 6u : (uint32_t)wgt::kPsWavesNoTris));
}
static void plan_pack() {
  const Cornell c;
  clear_knobs();
  check_pack(c, {});  // no triangles: the tree's parts are empty, their sources null
  check_pack(c, mesh500());
  setenv("WGT_PARK", "1", 1);
  check_pack(c, mesh500());
  clear_knobs();
}

int main() {
  fuzz_bvh();
  fuzz_obj();
  host_api();
  plan_limits();
  plan_frame();
  plan_form();
  plan_pack();
  std::printf("host_fuzz: %s (%d failed checks)\n", g_fail ? "FAIL" : "ok", g_fail);
  return g_fail ? 1 : 0;
}
