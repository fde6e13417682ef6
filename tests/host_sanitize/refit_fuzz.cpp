// refit_fuzz.cpp — the host side of the BVH refit under AddressSanitizer + UBSan (CPU only; built
// and run by tests/test_refit_sanitize.py): RefitBvh over seeded random meshes and motions,
// including non-finite input, and what wgt_update_triangles plans on the host (launch_plan.h
// refit_bvh, compact_bound, refit_levels) with the export of a device image (ExportImage).
// Exits non-zero on a failed invariant; the sanitizers abort on the first finding.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../include/wgt_api.h"
#include "../../webgputracer_amd/csrc/host/bvh.h"
#include "../../webgputracer_amd/csrc/host/launch_plan.h"

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                          \
    }                                                                    \
  } while (0)

using Verts = std::vector<float>;  // 9 per triangle: v0, v1, v2

static std::vector<wgt_triangle> pack(const Verts& v) {
  std::vector<wgt_triangle> t(v.size() / 9);
  for (size_t i = 0; i < t.size(); ++i) {
    const float* p = &v[i * 9];
    wgt_triangle& o = t[i];
    for (int c = 0; c < 3; ++c) {
      o.v0[c] = p[c];
      o.e1[c] = p[3 + c] - p[c];
      o.e2[c] = p[6 + c] - p[c];
      o.face_norm[c] = c == 1 ? 1.0f : 0.0f;
      o.col[c] = 0.25f * (float)(c + 1) + (float)(i % 7);
    }
    o.v0[3] = o.e1[3] = o.e2[3] = o.face_norm[3] = 1.0f;
    o.emissive = (float)(i % 2);
  }
  return t;
}

static Verts soup(std::mt19937& g, uint32_t n, float spread, float size) {
  std::uniform_real_distribution<float> u(0.0f, spread);
  std::normal_distribution<float> e(0.0f, size);
  Verts v;
  for (uint32_t i = 0; i < n; ++i) {
    const float x = u(g), y = u(g), z = u(g);
    const float p[9] = {x, y, z, x + e(g), y + e(g), z + e(g), x + e(g), y + e(g), z + e(g)};
    v.insert(v.end(), p, p + 9);
  }
  return v;
}

template <class T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static bool same_tree(const wgt::BvhOut& a, const wgt::BvhOut& b) {
  return same(a.nodes, b.nodes) && same(a.tris, b.tris) && same(a.cnodes, b.cnodes) && same(a.crefs, b.crefs) &&
         same(a.tshade, b.tshade) && std::memcmp(&a.cstep, &b.cstep, 4) == 0 && std::memcmp(&a.cbound, &b.cbound, 4) == 0 &&
         a.n_nodes == b.n_nodes && a.stack_need == b.stack_need && a.max_depth == b.max_depth && a.sah_cost == b.sah_cost;
}

struct Box6 {
  float lo[3], hi[3];
};
// The union of the record boxes below slot (node k, slot s), top-down: independent of RefitBvh's pass.
static Box6 below(const wgt::BvhOut& t, int32_t ref) {
  const float inf = std::numeric_limits<float>::infinity();
  Box6 b{{inf, inf, inf}, {-inf, -inf, -inf}};
  const auto grow = [&](const float* lo, const float* hi) {
    for (int a = 0; a < 3; ++a) {
      b.lo[a] = std::min(b.lo[a], lo[a]);
      b.hi[a] = std::max(b.hi[a], hi[a]);
    }
  };
  if (ref < 0) {
    for (uint32_t j = wgt::leaf_first(ref), end = j + wgt::leaf_count(ref); j < end; ++j) {
      const float* o = &t.tris[(size_t)j * 16];
      const float lo[3] = {o[7], o[11], o[12]};
      grow(lo, &o[13]);
    }
    return b;
  }
  const auto n = wgt::Node4(t.nodes, (size_t)ref);
  for (int s = 0; s < 4; ++s)
    if (n.live(s)) {
      const Box6 c = below(t, n.ref(s));
      grow(c.lo, c.hi);
    }
  return b;
}

// Every invariant of a refit tree against the triangles it was refit to and the tree before.
static void check_refit(const wgt::BvhOut& t, const wgt::BvhOut& built, const std::vector<wgt_triangle>& tris, double origin_bound) {
  CHECK(same(t.crefs, built.crefs) && t.n_nodes == built.n_nodes && t.sah_cost == built.sah_cost);
  CHECK(t.tris.size() == built.tris.size() && t.nodes.size() == built.nodes.size());
  for (size_t i = 0; i < tris.size(); ++i) {
    uint32_t idx, was;
    std::memcpy(&idx, &t.tris[i * 16 + 3], 4);
    std::memcpy(&was, &built.tris[i * 16 + 3], 4);
    CHECK(idx == was && idx < tris.size());
    if (idx >= tris.size()) return;
    wgt::f3 lo, hi;
    const wgt_triangle& r = tris[idx];
    wgt::tri_box(wgt::f3{r.v0[0], r.v0[1], r.v0[2]}, wgt::f3{r.e1[0], r.e1[1], r.e1[2]}, wgt::f3{r.e2[0], r.e2[1], r.e2[2]}, lo, hi);
    const float want[16] = {r.v0[0], r.v0[1], r.v0[2], 0.0f, r.e1[0], r.e1[1], r.e1[2], lo.x,
                            r.e2[0], r.e2[1], r.e2[2], lo.y, lo.z,    hi.x,    hi.y,    hi.z};
    for (int k = 0; k < 16; ++k)
      if (k != 3) CHECK(std::memcmp(&want[k], &t.tris[i * 16 + k], 4) == 0);
    CHECK(t.tshade[(size_t)idx * 8 + 3] == r.emissive && t.tshade[(size_t)idx * 8 + 4] == r.col[0]);
  }
  double M = std::max(origin_bound, 0x1p-60);
  for (uint32_t k = 0; k < t.n_nodes; ++k) {
    const auto n = wgt::Node4(t.nodes, k), was = wgt::Node4(built.nodes, k);
    for (int s = 0; s < 4; ++s) {
      CHECK(n.ref(s) == was.ref(s) && n.live(s) == was.live(s));
      if (!n.live(s)) continue;
      const Box6 b = below(t, n.ref(s));
      for (int a = 0; a < 3; ++a) {
        CHECK(std::memcmp(&b.lo[a], &n.lo(a, s), 4) == 0 && std::memcmp(&b.hi[a], &n.hi(a, s), 4) == 0);
        M = std::max({M, 2.0 * std::fabs((double)n.lo(a, s)), 2.0 * std::fabs((double)n.hi(a, s))});
      }
    }
  }
  CHECK((float)M == t.cbound);
  CHECK(wgt::compact_bound(origin_bound / 4.0, &t.nodes[0]) == M);  // the root alone gives it
  // the decoded compact planes keep the margin
  const double G = std::ldexp(M, -21), s = (double)t.cstep;
  int frac_exp;
  CHECK(std::frexp(t.cstep, &frac_exp) == 0.5f);
  for (uint32_t k = 0; k < t.n_nodes; ++k) {
    const auto n = wgt::Node4(t.nodes, k);
    const uint32_t* q = &t.cnodes[(size_t)k * 16];
    for (int a = 0; a < 3; ++a) {
      float org;
      std::memcpy(&org, &q[a], 4);
      const double orgd = (double)org * s;
      for (int i = 0; i < 4; ++i) {
        const uint32_t lo_h = (q[4 + 4 * a + i / 2] >> (16 * (i % 2))) & 0xffffu;
        const uint32_t hi_h = (q[4 + 4 * a + 2 + i / 2] >> (16 * (i % 2))) & 0xffffu;
        if (!n.live(i)) {
          CHECK(lo_h == 0x7c00u && hi_h == 0x7c00u);
          continue;
        }
        CHECK(orgd + (double)wgt::half_bits_to_float(lo_h) * s <= (double)n.lo(a, i) - G);
        CHECK(orgd + (double)wgt::half_bits_to_float(hi_h) * s >= (double)n.hi(a, i) + G);
      }
    }
  }
}

static void check_levels(const wgt::BvhOut& t) {
  const wgt::BvhImage im = wgt::DeviceImage(t);
  std::vector<uint32_t> order, begin;
  CHECK(wgt::refit_levels(im.level.data(), t.n_nodes, order, begin).empty());
  CHECK(order.size() == t.n_nodes && !begin.empty() && begin.front() == 0 && begin.back() == t.n_nodes);
  std::vector<int> seen(t.n_nodes, 0);
  for (size_t l = 0; l + 1 < begin.size(); ++l) {
    CHECK(begin[l] < begin[l + 1]);
    for (uint32_t j = begin[l]; j < begin[l + 1] && j < order.size(); ++j) {
      CHECK(order[j] < t.n_nodes);
      if (order[j] >= t.n_nodes) continue;
      CHECK(im.level[order[j]] == l);
      ++seen[order[j]];
    }
  }
  for (int s : seen) CHECK(s == 1);
  // the export inverts the image's refs
  std::vector<float> nodes(t.nodes.size());
  std::vector<uint32_t> cn(t.cnodes.size());
  std::vector<int32_t> cr(t.crefs.size());
  wgt::ExportImage(im.nodes.data(), im.crecs.data(), t.n_nodes, nodes.data(), cn.data(), cr.data());
  CHECK(same(nodes, t.nodes) && same(cn, t.cnodes) && same(cr, t.crefs));
  wgt::ExportImage(im.nodes.data(), im.crecs.data(), t.n_nodes, nullptr, nullptr, nullptr);
  std::vector<uint8_t> deep(im.level);
  deep.back() = 255;
  CHECK(!wgt::refit_levels(deep.data(), t.n_nodes, order, begin).empty());
}

static Verts moved(const Verts& v, int motion, std::mt19937& g) {
  Verts o = v;
  float lo[3] = {v[0], v[1], v[2]}, hi[3] = {v[0], v[1], v[2]};
  for (size_t i = 0; i < v.size(); ++i) {
    lo[i % 3] = std::min(lo[i % 3], v[i]);
    hi[i % 3] = std::max(hi[i % 3], v[i]);
  }
  const float size = std::max({hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]});
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  for (size_t i = 0; i < v.size(); ++i) {
    const int c = (int)(i % 3);
    switch (motion) {
      case 0: break;                                                     // identity
      case 1: o[i] = v[i] + (c == 0 ? 1000.0f : 0.0f); break;            // translation
      case 2: o[i] = lo[c] + (v[i] - lo[c]) * 0x1p-6f; break;            // shrink about a corner
      case 3: o[i] = lo[c] + (v[i] - lo[c]) * 8.0f; break;               // scale by 8
      case 4: o[i] = v[i] + u(g) * 0.05f * size; break;                  // jitter
      case 5: o[i] = v[i - (i % 9) + (size_t)c]; break;                  // collapsed to v0
      case 6: o[i] = u(g) * 1e6f; break;                                 // an unrelated soup: the worst tree
      default: o[i] = -v[i] * 0x1p-20f; break;                           // mirrored and tiny
    }
  }
  return o;
}

static void fuzz_refit() {
  std::mt19937 g(11);
  const uint32_t sizes[] = {1, 2, 8, 9, 33, 257, 1000, 3000};
  for (uint32_t n : sizes) {
    const Verts va = soup(g, n, n % 2 ? 500.0f : 3.0f, n % 2 ? 20.0f : 0.5f);
    const std::vector<wgt_triangle> A = pack(va);
    const double ext = wgt::scene_extent(nullptr, 0, nullptr, 0, A.data(), n);
    wgt::BvhOut built;
    CHECK(wgt::build_bvh(A.data(), n, ext, built).empty());
    if (built.n_nodes == 0) continue;
    check_levels(built);
    wgt::BvhOut t = built;
    CHECK(wgt::refit_bvh(A.data(), n, ext, t).empty());
    CHECK(same_tree(t, built));  // to the build's triangles: the build, bit for bit
    for (int motion = 0; motion < 8; ++motion) {
      const std::vector<wgt_triangle> B = pack(moved(va, motion, g));
      const double eb = std::max(wgt::scene_extent(nullptr, 0, nullptr, 0, B.data(), n), n % 3 ? 0.0 : 555.0);
      CHECK(wgt::refit_bvh(B.data(), n, eb, t).empty());  // refits accumulate: t was refit before
      check_refit(t, built, B, 4.0 * eb);
    }
    CHECK(wgt::refit_bvh(A.data(), n, ext, t).empty());
    CHECK(same_tree(t, built));  // and back
    // non-finite and overflowing input: refused with a reason, the tree untouched
    const float bad[] = {std::numeric_limits<float>::quiet_NaN(), std::numeric_limits<float>::infinity(),
                         -std::numeric_limits<float>::infinity(), 3.3e38f};
    for (float b : bad)
      for (int field = 0; field < 3; ++field) {
        std::vector<wgt_triangle> B = A;
        wgt_triangle& r = B[g() % n];
        (field == 0 ? r.v0 : field == 1 ? r.e1 : r.e2)[g() % 3] = b;
        std::string err;
        const bool ok = wgt::RefitBvh(t, B.data(), n, 4.0 * ext, err);
        // a NaN edge beside finite vertices leaves min/max finite (tri_box's comparisons drop it), as in a build
        CHECK(ok || !err.empty());
        if (!ok) CHECK(same_tree(t, built));
        else CHECK(wgt::refit_bvh(A.data(), n, ext, t).empty() && same_tree(t, built));
        if (field == 0) CHECK(!ok);
      }
    std::string err;
    CHECK(!wgt::RefitBvh(t, A.data(), n + 1, 4.0 * ext, err) && !err.empty());
    CHECK(!wgt::RefitBvh(t, A.data(), 0, 4.0 * ext, err));
    wgt::BvhOut none;
    CHECK(!wgt::RefitBvh(none, A.data(), n, 4.0 * ext, err));
    CHECK(same_tree(t, built));
  }
}

int main() {
  fuzz_refit();
  if (g_fail) {
    std::fprintf(stderr, "refit_fuzz: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("refit_fuzz: ok\n");
  return 0;
}
