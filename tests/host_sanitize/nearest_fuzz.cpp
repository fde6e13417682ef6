// nearest_fuzz.cpp — the host side of the closest-point query under AddressSanitizer + UBSan (CPU only;
// built and run by tests/test_nearest_sanitize.py): the definition's brute force (launch_plan.h
// nearest_points_spec over wgt_nearest.h) on seeded random, degenerate, NaN and huge inputs with every
// subset of the output fields, and what wgt_nearest_points plans on the host (check_nearest_args in
// its order, plan_nearest_stage).  Exits non-zero on a failed invariant; the sanitizers abort on the
// first finding.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../include/wgt_api.h"
#include "../../webgputracer_amd/csrc/host/launch_plan.h"

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                          \
    }                                                                    \
  } while (0)

static const float kInf = std::numeric_limits<float>::infinity();
static const float kNan = std::numeric_limits<float>::quiet_NaN();

// kind 0: a soup in the Cornell box; 1: zero-area (collinear, or a point); 2: huge (coordinates to
// 2^40, edges to 2^30); 3: tiny (denormal edges); 4: NaN and infinite fields among ordinary ones.
static std::vector<wgt_triangle> mesh(std::mt19937& g, int kind, uint32_t n) {
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  std::vector<wgt_triangle> t(n);
  for (uint32_t i = 0; i < n; ++i) {
    wgt_triangle& r = t[i];
    std::memset(&r, 0, sizeof r);
    float s = 20.0f, c = 280.0f;
    if (kind == 2) s = 0x1p30f, c = 0x1p39f;
    if (kind == 3) s = 0x1p-140f, c = 1.0f;
    for (int a = 0; a < 3; ++a) {
      r.v0[a] = c + c * u(g);
      r.e1[a] = s * u(g);
      r.e2[a] = s * u(g);
    }
    if (kind == 1)
      for (int a = 0; a < 3; ++a) r.e2[a] = (i & 1) ? r.e1[a] : 0.0f, r.e1[a] = (i & 2) ? r.e1[a] : 0.0f;
    if (kind == 4 && i % 3 == 0) r.v0[i % 3] = (i & 4) ? kNan : kInf;
    if (kind == 4 && i % 5 == 0) r.e1[i % 3] = (i & 8) ? kNan : -kInf;
  }
  return t;
}

static std::vector<float> points(std::mt19937& g, int kind, uint32_t n) {
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  std::vector<float> p((size_t)3 * n);
  const float scale[] = {600.0f, 1e7f, 0x1p41f, 3e38f, 1e-30f};
  for (size_t i = 0; i < p.size(); ++i) p[i] = scale[kind % 5] * u(g);
  if (kind >= 5)
    for (uint32_t i = 0; i < n; ++i) {
      if (i % 4 == 0) p[i] = kNan;
      if (i % 4 == 1) p[(size_t)n + i] = kInf;
      if (i % 4 == 2) p[2 * (size_t)n + i] = -kInf;
    }
  return p;
}

static void run_spec(std::mt19937& g, int mk, int pk, uint32_t nt, uint32_t n) {
  using namespace wgt;
  const std::vector<wgt_triangle> T = mesh(g, mk, nt);
  const std::vector<float> P = points(g, pk, n);
  std::vector<float> lim(n);
  std::uniform_real_distribution<float> u(0.0f, 1.0f);
  for (uint32_t i = 0; i < n; ++i) {
    const float m[] = {kInf, 0.0f, -1.0f, kNan, 1e3f * u(g), 1e30f};
    lim[i] = m[i % 6];
  }
  const uint32_t first = 17;
  // the full record, with exactly-sized buffers, then every other subset of the fields against it
  std::vector<uint32_t> prim(n);
  std::vector<float> dist(n), pos((size_t)3 * n), uv((size_t)2 * n);
  for (int radius = 0; radius < 2; ++radius) {
    const float* md = radius ? lim.data() : nullptr;
    const wgt_nearest_buffers all{prim.data(), dist.data(), pos.data(), uv.data()};
    nearest_points_spec(T.data(), nt, first, P.data(), md, n, all);
    for (uint32_t i = 0; i < n; ++i) {
      const bool miss = prim[i] == kNoHit;
      CHECK(miss || (prim[i] >= first && prim[i] < first + nt));
      CHECK(miss ? dist[i] == kInf : (dist[i] >= 0.0f && dist[i] < kInf));
      if (radius && !miss) CHECK(dist[i] < lim[i]);
      if (radius && !(lim[i] > 0.0f)) CHECK(miss);
      if (miss) CHECK(pos[i] == 0.0f && pos[n + i] == 0.0f && pos[2 * (size_t)n + i] == 0.0f && uv[i] == 0.0f && uv[n + i] == 0.0f);
      const bool odd = !(std::isfinite(P[i]) && std::isfinite(P[n + i]) && std::isfinite(P[2 * (size_t)n + i]));
      if (odd && mk != 4) CHECK(miss);
    }
    for (int mask = 1; mask < 15; ++mask) {
      std::vector<uint32_t> prim1(mask & 1 ? n : 0);
      std::vector<float> dist1(mask & 2 ? n : 0), pos1(mask & 4 ? (size_t)3 * n : 0), uv1(mask & 8 ? (size_t)2 * n : 0);
      const wgt_nearest_buffers some{mask & 1 ? prim1.data() : nullptr, mask & 2 ? dist1.data() : nullptr,
                                     mask & 4 ? pos1.data() : nullptr, mask & 8 ? uv1.data() : nullptr};
      nearest_points_spec(T.data(), nt, first, P.data(), md, n, some);
      if (mask & 1) CHECK(std::memcmp(prim1.data(), prim.data(), (size_t)n * 4) == 0);
      if (mask & 2) CHECK(std::memcmp(dist1.data(), dist.data(), (size_t)n * 4) == 0);
      if (mask & 4) CHECK(std::memcmp(pos1.data(), pos.data(), (size_t)n * 12) == 0);
      if (mask & 8) CHECK(std::memcmp(uv1.data(), uv.data(), (size_t)n * 8) == 0);
    }
  }
}

static void run_plans() {
  using namespace wgt;
  float x = 0.0f;
  uint32_t id = 0;
  const wgt_nearest_buffers none{}, one{&id, nullptr, nullptr, nullptr}, uvs{nullptr, nullptr, nullptr, &x};
  // the order: points, the struct, its fields, the count
  CHECK(std::string(check_nearest_args(nullptr, nullptr, 1ull << 40)) == "null points");
  CHECK(std::string(check_nearest_args(&x, nullptr, 1ull << 40)) == "null output buffers");
  CHECK(std::string(check_nearest_args(&x, &none, 1ull << 40)) == "no nearest field asked for");
  CHECK(std::string(check_nearest_args(&x, &one, 1ull << 40)) == "too many points");
  CHECK(check_nearest_args(&x, &one, kNearestMaxPoints) == nullptr);
  CHECK(check_nearest_args(&x, &uvs, 0) == nullptr);
  for (uint32_t n : {1u, 255u, 256u, 257u, 0x7fffffffu, 0xffffffffu})
    for (int mask = 1; mask < 16; ++mask)
      for (int radius = 0; radius < 2; ++radius) {
        const wgt_nearest_buffers b{mask & 1 ? &id : nullptr, mask & 2 ? &x : nullptr, mask & 4 ? &x : nullptr,
                                    mask & 8 ? &x : nullptr};
        const NearestStage s = plan_nearest_stage(b, radius != 0, n);
        const size_t N = n;
        CHECK(s.points == N * 12 && s.limits == (radius ? N * 4 : 0));
        CHECK(s.prim == (mask & 1 ? N * 4 : 0) && s.dist == (mask & 2 ? N * 4 : 0));
        CHECK(s.uv_at == (mask & 4 ? 3 * N : 0));
        CHECK(s.vec == ((mask & 4 ? 3 * N : 0) + (mask & 8 ? 2 * N : 0)) * 4);
      }
}

int main() {
  std::mt19937 g(12345);
  for (int mk = 0; mk < 5; ++mk)
    for (int pk = 0; pk < 10; ++pk) run_spec(g, mk, pk, 1 + (uint32_t)(g() % 97), 1 + (uint32_t)(g() % 61));
  run_spec(g, 0, 0, 0, 33);    // no triangles: misses
  run_spec(g, 0, 0, 500, 257);
  run_plans();
  if (g_fail) {
    std::fprintf(stderr, "nearest_fuzz: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("nearest_fuzz: ok\n");
  return 0;
}
