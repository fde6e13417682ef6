// nearest_k_fuzz.cpp — what wgt_nearest_k_points decides and computes on the host, under AddressSanitizer +
// UBSan (CPU only; built and run by tests/test_nearest_k_sanitize.py): check_nearest_k_args in its order,
// plan_nearest_k_stage, plan_nearest_k (the mode, the list length and words, the LDS bytes and its refusal)
// over seeded random and boundary arguments, and the brute force nearest_k_points_spec over random,
// degenerate, NaN and huge inputs with every subset of the fields at k = 1 and 32, into buffers of exactly
// the asked-for size.  Exits non-zero on a failed invariant; the sanitizers abort on the first finding.
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

using namespace wgt;

static bool says(const char* got, const char* want) {
  return want ? got && std::strstr(got, want) != nullptr : got == nullptr;
}

static wgt_nearest_k_buffers fields(int f, uint32_t* count, uint32_t* prim, float* dist, float* pos, float* uv) {
  return wgt_nearest_k_buffers{(f & 1) ? count : nullptr, (f & 2) ? prim : nullptr, (f & 4) ? dist : nullptr,
                               (f & 8) ? pos : nullptr, (f & 16) ? uv : nullptr};
}

static void plans(std::mt19937& g) {
  float pt = 0.0f, fl = 0.0f;
  uint32_t word = 0;
  // the order of the refusals: points, out, an out without a field, n, k; every combination of faults
  // reports the first one in that order
  for (int m = 0; m < 32; ++m) {
    const bool no_points = m & 1, no_out = m & 2, empty = m & 4, many = m & 8, bad_k = m & 16;
    wgt_nearest_k_buffers out{};
    if (!empty) out.uv = &fl;
    const char* want = no_points ? "null points" : no_out ? "null output buffers" : empty ? "no nearest field"
                       : many ? "too many points" : bad_k ? "k out of range" : nullptr;
    CHECK(says(check_nearest_k_args(no_points ? nullptr : &pt, no_out ? nullptr : &out, many ? 1ull << 32 : 0xffffffffull,
                                    bad_k ? 33u : 32u), want));
  }
  for (int f = 1; f < 32; ++f) {
    const wgt_nearest_k_buffers out = fields(f, &word, &word, &fl, &fl, &fl);
    const bool lists = (f & 30) != 0;
    // k's bounds are exact at any 64-bit value, and ignored with count alone
    for (uint64_t k : {1ull, 2ull, 31ull, 32ull}) CHECK(check_nearest_k_args(&pt, &out, 1, k) == nullptr);
    for (uint64_t k : {0ull, 33ull, 0xffffffffull, 0x100000000ull, ~0ull})
      CHECK(says(check_nearest_k_args(&pt, &out, 1, k), lists ? "k out of range" : nullptr));
    // the staging: bytes of exactly the planes asked for, without overflow at the largest n and k
    for (uint32_t n : {1u, 63u, 64u, 65u, 4097u, 0x7fffffffu, 0xffffffffu})
      for (uint32_t k : {1u, 7u, 32u})
        for (int lim = 0; lim < 2; ++lim) {
          const NearestKStage st = plan_nearest_k_stage(out, lim != 0, n, k);
          const size_t planes = (size_t)n * k * 4;
          CHECK(st.points == (size_t)n * 12 && st.limits == (lim ? (size_t)n * 4 : 0));
          CHECK(st.count == ((f & 1) ? (size_t)n * 4 : 0));
          CHECK(st.prim == ((f & 2) ? planes : 0) && st.dist == ((f & 4) ? planes : 0));
          CHECK(st.vec == ((f & 8) ? 3 * planes : 0) + ((f & 16) ? 2 * planes : 0));
          CHECK(st.uv_at * 4 == ((f & 8) ? 3 * planes : 0));
        }
  }
  // the launch plan over random scenes, fields and k
  for (int it = 0; it < 20000; ++it) {
    DevScene sc{};
    sc.n_tris = g() % 3 ? 1u + g() % 100000u : 0u;
    // a scene's stack is within 1..kStackMax + 1; larger values (no builder makes them) must be refused, not launched
    sc.stack = g() % 8 ? 1u + g() % 32u : 1u + g() % 4096u;
    const int f = (int)(g() % 32u);
    const wgt_nearest_k_buffers out = fields(f, &word, &word, &fl, &fl, &fl);
    const uint32_t n = g() % 4 ? 1u + g() % 100000u : 0xffffffffu - g() % 200000u;
    const uint32_t k = g() % 16 ? 1u + g() % 32u : g();
    NearestKPlan p;
    const std::string bad = plan_nearest_k(sc, out, n, k, p);
    const bool lists = (f & 30) != 0;
    const uint32_t want_k = lists ? k : 0u, words = (f & 24) ? 3u : 2u;
    CHECK(p.n == n && p.k == want_k && p.words == words);
    CHECK(p.mode == ((f & 1) ? kNearestKCount : kNearestKCull));
    CHECK(p.sort == (want_k > 0 ? 1u : 0u));  // no WGT_NEAREST_K_SORT in this process
    if (f == 0) {
      CHECK(bad.find("no nearest field") != std::string::npos && p.lds == 0u);
      continue;
    }
    if (lists && (k < 1u || k > 32u)) {
      CHECK(bad.find("k out of range") != std::string::npos && p.lds == 0u);
      continue;
    }
    const unsigned long long lds = 4ull * 64ull * ((unsigned long long)sc.stack + (unsigned long long)words * want_k);
    if (lds > 65536ull) {
      CHECK(bad.find("bytes of LDS") != std::string::npos && p.lds == 0u);
      continue;
    }
    CHECK(bad.empty() && p.lds == lds && p.lds == nearest_k_lds_bytes(sc.stack, p.k, p.words));
    // sized for the call's k, not for 32; the cull form always has a list to read its k-th entry from
    CHECK(((size_t)sc.stack + (size_t)p.words * p.k) * kBlock * sizeof(int) == p.lds);
    CHECK(p.mode == kNearestKCount || p.k >= 1u);
  }
  // every scene a builder makes fits at every k
  for (uint32_t stack = 1; stack <= (uint32_t)kStackMax + 1; ++stack)
    for (uint32_t k = 1; k <= 32; ++k) {
      DevScene sc{};
      sc.stack = stack;
      NearestKPlan p;
      CHECK(plan_nearest_k(sc, fields(31, &word, &word, &fl, &fl, &fl), 1, k, p).empty());
    }
}

static float pick(std::mt19937& g, int kind) {
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  const float inf = std::numeric_limits<float>::infinity();
  switch (kind) {
    case 0: return 100.0f * u(g);
    case 1: return 0x1p40f * u(g);   // the scene's coordinate limit
    case 2: return 0x1p-100f * u(g);
    case 3: return 3.0e38f * u(g);   // squares overflow
    case 4: return std::nanf("");
    case 5: return (g() & 1) ? inf : -inf;
    default: return (float)((int)(g() % 5u) - 2);  // small integers: ties and exact zeros
  }
}

static void spec(std::mt19937& g) {
  const float inf = std::numeric_limits<float>::infinity();
  for (int it = 0; it < 600; ++it) {
    const uint32_t n_tris = it % 7 == 0 ? 0u : 1u + g() % 80u;
    const uint32_t n = 1u + g() % 9u;
    const int tkind = (int)(g() % 8u), pkind = (int)(g() % 8u);
    std::vector<wgt_triangle> T(n_tris);
    for (auto& t : T) {
      std::memset(&t, 0, sizeof t);
      const int shape = (int)(g() % 4u);  // ordinary, a point, collinear, a copy of the first
      for (int a = 0; a < 3; ++a) {
        t.v0[a] = pick(g, g() % 4u ? 0 : tkind);
        t.e1[a] = shape == 1 ? 0.0f : pick(g, g() % 4u ? 0 : tkind);
        t.e2[a] = shape == 1 ? 0.0f : shape == 2 ? 2.0f * t.e1[a] : pick(g, g() % 4u ? 0 : tkind);
      }
      if (shape == 3) t = T[0];
    }
    std::vector<float> P(3 * (size_t)n), M(n);
    for (auto& x : P) x = pick(g, g() % 3u ? 0 : pkind);
    for (auto& m : M) m = g() % 5u == 0 ? pick(g, (int)(g() % 7u)) : 150.0f * (float)(g() % 4u);
    const float* lim = g() % 3u ? M.data() : nullptr;
    for (uint32_t k : {1u, 32u}) {
      // the reference answer: every field
      std::vector<uint32_t> rc(n), rp((size_t)k * n);
      std::vector<float> rd((size_t)k * n), rpos(3 * (size_t)k * n), ruv(2 * (size_t)k * n);
      nearest_k_points_spec(T.data(), n_tris, 5u, P.data(), lim, n, k,
                            wgt_nearest_k_buffers{rc.data(), rp.data(), rd.data(), rpos.data(), ruv.data()});
      for (uint32_t i = 0; i < n; ++i) {
        const float m = lim ? lim[i] : inf;
        CHECK(rc[i] <= n_tris);
        for (uint32_t j = 0; j < k; ++j) {
          const bool have = j < rc[i];
          CHECK((rp[(size_t)j * n + i] != 0xffffffffu) == have);
          const float d = rd[(size_t)j * n + i];
          CHECK(have ? (d < m && d >= 0.0f) : d == inf);
          if (have) CHECK(rp[(size_t)j * n + i] >= 5u && rp[(size_t)j * n + i] < 5u + n_tris);
          if (have && j) CHECK(rd[(size_t)(j - 1) * n + i] <= d);
          if (!have)
            for (int a = 0; a < 3; ++a) CHECK(rpos[((size_t)3 * j + a) * n + i] == 0.0f);
        }
        const bool bad_point = !(std::fabs(P[i]) + std::fabs(P[n + i]) + std::fabs(P[2 * (size_t)n + i]) < inf);
        if (bad_point || !(m > 0.0f) || n_tris == 0) CHECK(rc[i] == 0u);
      }
      // every subset of the fields, each buffer of exactly its size: the same bits, nothing else written
      for (int f = 1; f < 32; ++f) {
        std::vector<uint32_t> c(n), p((size_t)k * n);
        std::vector<float> d((size_t)k * n), pos(3 * (size_t)k * n), uv(2 * (size_t)k * n);
        nearest_k_points_spec(T.data(), n_tris, 5u, P.data(), lim, n, k, fields(f, c.data(), p.data(), d.data(), pos.data(), uv.data()));
        if (f & 1) CHECK(c == rc);
        if (f & 2) CHECK(p == rp);
        if (f & 4) CHECK(std::memcmp(d.data(), rd.data(), d.size() * 4) == 0);
        if (f & 8) CHECK(std::memcmp(pos.data(), rpos.data(), pos.size() * 4) == 0);
        if (f & 16) CHECK(std::memcmp(uv.data(), ruv.data(), uv.size() * 4) == 0);
      }
    }
    // count alone ignores k, whatever it is: no list buffer exists to write
    std::vector<uint32_t> c(n), c1(n);
    nearest_k_points_spec(T.data(), n_tris, 0u, P.data(), lim, n, 0xffffffffu, fields(1, c.data(), nullptr, nullptr, nullptr, nullptr));
    nearest_k_points_spec(T.data(), n_tris, 0u, P.data(), lim, n, 0u, fields(1, c1.data(), nullptr, nullptr, nullptr, nullptr));
    CHECK(c == c1);
  }
}

int main() {
  std::mt19937 g(20261021u);
  plans(g);
  spec(g);
  if (g_fail) {
    std::fprintf(stderr, "nearest_k_fuzz: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("nearest_k_fuzz: ok\n");
  return 0;
}
