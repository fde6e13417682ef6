// overlap_self_plan_fuzz.cpp — what wgt_overlap_self decides and computes on the host, under AddressSanitizer +
// UBSan (CPU only; built and run by tests/test_overlap_self_sanitize.py): plan_overlap_self (the checks in their
// order, one lane per resident triangle, the form, the list length, the LDS bytes and its refusal) and
// stage_overlap_self over boundary and seeded random arguments, and the brute force overlap_self_spec over
// random, degenerate, NaN and out-of-range meshes, with and without labels (any 32-bit value: they are never
// addresses), with every subset of the fields, into buffers of exactly the asked-for size.  Exits non-zero on a
// failed invariant; the sanitizers abort on the first finding.
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

static bool says(const std::string& got, const char* want) {
  return want ? got.find(want) != std::string::npos : got.empty();
}

static wgt_overlap_buffers fields(int f, uint8_t* hit, uint32_t* count, uint32_t* prim) {
  return wgt_overlap_buffers{(f & 1) ? hit : nullptr, (f & 2) ? count : nullptr, (f & 4) ? prim : nullptr};
}

// The refusal the checks' order gives these arguments, null when fine.
static const char* refusal(bool no_out, int f, uint64_t k) {
  return no_out ? "null output buffers" : f == 0 ? "no overlap field asked for" : k > 32 ? "k out of range"
         : (k == 0 && (f & 4)) ? "prim asked for with k == 0" : (k > 0 && !(f & 4)) ? "k > 0 without prim" : nullptr;
}

static void plans(std::mt19937& g) {
  uint8_t byte = 0;
  uint32_t word = 0;
  const uint32_t ns[] = {0u, 1u, 63u, 64u, 65u};
  const uint64_t ks[] = {0ull, 1ull, 32ull, 33ull};
  // every combination of the triangle count, k, the fields, an index buffer or none and a null struct, at the
  // shallowest and the deepest stack: the first fault in the checks' order is reported, else the lanes, the
  // form, the list length and the LDS bytes
  for (uint32_t stack : {1u, (uint32_t)kStackMax + 1u})
    for (uint32_t n : ns)
      for (uint64_t k : ks)
        for (int f = 0; f < 8; ++f)
          for (int m = 0; m < 4; ++m) {
            const bool no_index = m & 1, no_out = m & 2;
            DevScene sc{};
            sc.stack = stack;
            sc.n_tris = n;
            const wgt_overlap_buffers out = fields(f, &byte, &word, &word);
            const char* want = refusal(no_out, f, k);
            const char* said = check_overlap_self_args(no_out ? nullptr : &out, k);
            CHECK(says(said ? said : "", want));
            OverlapSelfPlan p;
            const std::string bad = plan_overlap_self(sc, no_out ? nullptr : &out, k, p);
            CHECK(says(bad, want) && p.n == n);
            if (want) {
              CHECK(p.lds == 0u && p.k == 0u && p.any == 0u);
              continue;
            }
            CHECK(p.k == (uint32_t)k && p.any == (f == 1 ? 1u : 0u));
            CHECK(p.lds == 4u * 64u * (stack + (uint32_t)k) && p.lds == overlap_lds_bytes(stack, p.k));
            CHECK(p.lds <= kOverlapLdsPerWorkgroup);
            CHECK(!p.any || p.k == 0u);  // the any form has no list
            // the staging: the labels up when there are any, exactly the asked-for fields down, nothing else
            const StageLayout lay = stage_overlap_self(no_index ? nullptr : &word, out, n, p.k);
            CHECK(lay.n == kOssParts);
            CHECK(lay.part[kOssIndex].bytes == (no_index ? 0 : (size_t)n * 12) && lay.part[kOssIndex].dst == nullptr);
            CHECK(lay.part[kOssIndex].src == (n && !no_index ? (const void*)&word : nullptr));
            CHECK(lay.part[kOssHit].bytes == ((f & 1) ? (size_t)n : 0));
            CHECK(lay.part[kOssCount].bytes == ((f & 2) ? (size_t)n * 4 : 0));
            CHECK(lay.part[kOssPrim].bytes == ((f & 4) ? (size_t)n * k * 4 : 0));
            for (int part = kOssHit; part < kOssParts; ++part) {
              CHECK(lay.part[part].src == nullptr);
              CHECK((lay.part[part].dst != nullptr) == (lay.part[part].bytes != 0));
              CHECK(lay.off[part] >= lay.off[part - 1] + lay.part[part - 1].bytes);
            }
            CHECK(lay.bytes() >= lay.off[kOssPrim] + lay.part[kOssPrim].bytes);
            // without labels the launch gets a null index pointer: part 0 has no bytes
            char base = 0;
            CHECK((lay.at(&base, kOssIndex) == nullptr) == (no_index || n == 0));
          }
  // seeded random arguments: any k at all, stacks no builder makes (refused, not launched)
  for (int it = 0; it < 20000; ++it) {
    DevScene sc{};
    sc.n_tris = g() % 4 ? 1u + g() % 100000u : 0xffffffffu - g() % 200000u;
    sc.stack = g() % 8 ? 1u + g() % 32u : 1u + g() % 4096u;
    const int f = (int)(g() % 8u);
    const wgt_overlap_buffers out = fields(f, &byte, &word, &word);
    const uint64_t k = g() % 16 ? g() % 34u : ((uint64_t)g() << 32 | g());
    OverlapSelfPlan p;
    const std::string bad = plan_overlap_self(sc, &out, k, p);
    CHECK(p.n == sc.n_tris);
    if (const char* want = refusal(false, f, k)) {
      CHECK(says(bad, want) && p.lds == 0u);
      continue;
    }
    const unsigned long long lds = 4ull * 64ull * ((unsigned long long)sc.stack + k);
    if (lds > 65536ull) {
      CHECK(bad.find("bytes of LDS") != std::string::npos && p.lds == 0u);
      continue;
    }
    CHECK(bad.empty() && p.lds == lds && p.k == k && p.any == (f == 1 ? 1u : 0u));
    // the largest staging does not overflow
    const StageLayout lay = stage_overlap_self(&word, out, sc.n_tris, p.k);
    CHECK(lay.bytes() >= (size_t)sc.n_tris * 12 + ((f & 4) ? (size_t)sc.n_tris * k * 4 : 0));
  }
  // every scene a builder makes fits at every k
  for (uint32_t stack = 1; stack <= (uint32_t)kStackMax + 1; ++stack)
    for (uint32_t k = 1; k <= 32; ++k) {
      DevScene sc{};
      sc.stack = stack;
      sc.n_tris = 1;
      const wgt_overlap_buffers all = fields(7, &byte, &word, &word);
      OverlapSelfPlan p;
      CHECK(plan_overlap_self(sc, &all, k, p).empty());
    }
}

static float pick(std::mt19937& g, int kind) {
  std::uniform_real_distribution<float> u(-1.0f, 1.0f);
  const float inf = std::numeric_limits<float>::infinity();
  switch (kind) {
    case 0: return 4.0f * u(g);
    case 1: return 0x1p40f * u(g);   // the scene's coordinate limit
    case 2: return 0x1p-100f * u(g);
    case 3: return 3.0e38f * u(g);   // beyond every limit: products overflow
    case 4: return std::nanf("");
    case 5: return (g() & 1) ? inf : -inf;
    case 6: return 0x1p41f * ((g() & 1) ? 1.0f : -1.0f);  // just out of range
    default: return (float)((int)(g() % 5u) - 2);  // small integers: touching and coplanar pairs, exact zeros
  }
}

static void spec(std::mt19937& g) {
  for (int it = 0; it < 1500; ++it) {
    const uint32_t ns[] = {1u, 2u, 63u, 64u, 65u};
    const uint32_t n = it % 50 == 0 ? ns[g() % 5u] : 1u + g() % 40u;
    const int tkind = (int)(g() % 8u);
    std::vector<wgt_triangle> T(n);
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
    // labels: a small range (many neighbours), or any 32-bit value
    std::vector<uint32_t> L(3 * (size_t)n);
    const bool wide = g() % 3u == 0;
    for (auto& l : L) l = wide ? (uint32_t)g() : (uint32_t)(g() % (2u * n + 1u));
    for (int indexed = 0; indexed < 2; ++indexed) {
      const uint32_t* idx = indexed ? L.data() : nullptr;
      std::vector<uint32_t> rc32;
      for (uint32_t k : {1u, 32u}) {
        // the reference answer: every field
        std::vector<uint8_t> rh(n);
        std::vector<uint32_t> rc(n), rp((size_t)k * n);
        overlap_self_spec(T.data(), n, 5u, idx, k, wgt_overlap_buffers{rh.data(), rc.data(), rp.data()});
        unsigned long long total = 0;
        for (uint32_t s = 0; s < n; ++s) {
          CHECK(rc[s] < n && rh[s] == (rc[s] > 0 ? 1 : 0));
          total += rc[s];
          for (uint32_t j = 0; j < k; ++j) {
            const uint32_t id = rp[(size_t)j * n + s];
            CHECK((id != 0xffffffffu) == (j < rc[s]));
            if (j < rc[s]) CHECK(id >= 5u && id < 5u + n && id != 5u + s);
            if (j < rc[s] && j) CHECK(rp[(size_t)(j - 1) * n + s] < id);
            if (j < rc[s] && indexed)  // a reported triangle shares no label
              for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) CHECK(L[3 * (size_t)s + a] != L[3 * (size_t)(id - 5u) + b]);
            // symmetry, wherever the partner's list is complete: s is in it
            if (j < rc[s] && rc[id - 5u] <= k) {
              bool back = false;
              for (uint32_t e = 0; e < rc[id - 5u]; ++e) back = back || rp[(size_t)e * n + (id - 5u)] == 5u + s;
              CHECK(back);
            }
          }
        }
        CHECK(total % 2ull == 0ull);  // every pair is counted from both sides
        if (k == 1u) rc32 = rc;
        if (k == 32u) CHECK(rc == rc32);  // the count does not depend on k
        // every subset of the fields, each buffer of exactly its size: the same bits, nothing else written
        for (int f = 1; f < 8; ++f) {
          std::vector<uint8_t> h(n);
          std::vector<uint32_t> c(n), p((size_t)k * n);
          overlap_self_spec(T.data(), n, 5u, idx, (f & 4) ? k : 0u, fields(f, h.data(), c.data(), p.data()));
          if (f & 1) CHECK(h == rh);
          if (f & 2) CHECK(c == rc);
          if (f & 4) CHECK(p == rp);
        }
      }
    }
    // labels that are all one value make everything adjacent: the empty answer
    std::vector<uint32_t> same(3 * (size_t)n, 0xfffffff0u), c(n, 7u), p((size_t)2 * n, 7u);
    overlap_self_spec(T.data(), n, 0u, same.data(), 2u, fields(6, nullptr, c.data(), p.data()));
    for (uint32_t i = 0; i < n; ++i) CHECK(c[i] == 0u && p[i] == 0xffffffffu && p[(size_t)n + i] == 0xffffffffu);
  }
  // no triangles: nothing is read, nothing is written
  overlap_self_spec(nullptr, 0u, 0u, nullptr, 2u, fields(7, nullptr, nullptr, nullptr));
}

int main() {
  std::mt19937 g(20261021u);
  plans(g);
  spec(g);
  if (g_fail) {
    std::fprintf(stderr, "overlap_self_plan_fuzz: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("overlap_self_plan_fuzz: ok\n");
  return 0;
}
