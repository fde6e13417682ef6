// multihit_plan_fuzz.cpp — what wgt_trace_multi_hits plans on the host, under AddressSanitizer + UBSan (CPU
// only; built and run by tests/test_multihit_sanitize.py): check_multi_hit_args in its order,
// plan_multi_hit_stage, and plan_multi_hit (the mode, the list length, the LDS bytes and its refusal) over
// seeded random and boundary arguments.  Exits non-zero on a failed invariant; the sanitizers abort on the
// first finding.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

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

int main() {
  std::mt19937 g(20261021u);
  float ray = 0.0f, dist = 0.0f;
  uint32_t word = 0;
  // the order of the refusals: rays, out, an out without a field, flags, k; every combination of faults
  // reports the first one in that order
  for (int m = 0; m < 32; ++m) {
    const bool no_rays = m & 1, no_out = m & 2, empty = m & 4, flags = m & 8, bad_k = m & 16;
    wgt_multi_hit_buffers out{};
    if (!empty) out.prim = &word;
    const char* want = no_rays ? "null rays" : no_out ? "null output buffers" : empty ? "no multi-hit field"
                       : flags ? "unknown multi-hit flags" : bad_k ? "k out of range" : nullptr;
    CHECK(says(check_multi_hit_args(no_rays ? nullptr : &ray, no_out ? nullptr : &out, bad_k ? 33u : 32u,
                                    flags ? 2u : 1u), want));
  }
  for (int f = 1; f < 8; ++f) {
    wgt_multi_hit_buffers out{(f & 1) ? &word : nullptr, (f & 2) ? &word : nullptr, (f & 4) ? &dist : nullptr};
    const bool lists = (f & 6) != 0;
    // k's bounds are exact at any 64-bit value, and ignored with count alone; every flag bit but the one is unknown
    for (uint64_t k : {1ull, 2ull, 31ull, 32ull}) CHECK(check_multi_hit_args(&ray, &out, k, 0) == nullptr);
    for (uint64_t k : {0ull, 33ull, 0xffffffffull, 0x100000000ull, ~0ull})
      CHECK(says(check_multi_hit_args(&ray, &out, k, 1), lists ? "k out of range" : nullptr));
    for (int b = 1; b < 64; ++b)
      CHECK(says(check_multi_hit_args(&ray, &out, 1, 1ull << b), "unknown multi-hit flags"));
    // the staging: bytes of exactly the planes asked for, without overflow at the largest n and k
    for (uint32_t n : {1u, 63u, 64u, 65u, 4097u, 0x7fffffffu, 0xffffffffu})
      for (uint32_t k : {1u, 7u, 32u})
        for (int lim = 0; lim < 2; ++lim) {
          const MultiHitStage st = plan_multi_hit_stage(out, lim != 0, n, k);
          CHECK(st.rays == (size_t)n * 24 && st.limits == (lim ? (size_t)n * 4 : 0));
          CHECK(st.count == ((f & 1) ? (size_t)n * 4 : 0));
          CHECK(st.prim == ((f & 2) ? (size_t)n * k * 4 : 0) && st.dist == ((f & 4) ? (size_t)n * k * 4 : 0));
        }
  }
  // the launch plan over random scenes, fields, k and flags
  for (int it = 0; it < 20000; ++it) {
    DevScene sc{};
    sc.n_tris = g() % 3 ? 1u + g() % 100000u : 0u;
    // a scene's stack is within 1..kStackMax + 1; larger values (no builder makes them) must be refused, not launched
    sc.stack = g() % 8 ? 1u + g() % 32u : 1u + g() % 4096u;
    const int f = 1 + (int)(g() % 7u);
    wgt_multi_hit_buffers out{(f & 1) ? &word : nullptr, (f & 2) ? &word : nullptr, (f & 4) ? &dist : nullptr};
    const uint32_t n = g() % 4 ? 1u + g() % 100000u : 0xffffffffu - g() % 200000u;
    const uint32_t k = g() % 16 ? 1u + g() % 32u : g();
    const uint32_t flags = g() % 2;
    MultiHitPlan p;
    const std::string bad = plan_multi_hit(sc, out, n, k, flags, p);
    const uint32_t want_k = (f & 6) ? k : 0u;
    CHECK(p.n == n && p.k == want_k && p.tris_only == flags);
    CHECK(p.mode == ((f & 1) ? kMultiHitCount : kMultiHitCull));
    const unsigned long long lds = 4ull * 64ull * ((unsigned long long)sc.stack + 2ull * want_k);
    if ((f & 6) && (k < 1u || k > 32u)) {
      CHECK(bad.find("k out of range") != std::string::npos && p.lds == 0u);
      continue;
    }
    if (lds > 65536ull) {
      CHECK(bad.find("bytes of LDS") != std::string::npos && p.lds == 0u);
      continue;
    }
    CHECK(bad.empty() && p.lds == lds && p.lds == multi_hit_lds_bytes(sc.stack, p.k));
    // what the kernel indexes stays inside what the launch allocates: stack entries, then 2 k list words per lane
    CHECK(((size_t)sc.stack + 2 * (size_t)p.k) * kBlock * sizeof(int) == p.lds);
    CHECK(p.mode == kMultiHitCount || p.k >= 1u);
  }
  if (g_fail) {
    std::fprintf(stderr, "multihit_plan_fuzz: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("multihit_plan_fuzz: ok\n");
  return 0;
}
