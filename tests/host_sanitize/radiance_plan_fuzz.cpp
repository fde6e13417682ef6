// radiance_plan_fuzz.cpp — what wgt_trace_radiance plans on the host, under AddressSanitizer + UBSan (CPU
// only; built and run by tests/test_radiance_sanitize.py): check_radiance_args in its order,
// plan_radiance_stage, and plan_radiance (the launch's uniform arguments and its form) over seeded random
// and boundary arguments.  Exits non-zero on a failed invariant; the sanitizers abort on the first finding.
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
  float ray = 0.0f;
  uint32_t word = 0;
  float rgb = 0.0f;
  // the order of the refusals: rays, out, an out without a field, samples; every combination of faults
  // reports the first one in that order
  for (int m = 0; m < 16; ++m) {
    const bool no_rays = m & 1, no_out = m & 2, empty = m & 4, many = m & 8;
    wgt_radiance_buffers out{};
    if (!empty) out.prim = &word;
    const char* want = no_rays ? "null rays" : no_out ? "null output buffers" : empty ? "no radiance field"
                       : many ? "too many samples" : nullptr;
    CHECK(says(check_radiance_args(no_rays ? nullptr : &ray, no_out ? nullptr : &out, many ? 65537u : 65536u), want));
  }
  // each single field is enough; the sample count's bound is exact, at any 64-bit value
  for (int f = 1; f < 8; ++f) {
    wgt_radiance_buffers out{(f & 1) ? &rgb : nullptr, (f & 2) ? &word : nullptr, (f & 4) ? &word : nullptr};
    for (uint64_t s : {0ull, 1ull, 3ull, 65536ull}) CHECK(check_radiance_args(&ray, &out, s) == nullptr);
    for (uint64_t s : {65537ull, 0xffffffffull, 0x100000000ull, ~0ull})
      CHECK(says(check_radiance_args(&ray, &out, s), "too many samples"));
    // the staging: bytes of exactly the planes asked for, without overflow at the largest n
    for (uint32_t n : {1u, 63u, 64u, 65u, 4097u, 0x7fffffffu, 0xffffffffu})
      for (int seeds = 0; seeds < 2; ++seeds) {
        const RadianceStage st = plan_radiance_stage(out, seeds != 0, n);
        CHECK(st.rays == (size_t)n * 24 && st.seeds == (seeds ? (size_t)n * 4 : 0));
        CHECK(st.rgb == ((f & 1) ? (size_t)n * 12 : 0) && st.prim == ((f & 2) ? (size_t)n * 4 : 0));
        CHECK(st.seed_out == ((f & 4) ? (size_t)n * 4 : 0));
      }
  }
  // the launch plan over random scenes' forms, counts and knobs
  const char* knobs[] = {"WGT_KERNEL", "WGT_CNODE", "WGT_PS_TO_TRAV", "WGT_PS_TO_SERVICE", "WGT_PS_SVC_FRAC",
                         "WGT_TRI_RATIO", "WGT_PQ_REFILL"};
  for (int it = 0; it < 20000; ++it) {
    for (const char* k : knobs) {
      if (g() % 3 == 0) setenv(k, std::to_string(g() % 5).c_str(), 1);
      else unsetenv(k);
    }
    DevScene sc{};
    sc.n_tris = g() % 3 ? 1u + g() % 100000u : 0u;
    sc.n_nodes = 1u + g() % 200000u;
    sc.stack = 2u + g() % 31u;
    sc.ps_waves = g() % 2 ? 6u : 5u;
    sc.ps_park = g() % 4 == 0;
    sc.ps_cap = sc.ps_park ? std::min<uint32_t>(sc.stack, kMinPsCap + g() % 24u) : sc.stack;
    const uint32_t n = g() % 4 ? 1u + g() % 100000u : 0xffffffffu - g() % 200000u;
    const uint32_t samples = g() % 65537u, seed0 = g(), resident = g() % 5 ? 1u + g() % 8192u : 0u;
    RadianceArgs a;
    const std::string bad = plan_radiance(sc, seed0, samples, n, resident, a);
    CHECK(a.n == n && a.samples == samples && a.seed0 == seed0 && a.fs == (float)samples);
    const bool pow2 = samples && !(samples & (samples - 1u));
    CHECK(pow2 ? a.inv_fs * a.fs == 1.0f : a.inv_fs == 0.0f);
    const bool flat_asked = env_u32("WGT_KERNEL", 2) != 2;
    if (sc.n_tris == 0 || flat_asked || resident == 0 || (uint64_t)n + 64ull * resident > 0xffffffffull) {
      CHECK(bad.empty() && !a.persistent);  // the flat form: never refused
      continue;
    }
    CHECK(a.persistent);
    if (sc.ps_park && sc.ps_cap < sc.stack) {  // an LDS stack shorter than the tree's: refused, not launched
      CHECK(bad.find("stack entries in LDS") != std::string::npos);
      continue;
    }
    CHECK(bad.empty());
    CHECK(a.compact <= 1u && a.to_trav >= 1u && a.to_service >= 1u && a.tri_ratio >= 1u && a.refill >= 1u);
    CHECK(env_u32("WGT_CNODE", 1) != 0 || a.compact == 0u);
  }
  if (g_fail) {
    std::fprintf(stderr, "radiance_plan_fuzz: %d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("radiance_plan_fuzz: ok\n");
  return 0;
}
