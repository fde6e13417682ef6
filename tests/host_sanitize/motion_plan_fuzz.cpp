// motion_plan_fuzz.cpp — the motion passes' host decisions under AddressSanitizer + UBSan (CPU only;
// built and run by tests/test_motion_sanitize.py): the argument checks of wgt_motion_reproject and of
// wgt_temporal_accumulate_motion in their order (launch_plan.h check_motion_reproject_args,
// check_temporal_motion_args) over seeded random and boundary arguments, and the motion form's
// agreement with check_temporal_args wherever the motion buffers are not what is refused.  Exits
// non-zero on a failed invariant; the sanitizers abort on the first finding.
#include <cstdio>
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

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

// Pointers are never dereferenced by the checks: any non-null value stands for a buffer.
static char* const kBase = (char*)(uintptr_t)0x100000000ull;

static wgt_camera_param reference_camera() {
  return wgt_camera_param{{278.0f, 278.0f, -800.0f}, 0.0f, {278.0f, 278.0f, 0.0f}, 0.0f, 1.5f, 40.0f, 1u, 0u};
}

static wgt_hit_buffers random_guides(std::mt19937& g) {
  wgt_hit_buffers b{};
  b.prim = g() % 10 ? (uint32_t*)kBase : nullptr;
  b.pos = g() % 10 ? (float*)kBase : nullptr;
  b.norm = g() % 10 ? (float*)kBase : nullptr;
  b.flags = g() % 10 ? (uint8_t*)kBase : nullptr;
  b.dist = g() % 2 ? (float*)kBase : nullptr;  // ignored
  b.col = g() % 2 ? (float*)kBase : nullptr;   // ignored
  return b;
}

static void fuzz_reproject() {
  std::mt19937 g(11);
  const uint32_t counts[] = {0, 1, 2, 255, 256, 257, 1u << 20, (1u << 25) - 1, 1u << 25, (1u << 25) + 1, 1u << 31, 0xffffffffu};
  for (int round = 0; round < 20000; ++round) {
    const uint32_t n = g() % 3 ? counts[g() % (sizeof counts / sizeof *counts)] : g();
    const bool snap = g() % 8 != 0;
    const wgt_hit_buffers gb = random_guides(g);
    wgt_motion_buffers mb{g() % 10 ? (float*)kBase : nullptr, g() % 10 ? (float*)kBase : nullptr};
    const wgt_hit_buffers* guides = g() % 12 ? &gb : nullptr;
    const wgt_motion_buffers* out = g() % 12 ? &mb : nullptr;
    const std::string bad = wgt::check_motion_reproject_args(snap, n, guides, out);
    const char* want = !snap ? "snapshot"
                       : !guides ? "null guides"
                       : !gb.prim ? "guides.prim"
                       : !gb.pos ? "guides.pos"
                       : !gb.norm ? "guides.norm"
                       : !gb.flags ? "guides.flags"
                       : !out ? "null out"
                       : !mb.pos_prev ? "out.pos_prev"
                       : !mb.norm_prev ? "out.norm_prev"
                       : (n < 1 || n > (1u << 25)) ? "is not in 1.."
                                                   : nullptr;
    if (!want) CHECK(bad.empty());
    else CHECK(!bad.empty() && has(bad, want));
  }
}

static void fuzz_accumulate() {
  std::mt19937 g(13);
  const uint32_t dims[] = {0, 1, 5, 64, 67, 1920, 8192, 32768, 32769};
  for (int round = 0; round < 20000; ++round) {
    const uint32_t W = dims[g() % (sizeof dims / sizeof *dims)], H = dims[g() % (sizeof dims / sizeof *dims)];
    wgt_temporal_params p = wgt::temporal_defaults();
    if (g() % 4 == 0) p.max_history = g() % 2 ? 0u : 65537u;
    const wgt_camera_param cams[2] = {reference_camera(), reference_camera()};
    const wgt_hit_buffers gb = random_guides(g), gp = random_guides(g);
    wgt_temporal_state prev{(float*)(kBase + (2ull << 36)), (float*)(kBase + (4ull << 36)), (float*)(kBase + (6ull << 36))};
    wgt_temporal_state out{(float*)(kBase + (8ull << 36)), (float*)(kBase + (10ull << 36)), (float*)(kBase + (12ull << 36))};
    if (g() % 10 == 0) out.len = nullptr;
    if (g() % 10 == 0) prev.rgba32f = nullptr;
    if (g() % 4 == 0) out.moments = nullptr;
    if (g() % 4 == 0) prev.moments = nullptr;
    wgt_motion_buffers mb{g() % 6 ? (float*)kBase : nullptr, g() % 6 ? (float*)kBase : nullptr};
    const wgt_motion_buffers* motion = g() % 6 ? &mb : nullptr;
    const void* in = g() % 12 ? kBase : nullptr;
    const wgt_hit_buffers* guides = g() % 12 ? &gb : nullptr;
    const unsigned triple = g() % 3 == 0 ? 0u : g() % 3 ? 7u : g() % 8;
    const wgt_temporal_state* pprev = triple & 1 ? &prev : nullptr;
    const wgt_hit_buffers* pgp = triple & 2 ? &gp : nullptr;
    const wgt_camera_param* cam_prev = triple & 4 ? &cams[1] : nullptr;
    const std::string plain = wgt::check_temporal_args(&p, W, H, &cams[0], cam_prev, in, guides, pprev, pgp, &out);
    const std::string bad = wgt::check_temporal_motion_args(&p, W, H, &cams[0], cam_prev, in, guides, motion, pprev, pgp, &out);
    // everything up to and including the first-frame triple is the plain form's refusal, word for word
    const bool before = !in || !guides || !out.len || !gb.prim || !gb.pos || !gb.norm || !gb.flags || (triple != 0 && triple != 7u);
    if (before || triple == 0) {
      CHECK(bad == plain);  // on the first frame motion is not looked at, null or not
      continue;
    }
    const char* want = !motion ? "null motion" : !mb.pos_prev ? "motion.pos_prev" : !mb.norm_prev ? "motion.norm_prev" : nullptr;
    if (want) CHECK(has(bad, want));
    else CHECK(bad == plain);
  }
}

int main() {
  fuzz_reproject();
  fuzz_accumulate();
  if (g_fail) {
    std::fprintf(stderr, "motion_plan_fuzz: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("motion_plan_fuzz: ok\n");
  return 0;
}
