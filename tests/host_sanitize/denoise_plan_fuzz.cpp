// denoise_plan_fuzz.cpp — the denoiser's host decisions under AddressSanitizer + UBSan (CPU only;
// built and run by tests/test_denoise_sanitize.py): the argument checks in their order, the
// workspace size and layout, and each pass's kz (launch_plan.h check_denoise_args,
// check_denoise_workspace, denoise_workspace_bytes, plan_denoise) over seeded random and boundary
// arguments, and the synchronous form's staging layout (stage_denoise; stage_check.h).  Exits non-zero on a failed invariant; the sanitizers abort on the first finding.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "../../include/wgt_api.h"
#include "../../webgputracer_amd/csrc/host/launch_plan.h"
#include "stage_check.h"

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                          \
    }                                                                    \
  } while (0)

static bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }
static bool size_ok(uint64_t W, uint64_t H) { return W >= 1 && H >= 1 && W <= 32768 && H <= 32768 && W * H <= (1ull << 25); }

// Pointers are never dereferenced by the checks: any non-null value stands for a buffer.
static void* const kPtr = (void*)(uintptr_t)0x1000;

static void check_plan(const wgt_denoise_params& p, uint32_t W, uint32_t H) {
  const wgt::DenoisePlan d = wgt::plan_denoise(p, W, H);
  const size_t n = (size_t)W * H, bytes = wgt::denoise_workspace_bytes(W, H);
  CHECK(d.W == W && d.H == H && d.iterations == p.iterations && d.normal_power == p.normal_power);
  CHECK(d.demodulate == (p.flags & WGT_DENOISE_DEMODULATE));
  // the parts are 256-B aligned, in order, disjoint, large enough, and end at the size the caller is asked for
  CHECK(d.bytes == bytes && bytes % 256 == 0 && bytes >= 64 * n && bytes < 64 * n + 3 * 256);
  CHECK(d.off_rec % 256 == 0 && d.off_it0 % 256 == 0 && d.off_it1 % 256 == 0);
  CHECK(d.off_rec + 32 * n <= d.off_it0 && d.off_it0 + 16 * n <= d.off_it1 && d.off_it1 + 16 * n <= d.bytes);
  // kz of pass i: the restatement's two operations, then the power of four
  const float kz0 = 1.0f / (p.sigma_pos * p.sigma_pos);
  float pow4 = 1.0f;
  for (uint32_t i = 0; i < wgt::kDenoiseMaxIterations; ++i, pow4 *= 0.25f) {
    const float want = kz0 * pow4;
    CHECK(std::memcmp(&want, &d.kz[i], 4) == 0);
  }
}

static void fuzz() {
  std::mt19937 g(5);
  const uint32_t dims[] = {0, 1, 2, 3, 5, 17, 63, 64, 65, 67, 130, 255, 256, 1024, 1920, 4096, 8192, 32767, 32768, 32769,
                           65536, 0x7fffffffu, 0xffffffffu};
  const float sigmas[] = {1.0f, 0.25f, 16.0f, 1e-30f, 1e30f, std::numeric_limits<float>::denorm_min(),
                          std::numeric_limits<float>::max(), 0.0f, -0.0f, -1.0f, std::numeric_limits<float>::infinity(),
                          -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
  // 0 exactly for the refused sizes, else non-decreasing in the pixel count
  std::vector<std::pair<uint64_t, size_t>> sized;
  for (uint32_t W : dims)
    for (uint32_t H : dims) {
      const size_t bytes = wgt::denoise_workspace_bytes(W, H);
      CHECK((bytes != 0) == size_ok(W, H));
      if (bytes) sized.push_back({(uint64_t)W * H, bytes});
    }
  std::sort(sized.begin(), sized.end());
  for (size_t i = 1; i < sized.size(); ++i) CHECK(sized[i].second >= sized[i - 1].second);
  for (int round = 0; round < 20000; ++round) {
    const uint32_t W = g() % 4 ? dims[g() % (sizeof dims / sizeof *dims)] : g() % 40000;
    const uint32_t H = g() % 4 ? dims[g() % (sizeof dims / sizeof *dims)] : g() % 40000;
    wgt_denoise_params p = wgt::denoise_defaults();
    if (g() % 2) p.iterations = g() % 3 ? g() % 11 : g();
    if (g() % 2) p.normal_power = g() % 3 ? g() % 13 : g();
    if (g() % 2) p.sigma_pos = sigmas[g() % (sizeof sigmas / sizeof *sigmas)];
    if (g() % 4 == 0) p.flags = g() % 2 ? g() % 4 : g();
    const bool with_params = g() % 5 != 0;
    wgt_hit_buffers gb{};
    gb.prim = g() % 9 ? (uint32_t*)kPtr : nullptr;
    gb.pos = g() % 9 ? (float*)kPtr : nullptr;
    gb.norm = g() % 9 ? (float*)kPtr : nullptr;
    gb.col = g() % 9 ? (float*)kPtr : nullptr;
    gb.flags = g() % 9 ? (uint8_t*)kPtr : nullptr;
    gb.dist = g() % 2 ? (float*)kPtr : nullptr;  // ignored
    const void* in = g() % 9 ? kPtr : nullptr;
    const wgt_hit_buffers* guides = g() % 9 ? &gb : nullptr;
    const void* o32 = g() % 3 ? kPtr : nullptr;
    const void* o8 = g() % 3 ? kPtr : nullptr;
    const std::string bad = wgt::check_denoise_args(with_params ? &p : nullptr, W, H, in, guides, o32, o8);
    // the first failing check, in the documented order, words the refusal
    const bool params_ok = !with_params || (p.iterations >= 1 && p.iterations <= 8 && p.normal_power <= 10 &&
                                            p.sigma_pos > 0.0f && std::isfinite(p.sigma_pos) && (p.flags & ~1u) == 0);
    const char* want = !in ? "input"
                       : !guides ? "guides"
                       : !gb.prim ? "guides.prim"
                       : !gb.pos ? "guides.pos"
                       : !gb.norm ? "guides.norm"
                       : !gb.col ? "guides.col"
                       : !gb.flags ? "guides.flags"
                       : (!o32 && !o8) ? "outputs"
                       : !size_ok(W, H) ? "size"
                       : !params_ok ? "params."
                       : nullptr;
    if (!want) CHECK(bad.empty());
    else CHECK(!bad.empty() && has(bad, want));
    if (!want) {
      check_plan(with_params ? p : wgt::denoise_defaults(), W, H);
      const size_t need = wgt::denoise_workspace_bytes(W, H);
      CHECK(wgt::check_denoise_workspace(kPtr, need, W, H).empty());
      CHECK(wgt::check_denoise_workspace(kPtr, need + g() % 1000, W, H).empty());
      CHECK(has(wgt::check_denoise_workspace(nullptr, need, W, H), "null workspace"));
      CHECK(has(wgt::check_denoise_workspace((char*)kPtr + 1 + g() % 255, need, W, H), "misaligned"));
      CHECK(has(wgt::check_denoise_workspace(kPtr, need - 1 - g() % need, W, H), "workspace_bytes"));
      CHECK(has(wgt::check_denoise_workspace(nullptr, 0, W, H), "null workspace"));  // null before the size
    }
  }
}

// wgt_denoise's staging layout (stage_denoise): seeded sizes and the largest the checks accept (as
// arithmetic: nothing is allocated), with every combination of outputs that passes them.
static void fuzz_stage() {
  std::mt19937 g(11);
  for (int round = 0; round < 300; ++round) {
    const uint32_t W = round ? 1 + g() % 70 : 32768, H = round ? 1 + g() % 70 : 1024;
    CHECK(size_ok(W, H));
    const uint64_t n = (uint64_t)W * H;
    wgt_hit_buffers gb{};
    gb.prim = (uint32_t*)fake_ptr(1); gb.pos = (float*)fake_ptr(2); gb.norm = (float*)fake_ptr(3);
    gb.col = (float*)fake_ptr(4); gb.flags = (uint8_t*)fake_ptr(5);
    gb.dist = (float*)fake_ptr(6);  // ignored
    for (int o = 1; o < 4; ++o) {
      void* const o32 = o & 1 ? fake_ptr(7) : nullptr;
      void* const o8 = o & 2 ? fake_ptr(8) : nullptr;
      // the image is filtered in place: its part is the rgba32f output's too
      const StageWant want[] = {{n * 16, fake_ptr(0), o32}, {n * 4, gb.prim, nullptr}, {n * 12, gb.pos, nullptr},
                                {n * 12, gb.norm, nullptr}, {n * 12, gb.col, nullptr}, {n, gb.flags, nullptr},
                                {o8 ? n * 4 : 0, nullptr, o8}, {wgt::denoise_workspace_bytes(W, H), nullptr, nullptr}};
      static_assert(sizeof want / sizeof *want == wgt::kDnsParts, "one per part");
      g_fail += check_stage("stage_denoise", wgt::stage_denoise(W, H, fake_ptr(0), gb, o32, o8), want, wgt::kDnsParts);
    }
  }
}

int main() {
  fuzz();
  fuzz_stage();
  if (g_fail) {
    std::fprintf(stderr, "denoise_plan_fuzz: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("denoise_plan_fuzz: ok\n");
  return 0;
}
