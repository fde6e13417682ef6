// denoise_variance_plan_fuzz.cpp — the variance-guided denoiser's host decisions under
// AddressSanitizer + UBSan (CPU only; built and run by tests/test_denoise_variance_sanitize.py): the
// argument checks in their order, the workspace size and layout, each pass's kz and min_history as a
// float (launch_plan.h check_denoise_variance_args, check_denoise_variance_workspace,
// denoise_variance_workspace_bytes, plan_denoise_variance) over seeded random and boundary arguments,
// and the synchronous form's staging layout (stage_denoise_variance; stage_check.h).
// Exits non-zero on a failed invariant; the sanitizers abort on the first finding.
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

static void check_plan(const wgt_denoise_variance_params& p, uint32_t W, uint32_t H) {
  const wgt::DenoiseVariancePlan d = wgt::plan_denoise_variance(p, W, H);
  const size_t n = (size_t)W * H, bytes = wgt::denoise_variance_workspace_bytes(W, H);
  CHECK(d.W == W && d.H == H && d.iterations == p.iterations && d.normal_power == p.normal_power);
  CHECK(d.demodulate == (p.flags & WGT_DENOISE_DEMODULATE));
  CHECK(std::memcmp(&d.sigma_lum, &p.sigma_lum, 4) == 0);
  CHECK(d.min_history == (float)p.min_history && d.min_history >= 1.0f && d.min_history <= 64.0f);
  CHECK(d.tiled_max_step <= wgt::kDenoiseMaxTiledStep);
  // the parts are 256-B aligned, in order, disjoint, large enough, and end at the size the caller is asked for
  CHECK(d.bytes == bytes && bytes % 256 == 0 && bytes >= 64 * n && bytes < 64 * n + 3 * 256);
  CHECK(d.off_rec % 256 == 0 && d.off_it0 % 256 == 0 && d.off_it1 % 256 == 0);
  CHECK(d.off_rec + 32 * n <= d.off_it0 && d.off_it0 + 16 * n <= d.off_it1 && d.off_it1 + 16 * n <= d.bytes);
  // kz of pass i: the restatement's two operations, then the power of four; kz[0] is 1 / sigma_pos^2
  const float kz0 = 1.0f / (p.sigma_pos * p.sigma_pos);
  float pow4 = 1.0f;
  for (uint32_t i = 0; i < wgt::kDenoiseMaxIterations; ++i, pow4 *= 0.25f) {
    const float want = kz0 * pow4;
    CHECK(std::memcmp(&want, &d.kz[i], 4) == 0);
  }
  // the plain filter's plan of the shared parameters: the same layout and constants
  const wgt::DenoisePlan q = wgt::plan_denoise(wgt_denoise_params{p.iterations, p.normal_power, p.sigma_pos, p.flags}, W, H);
  CHECK(q.bytes == d.bytes && q.off_it0 == d.off_it0 && q.off_it1 == d.off_it1 && q.tiled_max_step == d.tiled_max_step);
}

static void fuzz() {
  std::mt19937 g(7);
  const uint32_t dims[] = {0, 1, 2, 3, 5, 17, 63, 64, 65, 67, 130, 255, 256, 1024, 1920, 4096, 8192, 32767, 32768, 32769,
                           65536, 0x7fffffffu, 0xffffffffu};
  const float sigmas[] = {1.0f, 0.25f, 4.0f, 64.0f, 1e-30f, 1e30f, std::numeric_limits<float>::denorm_min(),
                          std::numeric_limits<float>::max(), 0.0f, -0.0f, -1.0f, std::numeric_limits<float>::infinity(),
                          -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
  const uint32_t hists[] = {0, 1, 2, 3, 4, 63, 64, 65, 1000, 0x80000000u, 0xffffffffu};
  // the workspace is the plain filter's: 0 exactly for the refused sizes, else non-decreasing in the pixel count
  std::vector<std::pair<uint64_t, size_t>> sized;
  for (uint32_t W : dims)
    for (uint32_t H : dims) {
      const size_t bytes = wgt::denoise_variance_workspace_bytes(W, H);
      CHECK((bytes != 0) == size_ok(W, H));
      CHECK(bytes == wgt::denoise_workspace_bytes(W, H));
      if (bytes) sized.push_back({(uint64_t)W * H, bytes});
    }
  std::sort(sized.begin(), sized.end());
  for (size_t i = 1; i < sized.size(); ++i) CHECK(sized[i].second >= sized[i - 1].second);
  {
    const wgt_denoise_variance_params d = wgt::denoise_variance_defaults();
    CHECK(d.iterations == 5 && d.normal_power == 7 && d.sigma_pos == 1.0f && d.flags == WGT_DENOISE_DEMODULATE &&
          d.sigma_lum == 4.0f && d.min_history == 4);
    CHECK(sizeof(wgt_denoise_variance_params) == 24);
  }
  for (int round = 0; round < 20000; ++round) {
    const uint32_t W = g() % 4 ? dims[g() % (sizeof dims / sizeof *dims)] : g() % 40000;
    const uint32_t H = g() % 4 ? dims[g() % (sizeof dims / sizeof *dims)] : g() % 40000;
    wgt_denoise_variance_params p = wgt::denoise_variance_defaults();
    if (g() % 3 == 0) p.iterations = g() % 3 ? g() % 11 : g();
    if (g() % 3 == 0) p.normal_power = g() % 3 ? g() % 13 : g();
    if (g() % 3 == 0) p.sigma_pos = sigmas[g() % (sizeof sigmas / sizeof *sigmas)];
    if (g() % 4 == 0) p.flags = g() % 2 ? g() % 4 : g();
    if (g() % 3 == 0) p.sigma_lum = sigmas[g() % (sizeof sigmas / sizeof *sigmas)];
    if (g() % 3 == 0) p.min_history = hists[g() % (sizeof hists / sizeof *hists)];
    const bool with_params = g() % 5 != 0;
    wgt_hit_buffers gb{};
    gb.prim = g() % 9 ? (uint32_t*)kPtr : nullptr;
    gb.pos = g() % 9 ? (float*)kPtr : nullptr;
    gb.norm = g() % 9 ? (float*)kPtr : nullptr;
    gb.col = g() % 9 ? (float*)kPtr : nullptr;
    gb.flags = g() % 9 ? (uint8_t*)kPtr : nullptr;
    gb.dist = g() % 2 ? (float*)kPtr : nullptr;  // ignored
    wgt_temporal_state st{};
    st.rgba32f = g() % 9 ? (float*)kPtr : nullptr;
    st.len = g() % 9 ? (float*)kPtr : nullptr;
    st.moments = g() % 9 ? (float*)kPtr : nullptr;
    const wgt_temporal_state* state = g() % 9 ? &st : nullptr;
    const wgt_hit_buffers* guides = g() % 9 ? &gb : nullptr;
    const void* o32 = g() % 3 ? kPtr : nullptr;
    const void* o8 = g() % 3 ? kPtr : nullptr;
    const std::string bad = wgt::check_denoise_variance_args(with_params ? &p : nullptr, W, H, state, guides, o32, o8);
    // the first failing check, in the documented order, words the refusal
    const char* bad_param = !with_params ? nullptr
                            : !(p.iterations >= 1 && p.iterations <= 8) ? "params.iterations"
                            : !(p.normal_power <= 10) ? "params.normal_power"
                            : !(p.sigma_pos > 0.0f && std::isfinite(p.sigma_pos)) ? "params.sigma_pos"
                            : (p.flags & ~1u) ? "params.flags"
                            : !(p.sigma_lum > 0.0f && std::isfinite(p.sigma_lum)) ? "params.sigma_lum"
                            : !(p.min_history >= 1 && p.min_history <= 64) ? "params.min_history"
                            : nullptr;
    const char* want = !state ? "null state"
                       : !guides ? "null guides"
                       : !st.rgba32f ? "state.rgba32f"
                       : !st.len ? "state.len"
                       : !st.moments ? "state.moments"
                       : !gb.prim ? "guides.prim"
                       : !gb.pos ? "guides.pos"
                       : !gb.norm ? "guides.norm"
                       : !gb.col ? "guides.col"
                       : !gb.flags ? "guides.flags"
                       : (!o32 && !o8) ? "outputs"
                       : !size_ok(W, H) ? "size"
                       : bad_param;
    if (!want) CHECK(bad.empty());
    else CHECK(!bad.empty() && has(bad, want));
    if (!want) {
      check_plan(with_params ? p : wgt::denoise_variance_defaults(), W, H);
      const size_t need = wgt::denoise_variance_workspace_bytes(W, H);
      CHECK(wgt::check_denoise_variance_workspace(kPtr, need, W, H).empty());
      CHECK(wgt::check_denoise_variance_workspace(kPtr, need + g() % 1000, W, H).empty());
      CHECK(has(wgt::check_denoise_variance_workspace(nullptr, need, W, H), "null workspace"));
      CHECK(has(wgt::check_denoise_variance_workspace((char*)kPtr + 1 + g() % 255, need, W, H), "misaligned"));
      CHECK(has(wgt::check_denoise_variance_workspace(kPtr, need - 1 - g() % need, W, H), "workspace_bytes"));
      CHECK(has(wgt::check_denoise_variance_workspace(nullptr, 0, W, H), "null workspace"));  // null before the size
    }
  }
}

// wgt_denoise_variance's staging layout (stage_denoise_variance): seeded sizes and the largest the checks
// accept (as arithmetic: nothing is allocated), with every combination of outputs that passes them.
static void fuzz_stage() {
  std::mt19937 g(12);
  for (int round = 0; round < 300; ++round) {
    const uint32_t W = round ? 1 + g() % 70 : 32768, H = round ? 1 + g() % 70 : 1024;
    CHECK(size_ok(W, H));
    const uint64_t n = (uint64_t)W * H;
    const wgt_temporal_state st{(float*)fake_ptr(0), (float*)fake_ptr(1), (float*)fake_ptr(2)};
    wgt_hit_buffers gb{};
    gb.prim = (uint32_t*)fake_ptr(3); gb.pos = (float*)fake_ptr(4); gb.norm = (float*)fake_ptr(5);
    gb.col = (float*)fake_ptr(6); gb.flags = (uint8_t*)fake_ptr(7);
    gb.dist = (float*)fake_ptr(8);  // ignored
    for (int o = 1; o < 8; ++o) {
      if (!(o & 3)) continue;  // a colour output is required
      void* const o32 = o & 1 ? fake_ptr(9) : nullptr;
      void* const o8 = o & 2 ? fake_ptr(10) : nullptr;
      void* const var = o & 4 ? fake_ptr(11) : nullptr;
      // the state's image is filtered in place: its part is the rgba32f output's too
      const StageWant want[] = {{n * 16, st.rgba32f, o32}, {n * 4, st.len, nullptr}, {n * 8, st.moments, nullptr},
                                {n * 4, gb.prim, nullptr}, {n * 12, gb.pos, nullptr}, {n * 12, gb.norm, nullptr},
                                {n * 12, gb.col, nullptr}, {n, gb.flags, nullptr}, {o8 ? n * 4 : 0, nullptr, o8},
                                {var ? n * 4 : 0, nullptr, var},
                                {wgt::denoise_variance_workspace_bytes(W, H), nullptr, nullptr}};
      static_assert(sizeof want / sizeof *want == wgt::kDvsParts, "one per part");
      g_fail += check_stage("stage_denoise_variance", wgt::stage_denoise_variance(W, H, st, gb, o32, o8, var), want,
                            wgt::kDvsParts);
    }
  }
}

int main() {
  fuzz();
  fuzz_stage();
  if (g_fail) {
    std::fprintf(stderr, "denoise_variance_plan_fuzz: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("denoise_variance_plan_fuzz: ok\n");
  return 0;
}
