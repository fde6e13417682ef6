// sampled_plan_fuzz.cpp — the sampled renders' and the sample-map planner's host decisions under
// AddressSanitizer + UBSan (CPU only; built and run by tests/test_sampled_sanitize.py): the argument
// checks in their documented order (launch_plan.h check_sample_map after check_frame_args with spp
// taken as 1; check_sample_plan_args, check_sample_plan_workspace), the plan (the budget in double,
// the workspace layout), the budget cap from a histogram against a brute-force search, and the table
// of the sides' constants against make_frame, and wgt_sample_plan's staging layout (stage_sample_plan;
// stage_check.h).  Exits non-zero on a failed invariant; the sanitizers
// abort on the first finding.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>

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

// Pointers are never dereferenced by the checks: any non-null value stands for a buffer.
static char* const kBase = (char*)(uintptr_t)0x100000000ull;

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

static wgt_camera_param reference_camera(uint32_t spp) {
  return wgt_camera_param{{278.0f, 278.0f, -800.0f}, 0.0f, {278.0f, 278.0f, 0.0f}, 0.0f, 1.5f, 40.0f, spp, 0u};
}

// The sampled calls' own part of the order: the frame checks see spp 1 whatever the camera holds
// (an spp the plain call refuses is no refusal here), and the map is looked at last.
static void check_sampled_order() {
  const uint32_t spps[] = {0u, 1u, 7u, 65025u, 0xfffffeffu, 0xffffffffu};
  for (uint32_t spp : spps) {
    const wgt_camera_param cam = reference_camera(spp), c1 = wgt::sampled_camera(cam);
    CHECK(c1.spp == 1u && c1.seed == cam.seed && c1.fovy == cam.fovy && c1.origin[2] == cam.origin[2]);
    CHECK(wgt::check_frame_args(c1, 40, 24, 40, 24).empty());
    CHECK(has(wgt::check_frame_args(c1, 0, 24, 40, 24), "empty frame"));
    CHECK(has(wgt::check_frame_args(c1, 65536, 24, 40, 24), "65535"));
  }
  CHECK(!wgt::check_frame_args(reference_camera(0xffffffffu), 40, 24, 40, 24).empty());  // the plain call's refusal
  CHECK(wgt::check_sample_map(kBase) == nullptr);
  CHECK(has(wgt::check_sample_map(nullptr), "null sample map"));
}

// Every row is make_frame's triple for spp = k * k, bit for bit.
static void check_constants() {
  float tab[wgt::kSampleBins][4];
  wgt::sample_constants(tab);
  for (uint32_t k = 0; k < wgt::kSampleBins; ++k) {
    const wgt::DevFrame fr = wgt::make_frame(reference_camera(k * k), 64, 64);
    CHECK(fr.sqrt_spp == k);
    CHECK(bits(tab[k][0]) == bits(fr.recip_sqrt_spp));
    CHECK(bits(tab[k][1]) == bits(fr.fspp));
    CHECK(bits(tab[k][2]) == bits(fr.inv_fspp));
    CHECK(bits(tab[k][3]) == 0u);
    const bool pow2 = k != 0 && (k & (k - 1)) == 0;
    CHECK((tab[k][2] != 0.0f) == pow2);
    if (k) CHECK(tab[k][0] == 1.0f / (float)k);
  }
}

static float pick_float(std::mt19937& g, float good) {
  const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
  const float odd[] = {nan, inf, -inf, 0.0f, -0.0f, -1.0f, 1e-45f, 3e38f, good};
  return g() % 3 ? good : odd[g() % (sizeof odd / sizeof *odd)];
}

static void fuzz_plan_args() {
  std::mt19937 g(5);
  const uint32_t dims[] = {0, 1, 2, 3, 5, 17, 63, 64, 65, 67, 130, 255, 256, 1024, 1920, 4096, 8192, 32767, 32768, 32769,
                           65535, 0x80000000u, 0xffffffffu};
  const uint32_t small[] = {0, 1, 2, 3, 4, 8, 63, 64, 65, 254, 255, 256, 0x80000000u, 0xffffffffu};
  const size_t ND = sizeof dims / sizeof *dims, NS = sizeof small / sizeof *small;
  for (int round = 0; round < 40000; ++round) {
    const uint32_t W = g() % 4 ? dims[g() % 12 + 1] : dims[g() % ND], H = g() % 4 ? dims[g() % 12 + 1] : dims[g() % ND];
    wgt_sample_plan_params p = wgt::sample_plan_defaults();
    if (g() % 2) {
      p.side_min = g() % 3 ? g() % 9 : small[g() % NS];
      p.side_max = g() % 3 ? p.side_min + g() % 9 : small[g() % NS];
      p.gain = pick_float(g, 8.0f);
      p.lum_floor = pick_float(g, 0.01f);
      p.min_history = g() % 3 ? 1 + g() % 64 : small[g() % NS];
      p.dilate = g() % 3 ? g() % 4 : small[g() % NS];
      p.budget_spp = g() % 2 ? pick_float(g, 4.0f) : (float)(g() % 1000) * 0.25f;
    }
    wgt_temporal_state st{g() % 2 ? (float*)kBase : nullptr, g() % 10 ? (float*)kBase : nullptr,
                          g() % 10 ? (float*)kBase : nullptr};
    const wgt_temporal_state* state = g() % 12 ? &st : nullptr;
    const void* map = g() % 10 ? kBase : nullptr;
    const wgt_sample_plan_params* params = g() % 6 ? &p : nullptr;
    const std::string bad = wgt::check_sample_plan_args(params, W, H, state, map);
    const bool size_ok = W && H && W <= 32768 && H <= 32768 && (uint64_t)W * H <= (1ull << 25);
    const char* want = !state ? "null state"
                       : !st.len ? "state.len"
                       : !st.moments ? "state.moments"
                       : !map ? "null map_out"
                       : !size_ok ? "image size"
                       : !params ? ""
                       : p.side_min > 255 ? "side_min"
                       : p.side_max < p.side_min || p.side_max > 255 ? "side_max"
                       : !(p.gain > 0.0f) || !std::isfinite(p.gain) ? "gain"
                       : !(p.lum_floor > 0.0f) || !std::isfinite(p.lum_floor) ? "lum_floor"
                       : p.min_history < 1 || p.min_history > 64 ? "min_history"
                       : p.dilate > 3 ? "dilate"
                       : !(p.budget_spp >= 0.0f) || !std::isfinite(p.budget_spp) ? "budget_spp"
                       : "";
    CHECK(*want ? has(bad, want) : bad.empty());
    const size_t need = wgt::sample_plan_workspace_bytes(W, H);
    CHECK((need == 0) == !size_ok);
    if (!bad.empty()) continue;
    const wgt::SamplePlan plan = wgt::plan_sample_plan(params ? *params : wgt::sample_plan_defaults(), W, H);
    const wgt_sample_plan_params& q = params ? *params : p;
    CHECK(plan.bytes == need && need % 256 == 0 && plan.off_want == 0 && plan.off_bins >= (size_t)W * H);
    CHECK(plan.off_bins % 256 == 0 && plan.off_bins + (wgt::kSampleBins + 1) * 4 <= plan.bytes);
    if (params) {
      CHECK(plan.side_min_f == (float)q.side_min && plan.side_max_f == (float)q.side_max);
      CHECK(plan.budgeted == (q.budget_spp > 0.0f ? 1u : 0u));
      const long double b = std::floor((long double)q.budget_spp * W * H);
      CHECK(b >= 18446744073709551615.0L ? plan.budget == ~(uint64_t)0 : (long double)plan.budget == b);
    }
    // the workspace's checks, in their order
    CHECK(has(wgt::check_sample_plan_workspace(nullptr, need, W, H), "null workspace"));
    CHECK(has(wgt::check_sample_plan_workspace(kBase + 128, need, W, H), "misaligned"));
    CHECK(has(wgt::check_sample_plan_workspace(kBase, need - 1, W, H), "workspace_bytes"));
    CHECK(wgt::check_sample_plan_workspace(kBase, need, W, H).empty());
  }
}

// The cap from a histogram against a search over every cap.
static void fuzz_cap() {
  std::mt19937 g(9);
  for (int round = 0; round < 20000; ++round) {
    uint32_t bins[wgt::kSampleBins] = {};
    wgt_sample_plan_params p = wgt::sample_plan_defaults();
    p.side_min = g() % 4 ? g() % 6 : g() % 256;
    p.side_max = p.side_min + g() % (256 - p.side_min);
    const uint32_t W = 1 + g() % 300, H = 1 + g() % 300;
    for (uint32_t i = 0; i < W * H; ++i) {
      const uint32_t v = p.side_min + (g() % 3 ? g() % (p.side_max - p.side_min + 1) % 7 : g() % (p.side_max - p.side_min + 1));
      ++bins[v > p.side_max ? p.side_max : v];
      if (round % 8 && i > 2000) {  // the rest at one side
        bins[p.side_min] += W * H - i - 1;
        break;
      }
    }
    const float budgets[] = {0.0f, 0.25f, 1.0f, 3.99f, 4.0f, 17.5f, 1000.0f, 65025.0f, 1e9f, 3e38f};
    p.budget_spp = g() % 3 ? budgets[g() % 10] : (float)(g() % 70000) / 3.0f;
    const wgt::SamplePlan plan = wgt::plan_sample_plan(p, W, H);
    uint64_t total = ~(uint64_t)0;
    const uint32_t c = wgt::sample_plan_cap(plan, bins, total);
    CHECK(c >= p.side_min && c <= p.side_max);
    CHECK(total == wgt::sample_plan_total(bins, c));
    CHECK(wgt::sample_plan_total(bins, 255) >= total);
    if (!plan.budgeted) {
      CHECK(c == p.side_max);
      continue;
    }
    uint32_t best = p.side_min;
    for (uint32_t k = p.side_min; k <= p.side_max; ++k)
      if (wgt::sample_plan_total(bins, k) <= plan.budget) best = k;  // monotone in k: the last is the largest
    CHECK(c == best);
    if (wgt::sample_plan_total(bins, p.side_min) <= plan.budget) CHECK(total <= plan.budget);
    else CHECK(c == p.side_min);
  }
}

// wgt_sample_plan's staging layout (stage_sample_plan): seeded sizes and the largest the checks accept
// (as arithmetic: nothing is allocated), with and without total_out.
static void fuzz_stage() {
  std::mt19937 g(13);
  for (int round = 0; round < 300; ++round) {
    const uint32_t W = round ? 1 + g() % 70 : 32768, H = round ? 1 + g() % 70 : 1024;
    const uint64_t n = (uint64_t)W * H;
    CHECK(wgt::sample_plan_workspace_bytes(W, H) != 0);
    const wgt_temporal_state st{(float*)fake_ptr(0), (float*)fake_ptr(1), (float*)fake_ptr(2)};  // rgba32f: ignored
    for (int o = 0; o < 2; ++o) {
      void* const total = o ? fake_ptr(4) : nullptr;
      // the pass is always handed a total to write: its 8 bytes are there, fetched or not
      const StageWant want[] = {{n * 4, st.len, nullptr}, {n * 8, st.moments, nullptr}, {n, nullptr, fake_ptr(3)},
                                {8, nullptr, total}, {wgt::sample_plan_workspace_bytes(W, H), nullptr, nullptr}};
      static_assert(sizeof want / sizeof *want == wgt::kSpsParts, "one per part");
      g_fail += check_stage("stage_sample_plan", wgt::stage_sample_plan(W, H, st, fake_ptr(3), total), want, wgt::kSpsParts);
    }
  }
}

int main() {
  check_sampled_order();
  check_constants();
  fuzz_plan_args();
  fuzz_cap();
  fuzz_stage();
  if (g_fail) {
    std::fprintf(stderr, "sampled_plan_fuzz: %d failed checks\n", g_fail);
    return 1;
  }
  std::printf("sampled_plan_fuzz: ok\n");
  return 0;
}
