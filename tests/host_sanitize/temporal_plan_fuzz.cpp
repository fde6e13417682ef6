// temporal_plan_fuzz.cpp — the temporal accumulation's host decisions under AddressSanitizer + UBSan
// (CPU only; built and run by tests/test_temporal_sanitize.py): the argument checks in their order
// and the cameras' projection constants (launch_plan.h check_temporal_args, temporal_camera,
// plan_temporal) over seeded random and boundary arguments: overlapping ranges, sizes at the limits,
// NaN parameters, degenerate cameras; and the synchronous forms' staging layout (stage_temporal;
// stage_check.h).  Exits non-zero on a failed invariant; the sanitizers abort on
// the first finding.
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
static bool size_ok(uint64_t W, uint64_t H) { return W >= 1 && H >= 1 && W <= 32768 && H <= 32768 && W * H <= (1ull << 25); }
static bool overlap(uint64_t a, uint64_t na, uint64_t b, uint64_t nb) { return a < b + nb && b < a + na; }

// Pointers are never dereferenced by the checks: any non-null value stands for a buffer.
static char* const kBase = (char*)(uintptr_t)0x100000000ull;
static const float kInf = std::numeric_limits<float>::infinity();
static const float kNaN = std::numeric_limits<float>::quiet_NaN();

static wgt_camera_param reference_camera() {
  return wgt_camera_param{{278.0f, 278.0f, -800.0f}, 0.0f, {278.0f, 278.0f, 0.0f}, 0.0f, 1.5f, 40.0f, 1u, 0u};
}

static bool finite3(const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
static bool nan3(const float* v) { return std::isnan(v[0]) || std::isnan(v[1]) || std::isnan(v[2]); }

// The constants of a camera that passed the checks: finite for a regular camera, NaN for a
// degenerate one, and the same bits as the operations written out here.
static void check_camera(const wgt_camera_param& cam, uint32_t W, uint32_t H, bool degenerate) {
  const wgt::TemporalCam t = wgt::temporal_camera(cam, W, H);
  const wgt::DevFrame fr = wgt::make_frame(cam, W, H);
  if (degenerate) {
    CHECK(std::isnan(t.k) && nan3(t.nrm));
    return;
  }
  CHECK(finite3(t.o) && finite3(t.c) && finite3(t.nrm) && finite3(t.iu) && finite3(t.iv) && std::isfinite(t.k));
  const float c[3] = {fr.pox - fr.ox, fr.poy - fr.oy, fr.poz - fr.oz};
  const float n[3] = {fr.duy * fr.dvz - fr.duz * fr.dvy, fr.duz * fr.dvx - fr.dux * fr.dvz, fr.dux * fr.dvy - fr.duy * fr.dvx};
  const float k = c[0] * n[0] + c[1] * n[1] + c[2] * n[2];
  const float uu = fr.dux * fr.dux + fr.duy * fr.duy + fr.duz * fr.duz;
  const float iu0 = fr.dux / uu;
  CHECK(std::memcmp(c, t.c, 12) == 0 && std::memcmp(n, t.nrm, 12) == 0 && std::memcmp(&k, &t.k, 4) == 0);
  CHECK(std::memcmp(&iu0, &t.iu[0], 4) == 0 && t.o[0] == fr.ox && t.o[1] == fr.oy && t.o[2] == fr.oz);
  // the centre pixel's point at unit ray parameter projects back onto the centre of pixel (0, 0)
  const float q[3] = {c[0], c[1], c[2]};
  const float z = q[0] * n[0] + q[1] * n[1] + q[2] * n[2];
  CHECK(k / z == 1.0f);
}

static void fuzz() {
  std::mt19937 g(7);
  const uint32_t dims[] = {0, 1, 2, 3, 5, 17, 63, 64, 65, 67, 130, 255, 256, 1024, 1920, 4096, 8192, 32767, 32768, 32769,
                           65536, 0x7fffffffu, 0xffffffffu};
  const uint32_t hist[] = {0, 1, 2, 4, 32, 65535, 65536, 65537, 0x7fffffffu, 0xffffffffu};
  const float nmin[] = {0.9f, -1.0f, 1.0f, 0.0f, -0.0f, 0.5f, -1.0000001f, 1.0000001f, 2.0f, kInf, -kInf, kNaN};
  const float ptol[] = {1.0f, 0.0f, -0.0f, 1e-30f, 1e30f, std::numeric_limits<float>::max(), -1e-30f, -1.0f, kInf, -kInf, kNaN};
  for (int round = 0; round < 20000; ++round) {
    const uint32_t W = g() % 4 ? dims[g() % (sizeof dims / sizeof *dims)] : g() % 40000;
    const uint32_t H = g() % 4 ? dims[g() % (sizeof dims / sizeof *dims)] : g() % 40000;
    wgt_temporal_params p = wgt::temporal_defaults();
    if (g() % 2) p.max_history = hist[g() % (sizeof hist / sizeof *hist)];
    if (g() % 2) p.normal_min = nmin[g() % (sizeof nmin / sizeof *nmin)];
    if (g() % 2) p.plane_tol = ptol[g() % (sizeof ptol / sizeof *ptol)];
    if (g() % 4 == 0) p.flags = g() % 2 ? g() % 4 : g();
    const bool with_params = g() % 5 != 0;
    // cameras: the reference's, moved, degenerate (no error), and refused ones (NaN, out of range)
    wgt_camera_param cams[2] = {reference_camera(), reference_camera()};
    bool cam_bad[2] = {false, false}, cam_degenerate[2] = {false, false};
    for (int k = 0; k < 2; ++k) {
      wgt_camera_param& c = cams[k];
      c.spp = g() % 3 ? g() : 0u;  // ignored, 0 and 2^32 - 1 too
      c.seed = g();
      switch (g() % 8) {
        case 0: c.origin[0] += 3.5f; c.target[0] += 3.5f; break;
        case 1: std::memcpy(c.target, c.origin, sizeof c.origin); cam_degenerate[k] = true; break;
        case 2: c.target[0] = c.origin[0]; c.target[1] = c.origin[1] + 10.0f; c.target[2] = c.origin[2]; cam_degenerate[k] = true; break;
        case 3: c.origin[g() % 3] = g() % 2 ? kNaN : kInf; cam_bad[k] = true; break;
        case 4: c.aspect = kNaN; cam_bad[k] = true; break;
        case 5: c.target[g() % 3] = 0x1p41f; cam_bad[k] = true; break;
        default: break;
      }
    }
    wgt_hit_buffers gb{}, gp{};
    for (wgt_hit_buffers* b : {&gb, &gp}) {
      b->prim = g() % 12 ? (uint32_t*)kBase : nullptr;
      b->pos = g() % 12 ? (float*)kBase : nullptr;
      b->norm = g() % 12 ? (float*)kBase : nullptr;
      b->flags = g() % 12 ? (uint8_t*)kBase : nullptr;
      b->dist = g() % 2 ? (float*)kBase : nullptr;  // ignored
      b->col = g() % 2 ? (float*)kBase : nullptr;   // ignored
    }
    // out and prev buffers at random small distances of each other, so that ranges overlap or just do not
    const uint64_t n = (uint64_t)W * H;
    const auto near = [&](char* to, uint64_t bytes) -> char* {
      switch (g() % 6) {
        case 0: return to;
        case 1: return to + bytes;  // adjacent: no overlap
        case 2: return to + (bytes ? bytes - 1 : 0);
        case 3: return to - bytes;
        case 4: return to - (bytes ? bytes - 1 : 0);
        default: return to + (1ull << 36);
      }
    };
    const uint64_t nb = size_ok(W, H) ? n : 16;
    wgt_temporal_state prev{(float*)(kBase + (2ull << 36)), (float*)(kBase + (4ull << 36)), (float*)(kBase + (6ull << 36))};
    wgt_temporal_state out{(float*)near((char*)prev.rgba32f, nb * 16), (float*)near((char*)prev.len, nb * 4),
                           (float*)near((char*)prev.moments, nb * 8)};
    if (g() % 10 == 0) out.rgba32f = nullptr;
    if (g() % 10 == 0) out.len = nullptr;
    if (g() % 4 == 0) out.moments = nullptr;
    if (g() % 10 == 0) prev.rgba32f = nullptr;
    if (g() % 10 == 0) prev.len = nullptr;
    if (g() % 4 == 0) prev.moments = nullptr;
    const void* in = g() % 12 ? (g() % 2 ? (const void*)out.rgba32f : (const void*)kBase) : nullptr;
    if (!in && g() % 2) in = kBase;
    const wgt_camera_param* cam = g() % 12 ? &cams[0] : nullptr;
    const wgt_hit_buffers* guides = g() % 12 ? &gb : nullptr;
    const wgt_temporal_state* pout = g() % 12 ? &out : nullptr;
    // the first-frame triple: mostly all set or all null, sometimes mixed
    const unsigned triple = g() % 3 == 0 ? 0u : g() % 3 ? 7u : g() % 8;
    const wgt_temporal_state* pprev = triple & 1 ? &prev : nullptr;
    const wgt_hit_buffers* pgp = triple & 2 ? &gp : nullptr;
    const wgt_camera_param* cam_prev = triple & 4 ? &cams[1] : nullptr;
    const std::string bad =
        wgt::check_temporal_args(with_params ? &p : nullptr, W, H, cam, cam_prev, in, guides, pprev, pgp, pout);
    // the first failing check, in the documented order, words the refusal
    const bool params_ok = !with_params || (p.max_history >= 1 && p.max_history <= 65536 && p.normal_min >= -1.0f &&
                                            p.normal_min <= 1.0f && p.plane_tol >= 0.0f && std::isfinite(p.plane_tol) &&
                                            (p.flags & ~1u) == 0);
    const bool first = triple == 0;
    const char* want = !in ? "input"
                       : !cam ? "null camera"
                       : !guides ? "null guides"
                       : !pout ? "null out"
                       : !out.rgba32f ? "out.rgba32f"
                       : !out.len ? "out.len"
                       : !gb.prim ? "guides.prim"
                       : !gb.pos ? "guides.pos"
                       : !gb.norm ? "guides.norm"
                       : !gb.flags ? "guides.flags"
                       : (!first && triple != 7u) ? "first-frame"
                       : (!first && !prev.rgba32f) ? "prev.rgba32f"
                       : (!first && !prev.len) ? "prev.len"
                       : (!first && !gp.prim) ? "guides_prev.prim"
                       : (!first && !gp.pos) ? "guides_prev.pos"
                       : (!first && !gp.norm) ? "guides_prev.norm"
                       : (!first && !gp.flags) ? "guides_prev.flags"
                       : (!first && !prev.moments != !out.moments) ? "moments"
                       : !size_ok(W, H) ? "size"
                       : !params_ok ? "params."
                       : cam_bad[0] ? "cam: "
                       : (!first && cam_bad[1]) ? "cam_prev: "
                       : (!first && overlap((uintptr_t)out.rgba32f, n * 16, (uintptr_t)prev.rgba32f, n * 16)) ? "overlap: out.rgba32f"
                       : (!first && overlap((uintptr_t)out.len, n * 4, (uintptr_t)prev.len, n * 4)) ? "overlap: out.len"
                       : (!first && out.moments && overlap((uintptr_t)out.moments, n * 8, (uintptr_t)prev.moments, n * 8))
                           ? "overlap: out.moments"
                           : nullptr;
    if (!want) CHECK(bad.empty());
    else CHECK(!bad.empty() && has(bad, want));
    if (!want) {
      const wgt_temporal_params used = with_params ? p : wgt::temporal_defaults();
      const wgt::TemporalPlan plan = wgt::plan_temporal(used, W, H, cams[0], cam_prev);
      CHECK(plan.W == W && plan.H == H && plan.first == (first ? 1u : 0u) && plan.match_prim == (used.flags & 1u));
      CHECK(plan.max_history == (float)used.max_history && (uint32_t)plan.max_history == used.max_history);
      CHECK(std::memcmp(&plan.normal_min, &used.normal_min, 4) == 0 && std::memcmp(&plan.plane_tol, &used.plane_tol, 4) == 0);
      check_camera(cams[0], W, H, cam_degenerate[0]);
      if (!first) check_camera(cams[1], W, H, cam_degenerate[1]);
      const wgt::TemporalCam again = wgt::temporal_camera(cams[0], W, H);
      CHECK(std::memcmp(&again, &plan.cam, sizeof again) == 0);
    }
  }
  // the widest ranges end where they should: W * H = 2^25 and buffers a byte apart
  {
    const uint32_t W = 8192, H = 4096;
    const wgt_camera_param cam = reference_camera();
    wgt_hit_buffers gb{(uint32_t*)kBase, nullptr, (float*)kBase, (float*)kBase, nullptr, (uint8_t*)kBase};
    const size_t n = (size_t)W * H;
    wgt_temporal_state prev{(float*)(kBase + (1ull << 40)), (float*)(kBase + (2ull << 40)), nullptr};
    wgt_temporal_state out{(float*)((char*)prev.rgba32f + n * 16), (float*)((char*)prev.len - n * 4), nullptr};
    CHECK(wgt::check_temporal_args(nullptr, W, H, &cam, &cam, kBase, &gb, &prev, &gb, &out).empty());
    out.rgba32f = (float*)((char*)prev.rgba32f + n * 16 - 1);
    CHECK(has(wgt::check_temporal_args(nullptr, W, H, &cam, &cam, kBase, &gb, &prev, &gb, &out), "overlap: out.rgba32f"));
    out.rgba32f = (float*)((char*)prev.rgba32f + n * 16);
    out.len = (float*)((char*)prev.len - n * 4 + 1);
    CHECK(has(wgt::check_temporal_args(nullptr, W, H, &cam, &cam, kBase, &gb, &prev, &gb, &out), "overlap: out.len"));
    // buffers at the very top and bottom of the address space: no wrap-around
    prev.rgba32f = (float*)(uintptr_t)16;
    out.rgba32f = (float*)(~(uintptr_t)0 - 15);
    out.len = (float*)(kBase + (3ull << 40));
    CHECK(wgt::check_temporal_args(nullptr, 1, 1, &cam, &cam, kBase, &gb, &prev, &gb, &out).empty());
  }
}

// The accumulation's staging layout (stage_temporal), both forms: seeded sizes and the largest the checks
// accept (as arithmetic: nothing is allocated); first frame or not, moments or not, rgba8_out or not.
static void fuzz_stage() {
  std::mt19937 g(14);
  for (int round = 0; round < 300; ++round) {
    const uint32_t W = round ? 1 + g() % 70 : 32768, H = round ? 1 + g() % 70 : 1024;
    CHECK(size_ok(W, H));
    const uint64_t n = (uint64_t)W * H;
    wgt_hit_buffers gb{}, gp{};
    gb.prim = (uint32_t*)fake_ptr(1); gb.pos = (float*)fake_ptr(2); gb.norm = (float*)fake_ptr(3); gb.flags = (uint8_t*)fake_ptr(4);
    gb.col = (float*)fake_ptr(20);  // ignored
    gp.prim = (uint32_t*)fake_ptr(8); gp.pos = (float*)fake_ptr(9); gp.norm = (float*)fake_ptr(10); gp.flags = (uint8_t*)fake_ptr(11);
    const wgt_motion_buffers mb{(float*)fake_ptr(12), (float*)fake_ptr(13)};
    for (int o = 0; o < 16; ++o) {
      const bool first = o & 1, mom = o & 2, motion_form = o & 8;
      void* const o8 = o & 4 ? fake_ptr(17) : nullptr;
      const wgt_temporal_state prev{(float*)fake_ptr(5), (float*)fake_ptr(6), mom ? (float*)fake_ptr(7) : nullptr};
      const wgt_temporal_state out{(float*)fake_ptr(14), (float*)fake_ptr(15), mom ? (float*)fake_ptr(16) : nullptr};
      // the motion form's first frame does not look at its motion buffers: the runtime passes none
      const bool mot = motion_form && !first;
      const uint64_t p = first ? 0 : n, m = mot ? n : 0;
      // the image is accumulated in place: its part is out->rgba32f's too
      const StageWant want[] = {{n * 16, fake_ptr(0), out.rgba32f}, {n * 4, gb.prim, nullptr}, {n * 12, gb.pos, nullptr},
                                {n * 12, gb.norm, nullptr}, {n, gb.flags, nullptr}, {p * 16, prev.rgba32f, nullptr},
                                {p * 4, prev.len, nullptr}, {mom ? p * 8 : 0, prev.moments, nullptr},
                                {p * 4, gp.prim, nullptr}, {p * 12, gp.pos, nullptr}, {p * 12, gp.norm, nullptr},
                                {p, gp.flags, nullptr}, {m * 12, mb.pos_prev, nullptr}, {m * 12, mb.norm_prev, nullptr},
                                {n * 4, nullptr, out.len}, {mom ? n * 8 : 0, nullptr, out.moments},
                                {o8 ? n * 4 : 0, nullptr, o8}};
      static_assert(sizeof want / sizeof *want == wgt::kTpsParts, "one per part");
      g_fail += check_stage("stage_temporal",
                            wgt::stage_temporal(W, H, fake_ptr(0), gb, mot ? &mb : nullptr, first ? nullptr : &prev,
                                                first ? nullptr : &gp, out, o8),
                            want, wgt::kTpsParts);
      // a first frame's layout is the same whatever stands in for the buffers it does not look at
      if (first)
        g_fail += check_stage("stage_temporal (first frame, stale buffers)",
                              wgt::stage_temporal(W, H, fake_ptr(0), gb, &mb, nullptr, &gp, out, o8), want, wgt::kTpsParts);
    }
  }
}

int main() {
  fuzz();
  fuzz_stage();
  if (g_fail) {
    std::fprintf(stderr, "temporal_plan_fuzz: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("temporal_plan_fuzz: ok\n");
  return 0;
}
