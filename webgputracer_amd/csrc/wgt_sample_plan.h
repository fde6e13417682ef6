// wgt_sample_plan.h — what the sample-map planner's planning (host/launch_plan.cpp), its thin calls
// (wgt_runtime.cpp) and its kernels (wgt_sample_plan.hip) share: the plan of one call, the budget
// rule over the histogram (host and device run the same function) and the launcher.  A header of
// its own, as wgt_temporal.h: the other kernels' translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/wgt_api.h"

namespace wgt {

constexpr uint32_t kSampleSideMax = 255;       // a side is one uint8_t
constexpr uint32_t kSampleBins = 256;          // one histogram bin per side
constexpr uint32_t kSamplePlanMaxHistory = 64; // min_history's range, the variance filter's
constexpr uint32_t kSamplePlanMaxDilate = 3;
constexpr float kSamplePlanMomentLimit = 0x1p100f;  // the accumulation's own limit on what it keeps

// One call, decided on the host (plan_sample_plan).
struct SamplePlan {
  uint32_t W, H;
  uint32_t side_min, side_max, dilate;
  float side_min_f, side_max_f;  // the same as floats (exact): the clamp compares in float
  float gain, lum_floor;
  float min_history;   // (float)params.min_history: exact
  uint32_t budgeted;   // budget_spp > 0
  uint64_t budget;     // B = floor(budget_spp * W * H), computed in double, saturated at 2^64 - 1
  // the workspace: W * H wanted sides, then the 256 histogram bins and the chosen cap (one word)
  size_t off_want, off_bins, bytes;
};

// sum over the sides v of bins[v] * min(v, c)^2: the map's total under the cap c.  Integers only:
// W * H <= 2^25 pixels of at most 255^2 samples stay below 2^41.
__host__ __device__ inline uint64_t sample_plan_total(const uint32_t* bins, uint32_t c) {
  uint64_t s = 0;
  for (uint32_t v = 0; v < kSampleBins; ++v) {
    const uint64_t m = v < c ? v : c;
    s += (uint64_t)bins[v] * (m * m);
  }
  return s;
}

// Launcher implemented in wgt_sample_plan.hip, on `stream`: the wanted side of every pixel, its
// dilation with the histogram of the dilated sides, the cap chosen from the histogram (one
// workgroup), and the cap applied.  Device pointers; total (may be null) receives the map's sum
// of k^2.  The workspace holds nothing between calls.
hipError_t launch_sample_plan(const SamplePlan& plan, const float* len, const float* moments, void* ws,
                              uint8_t* map, unsigned long long* total, hipStream_t stream);

}  // namespace wgt
