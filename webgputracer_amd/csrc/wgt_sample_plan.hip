// wgt_sample_plan.hip — planning a sample map from the accumulated state (wgt_sample_plan,
// wgt_sample_plan_async): each pixel's relative standard deviation of luminance, from the moments
// wgt_temporal_accumulate keeps, becomes the side of its sample grid for the next frame; the sides
// are dilated, and an optional budget caps them.  A translation unit of its own:
// it runs between frames, on the accumulation's outputs, and reads no scene.
//
// The arithmetic is the specification's, operation by operation (tests/sample_plan_restatement.py
// is the same in numpy, and the map and its total are equal bit for bit): binary32, no fused
// multiply-add (-ffp-contract=off), the compiler's correctly rounded division, sqrt_rn, denormals
// kept.  No float is reduced across pixels: the budget rule works on a 256-bin histogram of the
// dilated sides filled with integer atomics, so no result depends on the order of waves.
//
//   k_sp_want   : one lane per pixel, 12 B read and 1 B written: the wanted side.
//   k_sp_dilate : one lane per pixel, a 64 x 4 workgroup: the maximum of the wanted sides within
//                 `dilate` pixels (in-image taps only, every index checked against W x H), written
//                 to the map; the workgroup's sides are counted in LDS, then added to the global bins.
//   k_sp_cap    : one workgroup of 256 lanes: lane c computes the map's total under the cap c from the
//                 bins (sample_plan_total, the host's function), lane 0 takes the largest cap within
//                 the budget and writes it and its total.
//   k_sp_apply  : one lane per pixel: map = min(map, cap); the launch ends at once when the cap is side_max.
#include "wgt_sample_plan.h"

#include "wgt_math.h"

namespace wgt {

namespace {

constexpr int kSpX = 64, kSpY = 4;
constexpr int kSpFlat = 256;

__device__ __forceinline__ bool within(float v) { return __builtin_fabsf(v) <= kSamplePlanMomentLimit; }  // NaN and inf fail

// Steps 1-4 of the specification.  Nothing here makes a NaN that reaches the conversion: m1 and m2
// are finite, m1 * m1 is finite or +inf, so m2 - m1 * m1 is finite or -inf and var is in [0, 2^100];
// the divisor is positive and finite (lum_floor > 0), so rel is in [0, +inf]; gain is finite and
// > 0, so rel * gain is 0 * finite, finite * finite or inf * positive; and the clamp compares in
// float, so +inf becomes side_max before it is converted.
__device__ __forceinline__ uint32_t wanted_side(const SamplePlan& p, float len, float m1, float m2) {
  const bool measured = len >= p.min_history && within(m1) && within(m2) && len >= 1.0f;
  if (!measured) return len == 0.0f ? p.side_min : p.side_max;
  const float var = max0(m2 - m1 * m1);
  const float rel = sqrt_rn(var) / (__builtin_fabsf(m1) + p.lum_floor);
  float w = __builtin_ceilf(rel * p.gain);
  w = w < p.side_min_f ? p.side_min_f : w;
  w = w > p.side_max_f ? p.side_max_f : w;
  return (uint32_t)w;
}

__global__ void __launch_bounds__(kSpFlat)
k_sp_want(SamplePlan p, const float* __restrict__ len, const float* __restrict__ mom, uint8_t* __restrict__ want) {
  const size_t n = (size_t)p.W * p.H;
  const size_t i = (size_t)blockIdx.x * kSpFlat + threadIdx.x;
  if (i >= n) return;
  want[i] = (uint8_t)wanted_side(p, len[i], mom[i], mom[n + i]);
}

__global__ void __launch_bounds__(kSpX * kSpY)
k_sp_dilate(SamplePlan p, const uint8_t* __restrict__ want, uint8_t* __restrict__ map, uint32_t* __restrict__ bins) {
  __shared__ uint32_t s_bins[kSampleBins];
  const uint32_t t = threadIdx.y * kSpX + threadIdx.x;
  s_bins[t] = 0u;  // kSpX * kSpY == kSampleBins
  __syncthreads();
  const uint32_t x = blockIdx.x * kSpX + threadIdx.x, y = blockIdx.y * kSpY + threadIdx.y;
  if (x < p.W && y < p.H) {
    const int r = (int)p.dilate;
    uint32_t m = 0;
    for (int dy = -r; dy <= r; ++dy) {
      const int yy = (int)y + dy;
      if (yy < 0 || yy >= (int)p.H) continue;
      for (int dx = -r; dx <= r; ++dx) {
        const int xx = (int)x + dx;
        if (xx < 0 || xx >= (int)p.W) continue;
        const uint32_t w = want[(size_t)yy * p.W + xx];
        m = w > m ? w : m;
      }
    }
    map[(size_t)y * p.W + x] = (uint8_t)m;
    atomicAdd(&s_bins[m], 1u);
  }
  __syncthreads();
  if (s_bins[t]) atomicAdd(&bins[t], s_bins[t]);
}
static_assert(kSpX * kSpY == (int)kSampleBins, "one lane per bin");

// bins[kSampleBins] receives the cap
__global__ void __launch_bounds__(kSampleBins)
k_sp_cap(SamplePlan p, uint32_t* __restrict__ bins, unsigned long long* __restrict__ total) {
  __shared__ uint32_t s_bins[kSampleBins];
  __shared__ unsigned long long s_total[kSampleBins];
  const uint32_t t = threadIdx.x;
  s_bins[t] = bins[t];
  __syncthreads();
  s_total[t] = sample_plan_total(s_bins, t);
  __syncthreads();
  if (t == 0) {
    uint32_t c = p.side_max;
    if (p.budgeted) {
      while (c > p.side_min && s_total[c] > p.budget) --c;  // side_min when not even it meets the budget
    }
    bins[kSampleBins] = c;
    if (total) *total = s_total[c];
  }
}

__global__ void __launch_bounds__(kSpFlat)
k_sp_apply(SamplePlan p, const uint32_t* __restrict__ bins, uint8_t* __restrict__ map) {
  const uint32_t c = bins[kSampleBins];
  if (c >= p.side_max) return;  // no dilated side is above side_max
  const size_t n = (size_t)p.W * p.H;
  const size_t i = (size_t)blockIdx.x * kSpFlat + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = map[i];
  if (m > c) map[i] = (uint8_t)c;
}

}  // namespace

hipError_t launch_sample_plan(const SamplePlan& p, const float* len, const float* moments, void* ws, uint8_t* map,
                              unsigned long long* total, hipStream_t stream) {
  const size_t n = (size_t)p.W * p.H;
  if (n == 0) return hipSuccess;
  uint8_t* want = (uint8_t*)ws + p.off_want;
  uint32_t* bins = (uint32_t*)((char*)ws + p.off_bins);
  hipError_t e = hipMemsetAsync(bins, 0, (kSampleBins + 1) * sizeof(uint32_t), stream);
  if (e != hipSuccess) return e;
  const dim3 flat((uint32_t)((n + kSpFlat - 1) / kSpFlat));
  k_sp_want<<<flat, kSpFlat, 0, stream>>>(p, len, moments, want);
  const dim3 grid((p.W + kSpX - 1) / kSpX, (p.H + kSpY - 1) / kSpY), block(kSpX, kSpY);
  k_sp_dilate<<<grid, block, 0, stream>>>(p, want, map, bins);
  k_sp_cap<<<1, kSampleBins, 0, stream>>>(p, bins, total);
  if (p.budgeted) k_sp_apply<<<flat, kSpFlat, 0, stream>>>(p, bins, map);
  return hipGetLastError();
}

}  // namespace wgt
