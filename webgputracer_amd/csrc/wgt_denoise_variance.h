// wgt_denoise_variance.h — what the variance-guided denoiser's planning (host/launch_plan.cpp), its
// thin calls (wgt_runtime.cpp) and its kernels (wgt_denoise_variance.hip) share: the plan of one call
// and the launcher.  The size limits, the alignment and the tiled-step switch are wgt_denoise's.
#pragma once

#include "wgt_denoise.h"

namespace wgt {

constexpr uint32_t kDenoiseVarianceMaxMinHistory = 64;

// One call, decided on the host (plan_denoise_variance).  The workspace of a W x H image, each part
// kDenoiseAlign-aligned within it:
//   rec : 2 float4 per pixel, (normal.xyz, not valid: 0, valid: 1, valid under a history shorter than
//         min_history: 2) and (position.xyz, the input's alpha): a tap's guides in two 16-byte loads
//   it0, it1 : float4 per pixel, the iterates (rgb / albedo, variance), ping-pong; a pixel that is
//         not valid carries (its input rgb, -1) through them unchanged: a variance is never negative,
//         so the sign tells the 3 x 3 prefilter which neighbours count
struct DenoiseVariancePlan {
  uint32_t W, H;
  uint32_t iterations, normal_power, demodulate;
  float kz[kDenoiseMaxIterations];  // of pass i: (1 / sigma_pos^2) * 4^-i; kz[0] is the spatial estimate's too
  float sigma_lum;
  float min_history;                // the parameter as a float: len is compared with it and divides it
  uint32_t tiled_max_step;          // passes with a step up to this run LDS-tiled, the others gather (0: none)
  size_t off_rec, off_it0, off_it1, bytes;
};

// Launcher implemented in wgt_denoise_variance.hip: the pack pass, the spatial variance estimate, then
// plan.iterations a-trous passes, the last of which remodulates and writes out32 and/or out8 and var
// (device pointers; any may be null), all on `stream`.  state.rgba32f and out32 may alias: only the
// pack pass reads the state, and only the last pass writes out.
hipError_t launch_denoise_variance(const DenoiseVariancePlan& plan, const wgt_temporal_state& state,
                                   const wgt_hit_buffers& guides, void* ws, float4* out32, uchar4* out8, float* var,
                                   hipStream_t stream);

}  // namespace wgt
