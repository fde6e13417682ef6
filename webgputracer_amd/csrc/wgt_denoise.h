// wgt_denoise.h — what the denoiser's planning (host/launch_plan.cpp), its thin calls
// (wgt_runtime.cpp) and its kernels (wgt_denoise.hip) share: the plan of one call and the launcher.
// A header of its own, so that the render, query and refit kernels' translation units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/wgt_api.h"

namespace wgt {

constexpr uint32_t kDenoiseMaxDim = 32768;         // W, H
constexpr uint32_t kDenoiseMaxPixels = 1u << 25;   // W * H: every element index of the workspace < 2^27
constexpr uint32_t kDenoiseMaxIterations = 8;
constexpr uint32_t kDenoiseMaxNormalPower = 10;
constexpr size_t kDenoiseAlign = 256;
// The largest step whose LDS tile (8 rows of 64 + 4 step records of 48 B: 49 KB at 16) stays within
// the 64 KB a workgroup gets without asking for more, and the largest at which the tiled pass was
// measured faster than the gather: the default of WGT_DENOISE_TILED_STEP
constexpr uint32_t kDenoiseMaxTiledStep = 16;
constexpr uint32_t kDenoiseTiledStep = 8;

// One call, decided on the host (plan_denoise).  The workspace of a W x H image, each part
// kDenoiseAlign-aligned within it:
//   rec : 2 float4 per pixel, (normal.xyz, valid ? 1 : 0) and (position.xyz, 0): a tap's guides in
//         two 16-byte loads
//   it0, it1 : float4 per pixel, the iterates (rgb / albedo, the input's alpha), ping-pong; a pixel
//         that is not valid carries its input colour through them unchanged
struct DenoisePlan {
  uint32_t W, H;
  uint32_t iterations, normal_power, demodulate;
  float kz[kDenoiseMaxIterations];  // of pass i: (1 / sigma_pos^2) * 4^-i
  uint32_t tiled_max_step;          // passes with a step up to this run LDS-tiled, the others gather (0: none)
  size_t off_rec, off_it0, off_it1, bytes;
};

// Launcher implemented in wgt_denoise.hip: the pack pass, then plan.iterations a-trous passes, the
// last of which remodulates and writes out32 and/or out8 (device pointers; one may be null), all on
// `stream`.  in and out32 may alias: only the pack pass reads in, and only the last pass writes out.
hipError_t launch_denoise(const DenoisePlan& plan, const float4* in, const wgt_hit_buffers& guides, void* ws,
                          float4* out32, uchar4* out8, hipStream_t stream);

}  // namespace wgt
