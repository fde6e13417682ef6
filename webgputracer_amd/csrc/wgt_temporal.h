// wgt_temporal.h — what the temporal accumulation's planning (host/launch_plan.cpp), its thin calls
// (wgt_runtime.cpp) and its kernel (wgt_temporal.hip) share: the plan of one call and the launcher.
// A header of its own, as wgt_denoise.h: the render, query, refit and denoise kernels' translation
// units do not see it.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/wgt_api.h"

namespace wgt {

constexpr uint32_t kTemporalMaxHistory = 65536;
constexpr float kTemporalMinWeight = 0x1p-6f;  // history needs usable bilinear weights summing to this

// The projection constants of one camera, derived on the host from make_frame:
// a degenerate camera gives NaN constants, so no pixel finds history.
struct TemporalCam {
  float o[3];    // the origin
  float c[3];    // from the origin to the centre of pixel (0, 0)
  float nrm[3];  // cross(du, dv)
  float iu[3];   // du / dot(du, du)
  float iv[3];   // dv / dot(dv, dv)
  float k;       // dot(c, nrm)
};

// One call, decided on the host (plan_temporal).
struct TemporalPlan {
  uint32_t W, H;
  uint32_t first;       // the first-frame form: no previous frame, every pixel starts a history
  uint32_t match_prim;  // WGT_TEMPORAL_MATCH_PRIM
  float max_history;    // (float)params.max_history: exact, at most 2^16
  float normal_min, plane_tol;
  TemporalCam cam, cam_prev;  // cam_prev: zeros in the first-frame form
};

// Launcher implemented in wgt_temporal.hip: one pass on `stream`.  Device pointers; prev and
// guides_prev are null in the first-frame form (plan.first); out.moments and out8 may be null.
// out.rgba32f may equal `in` (each pixel reads only its own current colour); no out buffer may
// overlap the prev buffer of the same name (the callers' checks hold this).  motion (null: the plain
// form): the pixels' pos_prev and norm_prev of wgt_temporal_accumulate_motion, unused in the
// first-frame form.
hipError_t launch_temporal(const TemporalPlan& plan, const float4* in, const wgt_hit_buffers& guides,
                           const wgt_motion_buffers* motion, const wgt_temporal_state* prev,
                           const wgt_hit_buffers* guides_prev,
                           const wgt_temporal_state& out, uchar4* out8, hipStream_t stream);

}  // namespace wgt
