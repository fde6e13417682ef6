// wgt_radiance.h — what the radiance queries' launch (wgt_radiance.hip) and its plan
// (host/launch_plan.h plan_radiance) share: the launch's uniform arguments and the launchers.
#pragma once

#include "wgt_internal.h"

namespace wgt {

constexpr uint32_t kRadianceMaxSamples = 65536;

// One kernel argument: the call's uniform values and the launch form (plan_radiance).
struct RadianceArgs {
  uint32_t n, samples, seed0;
  float fs;      // f32(samples)
  float inv_fs;  // 1 / fs when samples is a power of two (exact: the kernels multiply), else 0
  // the form: the persistent phase-split kernel (scenes with triangles) or the flat one; the
  // persistent kernel on the 80-B compact records (with the 128-B form behind the origin-bound gate)
  uint32_t persistent, compact;
  // the phase thresholds and the refill trigger of the persistent form, as k_render_ps's (DevFrame)
  uint32_t to_trav, to_service, svc_frac, tri_ratio, refill;
};

// Launchers implemented in wgt_radiance.hip
// d_ws: two words of the context's, used in stream order (the ray queue's counter and the origin-bound
// flag; the persistent form only).  resident: radiance_resident_waves.  d_counts (may be null) selects
// the counting instantiations: += queries, traced, paths, NaN-ray queries.
hipError_t launch_radiance(const DevScene& sc, const RadianceArgs& a, const float* d_rays, const uint32_t* d_seeds,
                           const wgt_radiance_buffers& out, unsigned long long* d_counts, uint32_t resident,
                           uint32_t* d_ws, hipStream_t stream);
// Waves of k_radiance_ps resident on the whole device for this scene's LDS stack (both node forms).
hipError_t radiance_resident_waves(const DevScene& sc, int device, uint32_t& waves);

}  // namespace wgt
