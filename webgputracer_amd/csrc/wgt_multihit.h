// wgt_multihit.h — what the multi-hit queries' launch (wgt_multihit.hip) and its plan
// (host/launch_plan.h plan_multi_hit) share: the launch form, the LDS layout's size and the launcher.
#pragma once

#include "wgt_internal.h"

namespace wgt {

// The kernel's form.  kMultiHitCount: every hit is counted and the bound on the ray parameter stays the
// limit's (out->count asked for); its node step descends in slot order, as k_occluded's.  kMultiHitCull:
// the bound shrinks to the k-th distance once the list is full, and the node step sorts the children by
// entry distance, as trav_step's (the slot-order step was measured in this form too and lost: DESIGN.md §4.15).
enum MultiHitMode : uint32_t { kMultiHitCount, kMultiHitCull };

// One kernel argument: the call's uniform values and the launch form (plan_multi_hit).
struct MultiHitPlan {
  uint32_t n;
  uint32_t k;          // list entries per ray: 0 when neither prim nor dist is asked for
  uint32_t tris_only;  // WGT_MULTI_HIT_TRIS_ONLY: quads, lights and spheres are not tested
  uint32_t mode;       // MultiHitMode
  uint32_t lds;        // dynamic LDS bytes of the launch (multi_hit_lds_bytes)
};

// The LDS of one workgroup (one wave): the traversal stack of `stack` entries per lane, then the lanes'
// hit lists, k distances and k primitive ids each, all at stride kBlock.
constexpr size_t multi_hit_lds_bytes(uint32_t stack, uint32_t k) {
  return stack_lds_bytes(stack) + 2 * (size_t)k * kBlock * 4;
}
constexpr size_t kLdsPerWorkgroup = 64 * 1024;
static_assert(multi_hit_lds_bytes(kStackMax + 1, WGT_MULTI_HIT_MAX_K) <= kLdsPerWorkgroup,
              "the deepest stack and the longest list fit one workgroup's LDS");

// Launcher implemented in wgt_multihit.hip
// d_rays: six planes of p.n floats; d_max_dist may be null (no limit); out: device pointers, a null field
// is not written.  d_counts (may be null) selects the counting instantiations: += node visits, triangle
// tests.
hipError_t launch_multi_hit(const DevScene& sc, const MultiHitPlan& p, const float* d_rays, const float* d_max_dist,
                            const wgt_multi_hit_buffers& out, unsigned long long* d_counts, hipStream_t stream);

}  // namespace wgt
