// wgt_nearest_k.h — the k-nearest and within-radius closest-point query (wgt_nearest_k_points,
// DESIGN.md §4.16): its definition on top of wgt_nearest.h's per-triangle one, compiled for both sides
// (the kernel, wgt_nearest_k.hip, and the host's brute force wgt_nearest_k_points_spec,
// host/launch_plan.cpp), and what the launch and its plan (host/launch_plan.h plan_nearest_k) share: the
// launch form, the LDS layout's size and the launcher.
//
// For point p and radius m = max_dist[i] (none: +inf), with d2_t = nearest_on_tri(p, v0, e1, e2).d2 on
// triangle t's resident record:
//   S = { t : d2_t < +inf and sqrt_rn(d2_t) < m }                (nearest_k_member; IEEE f32 comparisons:
//                                                                 a NaN d2 is in no set, a NaN, zero or
//                                                                 negative m gives the empty set)
//   count = |S|, all of it, not capped at k
//   entry j < k = the j-th element of S by (d2, id) ascending    (nearest_k_less; d2 compared as f32)
//               = (prim = n_lights + n_quads + id, dist = sqrt_rn(d2), pos = q, uv = (v, w)), q, v and w
//                 from nearest_on_tri on the record again, as k_nearest recomputes its winner's
//   entries j >= min(|S|, k) = (kNoHit, +inf, 0, 0)
// A point with a NaN or infinite component has no finite d2 against finite triangles: S is empty, and
// both sides say so before they look at a triangle.  Only triangles are searched.
//
// Consequences (tests/test_nearest_k_restatement.py asserts each):
//   - sqrt_rn is monotone, so S is a prefix of the (d2, id) order over all triangles with a finite d2:
//     the first k of S are the first k of that order, cut where sqrt_rn(d2) < m first fails.  The cull
//     form relies on it: it keeps the first k of the whole order and applies the radius at the write-out.
//   - the list for k is a prefix of the list for any larger k.
//   - entry 0 equals wgt_nearest_points' record bit for bit, in all four fields, for the same point and
//     radius: the minimum of (d2, id) by nearest_better is the first element of the order, and
//     nearest_reported is nearest_k_member's radius half.
//   - two triangles with different d2 can round to the same dist: they are ordered by d2, not by id.
#pragma once

#include "wgt_internal.h"
#include "wgt_nearest.h"

namespace wgt {

// t is in S: a finite d2 (not NaN, not +inf) whose rounded root is below the radius.
WGT_HD bool nearest_k_member(float d2, float m) { return (d2 < __builtin_inff()) & (sqrt_rn(d2) < m); }
// The list's order: (d2, id) ascending.  Both d2 are finite and not negative where this is called.
WGT_HD bool nearest_k_less(float da, uint32_t ia, float db, uint32_t ib) { return (da < db) | ((da == db) & (ia < ib)); }

// The kernel's form.  kNearestKCount: every member of S is counted and the cull bound stays the radius'
// (out->count asked for); its node step descends in slot order for the count alone and nearest first when it
// also fills a list (NearestKPlan::sort).  kNearestKCull: the bound shrinks to the
// k-th d2's once the list is full, and the node step descends nearest first, as k_nearest's.
enum NearestKMode : uint32_t { kNearestKCount, kNearestKCull };

// One kernel argument: the call's uniform values and the launch form (plan_nearest_k).
struct NearestKPlan {
  uint32_t n;
  uint32_t k;      // list entries per point: 0 when no list field is asked for
  uint32_t words;  // list words per entry: d2 and id, and the record's byte offset when pos or uv is asked for
  uint32_t mode;   // NearestKMode
  uint32_t sort;   // the count form's node step descends nearest first too: set when it fills a list
                   // (plan_nearest_k; WGT_NEAREST_K_SORT forces either, the A/B of DESIGN.md §4.16)
  uint32_t lds;    // dynamic LDS bytes of the launch (nearest_k_lds_bytes)
};
constexpr uint32_t kNearestKMaxWords = 3;

// The LDS of one workgroup (one wave): the traversal stack of `stack` entries per lane, then the lanes'
// lists, `words` planes of k entries each (d2 bits, ids, record offsets), all at stride kBlock.
constexpr size_t nearest_k_lds_bytes(uint32_t stack, uint32_t k, uint32_t words) {
  return stack_lds_bytes(stack) + (size_t)words * k * kBlock * 4;
}
constexpr size_t kNearestKLdsPerWorkgroup = 64 * 1024;
static_assert(nearest_k_lds_bytes(kStackMax + 1, WGT_NEAREST_MAX_K, kNearestKMaxWords) <= kNearestKLdsPerWorkgroup,
              "the deepest stack and the longest list fit one workgroup's LDS");

// Launcher implemented in wgt_nearest_k.hip
// d_points: three planes of p.n floats; d_max_dist may be null (no radius); out: device pointers, a null
// field is not written.  d_counts (may be null) selects the counting instantiations: += node visits,
// triangle tests.
hipError_t launch_nearest_k(const DevScene& sc, const NearestKPlan& p, const float* d_points, const float* d_max_dist,
                            const wgt_nearest_k_buffers& out, unsigned long long* d_counts, hipStream_t stream);

}  // namespace wgt
