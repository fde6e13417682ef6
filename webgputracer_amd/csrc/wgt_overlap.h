// wgt_overlap.h — the triangle overlap query (wgt_overlap_triangles): which resident
// triangles a caller's triangle cuts.  The definition, compiled for both sides (the kernel,
// wgt_overlap.hip, and the host's brute force wgt_overlap_triangles_spec, host/launch_plan.cpp), so a
// decision either side takes has the same bits, and what the launch and its plan (host/launch_plan.h
// plan_overlap) share: the launch form, the LDS layout's size and the launcher.  Plain IEEE fp32 +, -, *,
// comparisons and selects, no contraction (-ffp-contract=off), every operation in the order written here,
// and no division anywhere.
//
// For the query triangle A = (a0, a1, a2) given by its corners and the resident triangle B given by its
// record (v0, e1, e2) and its padded box [lo, hi] = tri_box(v0, e1, e2) (row D of the resident record):
//   tri_overlap(A, B) = box clause and at least one of six segment tests
//   box clause: on each axis min(a0, a1, a2) <= hi and max(a0, a1, a2) >= lo   (exact; the query gets no pad)
//   segment tests, in this order, seg_crosses(origin, direction, triangle):
//     A's edges against B:  (a0, a1 - a0), (a1, a2 - a1), (a2, a0 - a2)  against (v0, e1, e2)
//     B's edges against A:  (v0, e1), (v0, e2), (v0 + e1, e2 - e1)       against (a0, a1 - a0, a2 - a0)
// A query is valid (overlap_query_ok) iff its nine coordinates are finite and within 2^40 and every
// component of a1 - a0, a2 - a0 and a2 - a1 is within 2^30 (the scene's own triangle limits,
// host/launch_plan.h check_triangle_limits); an invalid query's answer is empty on both sides before any
// triangle is looked at.
//
// The answer for query i, with S = { t : tri_overlap(A_i, record_t) }:
//   count = |S|, all of it, not capped at k;   hit = count > 0
//   entry j < k = the j-th lowest primitive id of S, as n_lights + n_quads + id
//   entries j >= min(|S|, k) = kNoHit
// Only triangles are searched.
//
// Consequences (tests/test_overlap_restatement.py asserts each):
//   - The box clause removes no real intersection: the pad only enlarges B, and two triangles that meet
//     have a common point, which lies in both their boxes.  It makes the tree's cull exact: every node box
//     is a union (exact minima and maxima) of the tri boxes below it, so a query box that misses a node box
//     misses every tri box below it, with plain comparisons, bit for bit, at any magnitude.  The traversal
//     answers what the brute force answers with no error analysis: no slack, no shrink, no premise on the
//     triangles' shapes.
//   - Coplanar pairs are never reported: all six determinants are zero.  Nearly coplanar pairs are decided
//     by rounding.
//   - A triangle that lies wholly inside a closed mesh cuts nothing: callers combine this query with
//     Context.points_inside.
//   - Touching counts: the comparisons admit equality.  Neighbours in one mesh that share a vertex or an
//     edge therefore usually report each other; a self-intersection check must filter those by id.
//   - The list for k is a prefix of the list for any larger k; hit equals count > 0.
#pragma once

#include "wgt_geom.h"
#include "wgt_internal.h"

namespace wgt {

// The segment o + t d, 0 <= t <= 1, crosses the triangle (w0, w0 + f1, w0 + f2): two-sided
// Moller-Trumbore with the quotients cleared (u = U / det, v = V / det, t = T / det, all compared after
// multiplying through by |det|).  Negation is exact, so the two signs of det are one test.  Every clause
// is a positive comparison: a NaN operand gives "no", and so does a zero determinant (a segment parallel
// to the plane, or a determinant that underflowed).
//
// Nothing overflows under the limits (coordinates within 2^40, so |tv| components <= 2^41; edge components
// within 2^30): a component of p or q is a difference of two products, |p| <= 2 * 2^30 * 2^30 = 2^61 and
// |q| <= 2 * 2^41 * 2^30 = 2^72, hence
//   |det| = |dot(f1, p)| <= 3 * 2^30 * 2^61 = 3 * 2^91,
//   |U| = |dot(tv, p)| <= 3 * 2^41 * 2^61 = 3 * 2^102, |V| = |dot(d, q)| and |T| = |dot(f2, q)| <= 3 * 2^30 * 2^72
//   = 3 * 2^102, and U' + V' <= 6 * 2^102 < 2^105.
// The resident triangle's third edge e2 - e1 is the one direction the limits bound by 2^31, not 2^30: with
// it as d the bounds double, which is as far from 2^128.
WGT_HD bool seg_crosses(f3 o, f3 d, f3 w0, f3 f1, f3 f2) {
  const f3 p = cross(d, f2);
  const float det = dot(f1, p);
  const f3 tv = o - w0;
  const float U = dot(tv, p);
  const f3 q = cross(tv, f1);
  const float V = dot(d, q);
  const float T = dot(f2, q);
  const bool neg = det < 0.0f;
  const float a = neg ? -det : det, Up = neg ? -U : U, Vp = neg ? -V : V, Tp = neg ? -T : T;
  return (a > 0.0f) & (Up >= 0.0f) & (Vp >= 0.0f) & (Up + Vp <= a) & (Tp >= 0.0f) & (Tp <= a);
}

// The query's own box: exact minima and maxima of its corners, no pad.
WGT_HD float min3_w(float a, float b, float c) {
  const float m = a < b ? a : b;
  return m < c ? m : c;
}
WGT_HD float max3_w(float a, float b, float c) {
  const float m = a > b ? a : b;
  return m > c ? m : c;
}
WGT_HD void overlap_query_box(f3 a0, f3 a1, f3 a2, f3& qlo, f3& qhi) {
  qlo = f3{min3_w(a0.x, a1.x, a2.x), min3_w(a0.y, a1.y, a2.y), min3_w(a0.z, a1.z, a2.z)};
  qhi = f3{max3_w(a0.x, a1.x, a2.x), max3_w(a0.y, a1.y, a2.y), max3_w(a0.z, a1.z, a2.z)};
}
// The query's box [qlo, qhi] overlaps the box [lo, hi] on all three axes: six positive comparisons.  It
// is the box clause on a triangle's padded box and the kernel's node test on a child's box.
WGT_HD bool overlap_boxes(f3 qlo, f3 qhi, float lox, float hix, float loy, float hiy, float loz, float hiz) {
  return (qlo.x <= hix) & (qhi.x >= lox) & (qlo.y <= hiy) & (qhi.y >= loy) & (qlo.z <= hiz) & (qhi.z >= loz);
}

// The six segment tests, with an early-out after each that says yes.
WGT_HD bool overlap_segments(f3 a0, f3 a1, f3 a2, f3 v0, f3 e1, f3 e2) {
  if (seg_crosses(a0, a1 - a0, v0, e1, e2)) return true;
  if (seg_crosses(a1, a2 - a1, v0, e1, e2)) return true;
  if (seg_crosses(a2, a0 - a2, v0, e1, e2)) return true;
  const f3 g1 = a1 - a0, g2 = a2 - a0;
  if (seg_crosses(v0, e1, a0, g1, g2)) return true;
  if (seg_crosses(v0, e2, a0, g1, g2)) return true;
  return seg_crosses(v0 + e1, e2 - e1, a0, g1, g2);
}

// Two triangles overlap: the box clause first, the segment tests only when it holds.
WGT_HD bool tri_overlap(f3 a0, f3 a1, f3 a2, f3 v0, f3 e1, f3 e2, f3 lo, f3 hi) {
  f3 qlo, qhi;
  overlap_query_box(a0, a1, a2, qlo, qhi);
  if (!overlap_boxes(qlo, qhi, lo.x, hi.x, lo.y, hi.y, lo.z, hi.z)) return false;
  return overlap_segments(a0, a1, a2, v0, e1, e2);
}

// The query is valid: positive comparisons again, so a NaN or an infinity fails.
constexpr float kOverlapCoordLimit = 0x1p40f;
constexpr float kOverlapEdgeLimit = 0x1p30f;
WGT_HD bool overlap_within(f3 v, float lim) {
  const float x = fabs_w(v.x), y = fabs_w(v.y), z = fabs_w(v.z);
  return (x <= lim) & (y <= lim) & (z <= lim);
}
WGT_HD bool overlap_query_ok(f3 a0, f3 a1, f3 a2) {
  const bool c0 = overlap_within(a0, kOverlapCoordLimit), c1 = overlap_within(a1, kOverlapCoordLimit),
             c2 = overlap_within(a2, kOverlapCoordLimit);
  const bool g1 = overlap_within(a1 - a0, kOverlapEdgeLimit), g2 = overlap_within(a2 - a0, kOverlapEdgeLimit),
             g3 = overlap_within(a2 - a1, kOverlapEdgeLimit);
  return c0 & c1 & c2 & g1 & g2 & g3;
}
// An empty node slot is the point box at kEmptySlotCoord; a valid query's box ends at 2^40 at most, so its
// upper corner is below the slot's lower one and the node test never keeps it.
static_assert(kOverlapCoordLimit < kEmptySlotCoord, "an empty slot overlaps no valid query");

// One kernel argument: the call's uniform values and the launch form (plan_overlap).
struct OverlapPlan {
  uint32_t n;
  uint32_t k;    // list entries per query: 0 when prim is not asked for
  uint32_t any;  // only hit is asked for: the traversal ends at the first overlapping triangle
  uint32_t lds;  // dynamic LDS bytes of the launch (overlap_lds_bytes)
};

// The LDS of one workgroup (one wave): the traversal stack of `stack` entries per lane, then the lanes'
// lists of k ids, one word per entry, all at stride kBlock.
constexpr size_t overlap_lds_bytes(uint32_t stack, uint32_t k) { return stack_lds_bytes(stack) + (size_t)k * kBlock * 4; }
constexpr size_t kOverlapLdsPerWorkgroup = 64 * 1024;
static_assert(overlap_lds_bytes(kStackMax + 1, WGT_OVERLAP_MAX_K) <= kOverlapLdsPerWorkgroup,
              "the deepest stack and the longest list fit one workgroup's LDS");

// The lane's list in LDS (k_overlap, k_overlap_self): entry j's id at list[j * kBlock], j < len <= k,
// ascending.  Inserts id if it belongs among the k lowest; every index written is at most k - 1.  A query
// meets each id once.
__device__ __forceinline__ void ov_insert(int* __restrict__ list, uint32_t k, uint32_t& len, uint32_t id) {
  if (k == 0) return;
  uint32_t j = len;
  if (len == k) {
    j = k - 1;
    if (!(id < (uint32_t)list[j * kBlock])) return;
  } else {
    ++len;
  }
  while (j > 0) {
    const int I = list[(j - 1) * kBlock];
    if (!(id < (uint32_t)I)) break;
    list[j * kBlock] = I;
    --j;
  }
  list[j * kBlock] = (int)id;
}

// Launcher implemented in wgt_overlap.hip
// d_tris: nine planes of p.n floats (a0.x a0.y a0.z a1.x ... a2.z); out: device pointers, a null field is
// not written.  d_counts (may be null) selects the counting instantiations: += node visits, triangle tests.
hipError_t launch_overlap(const DevScene& sc, const OverlapPlan& p, const float* d_tris, const wgt_overlap_buffers& out,
                          unsigned long long* d_counts, hipStream_t stream);

}  // namespace wgt
