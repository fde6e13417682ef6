// wgt_overlap_self.h — the self-intersection query (wgt_overlap_self): which resident
// triangles each resident triangle cuts, neighbours by the mesh's index buffer excluded.  The definition,
// compiled for both sides (the kernel, wgt_overlap_self.hip, and the host's brute force wgt_overlap_self_spec,
// host/launch_plan.cpp), so a decision either side takes has the same bits, and what the launch and its plan
// (host/launch_plan.h plan_overlap_self) share.  Plain IEEE fp32 +, -, *, comparisons and selects, no
// contraction (-ffp-contract=off), every operation in the order written here, and no division anywhere.
// seg_crosses, overlap_segments and overlap_boxes are wgt_overlap.h's, unchanged.
//
// For resident triangles s and t (ids are upload indices, word A.w of the record), each with its record
// (v0, e1, e2) and its padded box tri_box(v0, e1, e2) (row D of the record):
//   corners(x)      = (v0, fl(v0 + e1), fl(v0 + e2)), the sums tri_box forms
//   adjacent(s, t)  = with an index buffer (3 * n_tris uint32_t labels), any of s's three labels equals any
//                     of t's: nine integer comparisons.  Labels are compared for equality only; they are never
//                     addresses and need no range check.  Without an index buffer nothing is adjacent.
//   self_overlap(s, t), with lo = min(s, t) and hi = max(s, t):
//                     s != t and not adjacent(s, t) and overlap_boxes(padded box of s, padded box of t)
//                     and overlap_segments(corners(lo), record(hi))
// The lower id is always the query and the higher id always the resident, and the box clause is symmetric
// (six comparisons with equality, each the mirror of another), so the decision is one function of the
// unordered pair: t is in S_s iff s is in S_t, bit for bit.
//
// The answer for triangle s, with S_s = { t : self_overlap(s, t) }, in wgt_overlap_buffers sized n_tris and
// indexed by upload index:
//   count = |S_s|, all of it, not capped at k;   hit = count > 0
//   entry j < k = the j-th lowest id of S_s, as n_lights + n_quads + id;   entries j >= min(|S_s|, k) = kNoHit
// Only triangles are searched.
//
// Why the tree's cull is exact: lane s traverses with its own padded box; every node box is the exact union
// (minima and maxima) of the padded boxes below it; so a child whose box misses s's padded box holds no t that
// passes the box clause, by plain comparisons.  And the box clause removes no real intersection: two
// triangles that meet have a common point, which lies in both corner boxes, and a corner box nests in its
// padded box by monotone rounding (fl(mn - pad) <= mn and fl(mx + pad) >= mx for pad >= 0).
//
// Relation to wgt_overlap_triangles: for s < t not adjacent, tri_overlap(corners(s), record t) implies
// self_overlap(s, t): the same segment tests run on the same operands, and the box clause here (padded
// against padded) is a superset of that one (corner box against padded).
//
// Limits: two triangles that share a label and still cut each other (a fold through a shared vertex) are not
// reported; coplanar pairs are never reported (all six determinants are zero); only triangles are searched.
#pragma once

#include "wgt_overlap.h"

namespace wgt {

// adjacent(s, t) by labels: a = s's three, b = t's three.
WGT_HD bool self_adjacent(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t b0, uint32_t b1, uint32_t b2) {
  return (a0 == b0) | (a0 == b1) | (a0 == b2) | (a1 == b0) | (a1 == b1) | (a1 == b2) | (a2 == b0) | (a2 == b1) |
         (a2 == b2);
}

// The segment clause of a pair: the lower id's record gives the corners, the higher id's record is the
// resident triangle.
WGT_HD bool self_segments(f3 lv0, f3 le1, f3 le2, f3 hv0, f3 he1, f3 he2) {
  return overlap_segments(lv0, lv0 + le1, lv0 + le2, hv0, he1, he2);
}

// One kernel argument: the call's uniform values and the launch form (plan_overlap_self).
struct OverlapSelfPlan {
  uint32_t n;    // the scene's triangles: one lane each
  uint32_t k;    // list entries per triangle: 0 when prim is not asked for
  uint32_t any;  // only hit is asked for: the traversal ends at the first member
  uint32_t lds;  // dynamic LDS bytes of the launch (overlap_lds_bytes)
};

// Launcher implemented in wgt_overlap_self.hip
// d_index: 3 * p.n labels by upload index, or null (nothing is adjacent); out: device pointers sized p.n, a
// null field is not written.  d_counts (may be null) selects the counting instantiations: += node visits,
// triangle tests.
hipError_t launch_overlap_self(const DevScene& sc, const OverlapSelfPlan& p, const uint32_t* d_index,
                               const wgt_overlap_buffers& out, unsigned long long* d_counts, hipStream_t stream);

}  // namespace wgt
