// wgt_nearest.h — the definition of the closest-point query (wgt_nearest_points),
// compiled for both sides: the kernel (wgt_nearest.hip) and the host's brute force
// (wgt_nearest_points_spec, host/launch_plan.cpp) call these functions, so a value either side
// computes has the same bits.  Plain IEEE fp32 +, -, *, /, comparisons and selects, no contraction
// (-ffp-contract=off), every operation in the order written here.
//
// The answer for a point p is the minimum of (d2, primitive id) over the scene's triangles, d2 the
// squared distance from p to the closest point of the triangle as nearest_on_tri computes it, taken
// with nearest_better: a NaN or infinite d2 is never the answer.  dist = sqrt_rn(d2); the record is
// reported iff dist < max_dist (nearest_reported), else the miss record: prim = kNoHit, dist = +inf,
// pos = 0, uv = 0.
//
// Only triangles are searched (their primitive ids are the scene's: n_lights + n_quads + index);
// quads, lights and spheres are out of scope.  So is a signed distance (it needs angle-weighted
// pseudo-normals at edges and vertices).  The k nearest triangles and the number within the radius are
// wgt_nearest_k_points' answers (wgt_nearest_k.h), built on this per-triangle definition.
#pragma once

#include "wgt_math.h"

namespace wgt {

// The region of the triangle's plane the point projects into: which of the triangle's features
// carries the closest point.
enum NearestRegion : int { kNearVertex = 0, kNearEdge = 1, kNearFace = 2 };

struct NearestTri {
  float d2;    // squared distance from p to q
  float v, w;  // q = (v0 + v e1) + w e2
  f3 q;        // the closest point
  int region;  // NearestRegion
};

// The closest point of the triangle (v0, v0 + e1, v0 + e2) to p: the seven-region test of Ericson,
// Real-Time Collision Detection §5.1.5, with a = v0, ab = e1, ac = e2.  The other two corners are
// never rebuilt: p - b = (p - a) - ab and p - c = (p - a) - ac.  In order:
//   ap = p - v0                      d1 = dot(e1, ap)   d2 = dot(e2, ap)     dot: (x x + y y) + z z
//   bp = ap - e1                     d3 = dot(e1, bp)   d4 = dot(e2, bp)
//   cp = ap - e2                     d5 = dot(e1, cp)   d6 = dot(e2, cp)
//   vc = d1 d4 - d3 d2    vb = d5 d2 - d1 d6    va = d3 d6 - d5 d4
//   e43 = d4 - d3         e56 = d5 - d6
// The first test that holds names the region and its weights (v, w):
//   1. d1 <= 0 and d2 <= 0                    vertex a   (0, 0)
//   2. d3 >= 0 and d4 <= d3                   vertex b   (1, 0)
//   3. vc <= 0 and d1 >= 0 and d3 <= 0        edge ab    (d1 / (d1 - d3), 0)
//   4. d6 >= 0 and d5 <= d6                   vertex c   (0, 1)
//   5. vb <= 0 and d2 >= 0 and d6 <= 0        edge ac    (0, d2 / (d2 - d6))
//   6. va <= 0 and e43 >= 0 and e56 >= 0      edge bc    w = e43 / (e43 + e56), v = 1 - w
//   7. otherwise                              the face   s = (va + vb) + vc, (vb / s, vc / s)
// A comparison with a NaN is false, so a NaN operand falls through to the face and gives NaN weights.
// Then q = (v0 + v e1) + w e2, delta = p - q, d2 = (dx dx + dy dy) + dz dz.
// The quotients' operands are selected before the division, so two divisions serve all regions: the
// selected quotient is the one the table names, the same operation on the same operands.
WGT_HD NearestTri nearest_on_tri(f3 p, f3 v0, f3 e1, f3 e2) {
  const f3 ap = p - v0;
  const float d1 = dot(e1, ap), d2 = dot(e2, ap);
  const f3 bp = ap - e1;
  const float d3 = dot(e1, bp), d4 = dot(e2, bp);
  const f3 cp = ap - e2;
  const float d5 = dot(e1, cp), d6 = dot(e2, cp);
  const float vc = d1 * d4 - d3 * d2;
  const float vb = d5 * d2 - d1 * d6;
  const float va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  const bool ra = (d1 <= 0.0f) & (d2 <= 0.0f);
  const bool rb = (d3 >= 0.0f) & (d4 <= d3);
  const bool rab = (vc <= 0.0f) & (d1 >= 0.0f) & (d3 <= 0.0f);
  const bool rc = (d6 >= 0.0f) & (d5 <= d6);
  const bool rac = (vb <= 0.0f) & (d2 >= 0.0f) & (d6 <= 0.0f);
  const bool rbc = (va <= 0.0f) & (e43 >= 0.0f) & (e56 >= 0.0f);
  // the first test that holds: 1..6, else 7
  const int k = ra ? 1 : (rb ? 2 : (rab ? 3 : (rc ? 4 : (rac ? 5 : (rbc ? 6 : 7)))));
  // the region's quotient n / den (edges: the one quotient; the face: v), and the face's second one
  const float num = k == 3 ? d1 : (k == 5 ? d2 : (k == 6 ? e43 : vb));
  const float den = k == 3 ? d1 - d3 : (k == 5 ? d2 - d6 : (k == 6 ? e43 + e56 : (va + vb) + vc));
  const float q1 = num / den, q2 = vc / den;
  NearestTri r;
  r.v = k == 1 ? 0.0f : (k == 2 ? 1.0f : (k == 3 ? q1 : (k == 4 ? 0.0f : (k == 5 ? 0.0f : (k == 6 ? 1.0f - q1 : q1)))));
  r.w = k == 1 ? 0.0f : (k == 2 ? 0.0f : (k == 3 ? 0.0f : (k == 4 ? 1.0f : (k == 5 ? q1 : (k == 6 ? q1 : q2)))));
  r.region = (k == 1 || k == 2 || k == 4) ? kNearVertex : (k == 7 ? kNearFace : kNearEdge);
  r.q = (v0 + r.v * e1) + r.w * e2;
  const f3 dl = p - r.q;
  r.d2 = dot(dl, dl);
  return r;
}

// (d2, id) replaces (best, best_id): d2 < best, or d2 == best and the id is lower; never a NaN (both
// comparisons are false) and never an infinite d2 (best starts at +inf with id kNoHit, and inf is not
// below it).
WGT_HD bool nearest_better(float d2, uint32_t id, float best, uint32_t best_id) {
  return (d2 < __builtin_inff()) & ((d2 < best) | ((d2 == best) & (id < best_id)));
}

// The reported decision, exact: dist < max_dist as an IEEE comparison (a NaN, zero or negative limit
// reports nothing; +inf reports any answer).
WGT_HD bool nearest_reported(uint32_t best_id, float dist, float max_dist) { return (best_id != kNoHit) & (dist < max_dist); }
// ---- culling (the kernel's; the brute force culls nothing) ----------------------------------
// u = 2^-24.  A child box [lo, hi] is culled when its bound lb exceeds the cull bound of the current
// best (or of the radius), with
//   g_a = max(max(lo_a - p_a, p_a - hi_a) - kNearestShrink (hi_a - lo_a), 0) per axis,
//   lb = (gx gx + gy gy) + gz gz,        cull iff lb > min(fl(best F), FLT_MAX),  F = kNearestCullFactor.
// The claim: no triangle below a culled box has a computed d2 <= best.
//
// (1) If the computed closest point q of a triangle lies in the box, then without the shrink lb <= d2
// holds bit for bit, at any magnitude of p: lo_a <= q_a <= hi_a gives p_a - q_a <= p_a - lo_a and
// q_a - p_a <= hi_a - p_a in real numbers, a rounded difference is monotone in its operands, so
// |fl(p_a - q_a)| >= fl(gap_a); squares and sums of non-negative floats are monotone too, and lb and d2
// add their squares in the same order.  p, q and the planes are given floats and each difference
// rounds once, so a far point needs no slack of its own: what p - q loses to ulp(|p|), lo - p loses alike.
//
// (2) So what has to be covered is q outside the triangle's padded box (tri_box), which nests in every
// box above it.  In a vertex region q = v0, v0 + e1 or v0 + e2 up to the rounding of that sum; in an
// edge region the quotient's operands have the signs the region test checked, so 0 <= v, w <= 1 and q
// lies on the edge up to the rounding of (v0 + v e1) + w e2: at most 3 u (|v0_a| + |e1_a| + |e2_a|)
// per axis, far inside the pad's 1e-5 (|lo_a| + |hi_a|) + 1e-4 (hi_a - lo_a) + 1e-6.  Only the face's
// weights can leave the triangle.  There p projects into the triangle (up to the error below), so with
// e the longest edge and r = |p - q| + |e| every |ap|, |bp|, |cp| <= r and every |d_i| <= |e|^2.  A d_i is
// a dot product of an edge with a once-rounded difference: off by at most 5 u |e| r.  va, vb, vc
// are off by at most 20 u |e|^3 r each and their sum s, which is |e1 x e2|^2 = 4 A^2, by 60 u |e|^3 r, so v
// and w are off by at most 80 u |e|^3 r / (4 A^2) = 80 u sigma^2 r / |e|, sigma = |e|^2 / (2 A) the longest edge
// over the height on it, and q on axis a by at most (|e1_a| + |e2_a|) <= 2 (hi_a - lo_a) times that:
//   eta_a <= 160 u sigma^2 (hi_a - lo_a)  +  160 u sigma^2 |p - q|          ((hi_a - lo_a) <= |e|).
// The first term scales with the triangle: the shrink takes it off every box, whose extent is at least
// the triangle's.  The second scales with the DISTANCE, not with |p|: a triangle 1e5 units from a point at
// the origin loses as much as one 1e5 units from a point at 1e5, so a slack on |px| + |py| + |pz| does not
// cover it; a factor on the bound does.  A triangle that can still win has a computed d2 <= best, so
// |p - q|^2 <= best (1 + 3 u); the shrunk box is at most |p - q| + sqrt(3) 160 u sigma^2 |p - q| from p, and
// its computed bound at most (1 + 6 u) that squared (the gaps round three times each, the squares and
// sums as d2's):
//   lb <= best (1 + 9 u) (1 + sqrt(3) 160 u sigma^2)^2.
// The constants are chosen for sigma <= 20 (sigma^2 <= 400: the longest edge up to twenty heights):
//   kNearestShrink = 2^-8 >= 160 u 400 = 3.815e-3 (plus the rounding of the three operations),
//   F = 1 + 2^-6 = 1.015625 >= (1 + 9 u) (1 + sqrt(3) 3.815e-3)^2 = 1.01326, and fl(best F) loses one u more.
// A thinner triangle (a sliver: sigma in the thousands) is outside this premise: its face weights are
// quotients of rounding noise, its q can lie anywhere on its plane, and the brute force alone says
// where.  DESIGN.md §4.13 records what the tests do about such meshes.
// The radius culls the same way: a triangle is reported only if sqrt_rn(d2) < m, hence d2 < m^2 (1 + u)^2,
// and the bound is fl(fl(m m) F); it only culls, the reported decision is nearest_reported.
// Either bound is capped at FLT_MAX: an infinite d2 is never the answer, and the +inf of an empty
// slot (the point box at kEmptySlotCoord: its gap squared overflows) is above the bound whatever best is.
// NaN: p is finite where the kernel culls (kNearestCoordLimit) and the planes are finite, so no g is NaN.
constexpr float kNearestShrink = 0x1p-8f;
constexpr float kNearestCullFactor = 1.0f + 0x1p-6f;
constexpr float kNearestMaxBound = 3.4028234663852886e38f;  // FLT_MAX
WGT_HD float nearest_gap(float lo, float hi, float p) {
  return __builtin_fmaxf(__builtin_fmaxf(lo - p, p - hi) - kNearestShrink * (hi - lo), 0.0f);
}
WGT_HD float nearest_box_bound(float lox, float hix, float loy, float hiy, float loz, float hiz, f3 p) {
  const float gx = nearest_gap(lox, hix, p.x), gy = nearest_gap(loy, hiy, p.y), gz = nearest_gap(loz, hiz, p.z);
  return gx * gx + gy * gy + gz * gz;
}
WGT_HD float nearest_cull_bound(float d2) {
  const float b = d2 * kNearestCullFactor;
  return b < kNearestMaxBound ? b : kNearestMaxBound;
}
// The range outside which the kernel does not cull at all: a point with |px| + |py| + |pz| above 2^40
// (the scene's coordinate limit) scans every record.  Within it and the scene limits every gap is
// below 2^42 and every lb below 2^86: nothing overflows but an empty slot.  A point with a NaN or an
// infinite component has no finite d2 against finite triangles: the miss record at once.
constexpr float kNearestCoordLimit = 0x1p40f;

}  // namespace wgt
