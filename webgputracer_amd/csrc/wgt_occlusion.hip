// wgt_occlusion.hip — occlusion (any-hit) queries on caller-supplied rays with a per-ray
// distance limit (wgt_occluded_rays), in a translation unit of their own,
// away from the render kernels and their register budgets.
//
// occluded[i] = 1 iff the closest-hit query (closest_hit, wgt_trav.h) on ray i returns a primitive and a
// distance below max_dist[i].  The closest hit's distance is the minimum of ray_dist over
// the accepted primitives, and every primitive's accept decision and ray_dist are computed
// per primitive, whatever the scan or traversal order, so "some accepted primitive has
// ray_dist < max_dist" is the same statement as long as
//   (a) each primitive is tested by the code closest_hit tests it with (isect_quad<true>,
//       tri_test<false> with its own-box check, isect_sphere, the IEEE safe_inv), and
//   (b) culling is conservative (the node boxes' nesting, and t_hi below).
// A lane therefore stops at the first such primitive, a node step has no sorting network,
// and the distance limit culls the tree.
//
// The minimum argument needs every ray_dist to be a number: a NaN distance makes the
// reference accept whatever it scans next, so its answer depends on the scan order.  A
// ray with a NaN or infinite component, and a ray for which a quad or sphere yields a NaN
// distance (a quad with a NaN normal, an overflowing sphere discriminant), is answered by
// the closest-hit code itself (closest_hit) in its lane: the definition, verbatim.  A
// triangle never yields a NaN distance for a finite ray (its accepted t is finite, so
// o + t d - o is finite or infinite).
#include "wgt_hit.h"
#include "wgt_trav.h"

namespace wgt {

namespace {

// The bound t_hi on the ray parameter: every primitive accepted at parameter t >= kRayMin
// with ray_dist < m has t <= t_hi.  For a triangle t is the hit parameter of the spec, the
// Moller-Trumbore t clamped to the triangle's own slab interval (tri_test_rec): that is the
// t its ray_dist is computed from, and tri_test_rec compares that t with the bound, so the
// derivation below never sees the unclamped value.  The clamped t lies in the triangle's
// interval, hence in every ancestor's, so a node entered beyond t_hi still holds no
// triangle with t <= t_hi.
//
// ray_dist = fl(sqrt(fl(v . v))), v_i = fl(fl(o_i + fl(t d_i)) - o_i).  With u = 2^-24 and
// every operation rounding by a factor within 1 +- u:
//   v_i - t d_i = t d_i ((1 + e1)(1 + e2)(1 + e3) - 1) + e2 (1 + e3) o_i, so
//   ||v - t d|| <= 3.001 u t ||d|| + 1.0001 u ||o||  and  ||v|| >= t ||d|| (1 - 3.001 u) - 1.0001 u ||o||:
// the ABSOLUTE term in ||o|| is what the rounding of o + t d loses when the origin is far
// from the hit, and why m / ||d|| alone is wrong.  The dot product and the square root lose
// another factor (1 - 3 u); products that underflow (t d_i, v_i^2) lose at most 2^-62 of the
// result in absolute terms.  Hence
//   ray_dist >= t ||d|| (1 - 6.01 u) - 1.0001 u ||o|| - 2^-62, and ray_dist < m gives
//   t < (m + 1.0001 u ||o|| + 2^-62) / (||d|| (1 - 6.01 u)).
// Computed in fp32: l1 = |o_x| + |o_y| + |o_z| >= ||o|| (1 - 2 u), slack = 2^-22 l1 + 2^-60 (4 u
// against the 1.0001 u needed), nd = fl(||d||) <= ||d|| (1 + 3 u), and the quotient (m + slack) / nd
// rounds twice more: at least (m + slack) / ||d|| (1 - 6 u); the factor 1 + 2^-19 (32 u) covers
// these and the 6.01 u above with room to spare, and costs the cull nothing measurable.
// The derivation holds while nothing overflows and nd is a normal number well inside the
// range: l1 <= 2^40, 2^-40 <= nd <= 2^40, m <= 2^40 (then every term stays below 2^82).  Any
// other ray (an infinite limit among them) takes t_hi = kRayMax, which bounds every accepted
// t by the accept test itself.  t_hi only culls: the answer always comes from the exact
// comparison ray_dist < m.
__device__ __forceinline__ float occ_t_hi(float l1, float nd, float m) {
  const bool covered = l1 <= 0x1p40f && nd >= 0x1p-40f && nd <= 0x1p40f && m <= 0x1p40f;
  const float slack = 0x1p-22f * l1 + 0x1p-60f;
  const float q = ((m + slack) / nd) * (1.0f + 0x1p-19f);
  return covered ? __builtin_fminf(q, kRayMax) : kRayMax;
}

// One quad or sphere, tested alone against the limit: the reference's own accept code with
// the limit as the distance to beat.  `nan` reports a hit accepted with a NaN distance.
__device__ __forceinline__ bool occ_quad(f3 o, f3 d, const float4* __restrict__ q, float lim, bool& nan) {
  Hit h;
  h.dist = lim;
  h.prim = kNoHit;
  float qt = __builtin_inff();
  isect_quad<true>(o, d, q, 0u, h, qt);
  nan = nan || (h.prim != kNoHit && h.dist != h.dist);
  return h.prim != kNoHit && h.dist < lim;
}
__device__ __forceinline__ bool occ_sphere(f3 o, f3 d, const float4* __restrict__ s, float lim, bool& nan) {
  Hit h;
  h.dist = lim;
  h.prim = kNoHit;
  isect_sphere(o, d, s, 0u, h);
  nan = nan || (h.prim != kNoHit && h.dist != h.dist);
  return h.prim != kNoHit && h.dist < lim;
}

// Starts ray i: the limit's trivial cases, the fallback rays, the quad and sphere scans
// (scalar loads: the records are wave-uniform), then the traversal's initial state with
// t_hi as its bound.  Returns true when the lane has a traversal to run; otherwise the
// answer is written.
template <bool TRIS>
__device__ __forceinline__ bool occ_start(const DevScene& sc, const float* __restrict__ rays,
                                          const float* __restrict__ max_dist, uint32_t n, uint32_t i,
                                          uint8_t* __restrict__ out, int* __restrict__ lds, f3& o, f3& d,
                                          float& lim, Trav& t) {
  o = f3{rays[i], rays[(size_t)n + i], rays[2 * (size_t)n + i]};
  d = f3{rays[3 * (size_t)n + i], rays[4 * (size_t)n + i], rays[5 * (size_t)n + i]};
  const float m = max_dist[i];
  // ray_dist is never negative: no distance is below a limit that is zero, negative or NaN
  if (!(m > 0.0f)) {
    out[i] = 0;
    return false;
  }
  // the reference accepts ray_dist < kRayMax only (hit_init)
  lim = __builtin_fminf(m, kRayMax);
  const float l1 = fabs_w(o.x) + fabs_w(o.y) + fabs_w(o.z), nd = length(d);
  const float inf = __builtin_inff();
  bool fallback = !(l1 < inf && nd < inf);  // a NaN or infinite component (or an overflowing norm)
  bool occ = false;
  if (!fallback) {
    const uint32_t nlq = sc.n_lights + sc.n_quads;
    for (uint32_t k = 0; k < nlq; ++k) occ = occ_quad(o, d, sc.quads + 6 * k, lim, fallback) || occ;
    for (uint32_t k = 0; k < sc.n_spheres; ++k) occ = occ_sphere(o, d, sc.spheres + 2 * k, lim, fallback) || occ;
  }
  if (fallback) {
    Hit h;
    closest_hit<TRIS, true>(sc, o, d, lds, h);
    out[i] = (h.prim != kNoHit && h.dist < m) ? 1 : 0;
    return false;
  }
  if (occ || !TRIS) {
    out[i] = occ ? 1 : 0;
    return false;
  }
  trav_init<0, true>(sc, o, d, false, 0.0f, t);
  t.bt = occ_t_hi(l1, nd, m);
  return true;
}

// One BVH4 node OR one triangle per call, as trav_step; the result does not depend on the
// order of descent, so the node step sorts nothing: it descends into the first hit child
// (slot order) and pushes the other hit ones.  The builder's stack bound (bvh.cpp: (children
// - 1) per node on a root-to-node path, maximised over the paths) holds for ANY descent
// order: the entries on the stack are always unvisited siblings of the nodes on the current
// root-to-node path, at most (children - 1) per such node, whichever child was entered
// first.  As in trav_step a write for a missed child lands at the top, which stays within
// DevScene::stack (the bound + 1).
// Returns 0: go on, 1: occluded, 2: the traversal ended without a hit below the limit.
__device__ __forceinline__ int occ_step(const DevScene& sc, f3 o, f3 d, float lim, Trav& t,
                                        int* __restrict__ lds) {
  bool pop;
  int next = 0;
  if (t.lf < t.le) {
    float tt;
    uint32_t idx;
    // accepted exactly as trav_step accepts it (bi = kNoHit: t <= bt = t_hi), then the exact decision
    if (tri_test<false>(sc.tris, t.lf, o, d, t.ot, t.inv, t.bt, kNoHit, tt, idx)) {
      if (distance(o + tt * d, o) < lim) return 1;
    }
    t.lf += kTriRecordBytes;
    if (t.lf < t.le) return 0;
    pop = true;
  } else {
    uint32_t k0, k1, k2, k3;
    int r0, r1, r2, r3;
    node_keys<0>(sc, t, t.ref, k0, k1, k2, k3, r0, r1, r2, r3);
    const bool h0 = k0 != kMissKey, h1 = k1 != kMissKey, h2 = k2 != kMissKey, h3 = k3 != kMissKey;
    const bool p1 = h0, p2 = h0 || h1, p3 = p2 || h2;  // an earlier slot is hit: this one is pushed
    lds[t.sp * kBlock] = r3;
    t.sp += (h3 && p3) ? 1 : 0;
    lds[t.sp * kBlock] = r2;
    t.sp += (h2 && p2) ? 1 : 0;
    lds[t.sp * kBlock] = r1;
    t.sp += (h1 && p1) ? 1 : 0;
    next = h0 ? r0 : (h1 ? r1 : (h2 ? r2 : r3));
    pop = !(p3 || h3);
  }
  return trav_next(t, lds, pop, next) ? 2 : 0;
}

// Launch lane i runs ray i (the flat form, as k_trace_hits): each answer depends on its ray alone.
// A persistent form (a resident grid whose lanes refill from a launch-wide ray queue by ballot /
// mbcnt, as k_render_ps refills pixels) was built and measured against this one and removed: it
// was 1.4 to 5 times slower on every workload at every setting tried.
template <bool TRIS>
__global__ void __launch_bounds__(kBlock)
k_occluded(DevScene sc, const float* __restrict__ rays, const float* __restrict__ max_dist, uint32_t n,
           uint8_t* __restrict__ out) {
  extern __shared__ int s_stack[];  // sc.stack entries per lane (stack_lds_bytes)
  int* lds = s_stack + threadIdx.x;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  f3 o, d;
  float lim;
  Trav t;
  if (!occ_start<TRIS>(sc, rays, max_dist, n, i, out, lds, o, d, lim, t)) return;
  if (TRIS) {
    int r;
    while ((r = occ_step(sc, o, d, lim, t, lds)) == 0) {
    }
    out[i] = r == 1 ? 1 : 0;
  }
}

}  // namespace

hipError_t launch_occluded(const DevScene& sc, const float* d_rays, const float* d_max_dist, uint32_t n,
                           uint8_t* d_out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
  (sc.n_tris > 0 ? k_occluded<true> : k_occluded<false>)
      <<<grid, block, stack_lds_bytes(sc.stack), stream>>>(sc, d_rays, d_max_dist, n, d_out);
  return hipGetLastError();
}

}  // namespace wgt
