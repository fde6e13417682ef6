// wgt_multihit.hip — multi-hit ray queries (wgt_trace_multi_hits): the k nearest hits
// of each caller ray and the number of all its hits below a per-ray distance limit, in a translation
// unit of their own as the other queries are.
//
// A primitive is hit by ray i when the closest-hit code accepts it tested alone (isect_quad<true>,
// tri_test<false> with its own-box check and bi = kNoHit, isect_sphere) at a distance dist with
// dist < min(max_dist[i], kRayMax).  Every primitive's accept decision and distance are computed per
// primitive, whatever the scan or traversal order, so the set S of hit primitives needs
// no minimum over primitives and does not depend on the order either: count = |S|, and the list holds
// the first k elements of S by (dist, primitive id), a total order.  The BVH, the limit and the k-th
// distance only cull; membership and order always come from the exact comparisons.
//
// The form is k_occluded's: one ray per lane, kBlock lanes per workgroup, 128-B nodes, the per-lane
// stack of sc.stack entries in LDS, one node or one triangle per step with trav_next as the tail.  The
// lane's sorted list lives in LDS behind the stack (multi_hit_lds_bytes): k distances, then k ids, at
// stride kBlock, so a lane's column never meets another's bank; insertion shifts within the column, and
// the write-out after the traversal is planar, one coalesced store per plane and field.
#include "wgt_multihit.h"
#include "wgt_trav.h"

namespace wgt {

namespace {

// The bound on the ray parameter of every primitive accepted with ray_dist < m: occ_t_hi of
// wgt_occlusion.hip, whose comment derives it (the absolute term in |o|, the factor 1 + 2^-19, the range
// it is derived for; kRayMax outside it).  Restated here because that translation unit keeps it local.
__device__ __forceinline__ float mh_t_hi(float l1, float nd, float m) {
  const bool covered = l1 <= 0x1p40f && nd >= 0x1p-40f && nd <= 0x1p40f && m <= 0x1p40f;
  const float slack = 0x1p-22f * l1 + 0x1p-60f;
  const float q = ((m + slack) / nd) * (1.0f + 0x1p-19f);
  return covered ? __builtin_fminf(q, kRayMax) : kRayMax;
}
// The bound once the list is full with k-th distance D (a number, 0 <= D < kRayMax): a later primitive
// enters the list iff (dist, id) < (D, id_k), which needs dist <= D, that is dist < the float above D.
// The bound therefore still admits a hit with dist == D and a lower id.
__device__ __forceinline__ float mh_t_full(float l1, float nd, float D) {
  return mh_t_hi(l1, nd, __uint_as_float(__float_as_uint(D) + 1u));
}

// One quad or sphere tested alone against the limit, as occ_quad / occ_sphere: the reference's accept
// code with the limit as the distance to beat.  A NaN distance is below nothing: not a hit.
__device__ __forceinline__ bool mh_quad(f3 o, f3 d, const float4* __restrict__ q, float lim, float& dist) {
  Hit h;
  h.dist = lim;
  h.prim = kNoHit;
  float qt = __builtin_inff();
  isect_quad<true>(o, d, q, 0u, h, qt);
  dist = h.dist;
  return h.prim != kNoHit && h.dist < lim;
}
__device__ __forceinline__ bool mh_sphere(f3 o, f3 d, const float4* __restrict__ s, float lim, float& dist) {
  Hit h;
  h.dist = lim;
  h.prim = kNoHit;
  isect_sphere(o, d, s, 0u, h);
  dist = h.dist;
  return h.prim != kNoHit && h.dist < lim;
}

__device__ __forceinline__ bool mh_less(float da, uint32_t pa, float db, uint32_t pb) {
  return (da < db) | ((da == db) & (pa < pb));
}

// The lane's list: entry j's distance at list[j * kBlock], its id at list[(k + j) * kBlock], j < len <= k,
// ascending by (dist, id).  Inserts (dist, prim) if it belongs among the first k; every index written
// is at most k - 1.
__device__ __forceinline__ void mh_insert(int* __restrict__ list, uint32_t k, uint32_t& len, float dist,
                                          uint32_t prim) {
  if (k == 0) return;
  uint32_t j = len;
  if (len == k) {
    j = k - 1;
    if (!mh_less(dist, prim, __int_as_float(list[j * kBlock]), (uint32_t)list[(k + j) * kBlock])) return;
  } else {
    ++len;
  }
  while (j > 0) {
    const int D = list[(j - 1) * kBlock], P = list[(k + j - 1) * kBlock];
    if (!mh_less(dist, prim, __int_as_float(D), (uint32_t)P)) break;
    list[j * kBlock] = D;
    list[(k + j) * kBlock] = P;
    --j;
  }
  list[j * kBlock] = __float_as_int(dist);
  list[(k + j) * kBlock] = (int)prim;
}

// TRIS: the scene has triangles.  CULL: MultiHitMode kMultiHitCull, else kMultiHitCount.  STATS: the counting
// instantiation (wgt_trace_multi_hits_stats) adds its lanes' node visits and triangle tests to counts[0]
// and counts[1].
template <bool TRIS, bool CULL, bool STATS>
__global__ void __launch_bounds__(kBlock)
k_multi_hit(DevScene sc, MultiHitPlan p, const float* __restrict__ rays, const float* __restrict__ max_dist,
            wgt_multi_hit_buffers out, unsigned long long* __restrict__ counts) {
  extern __shared__ int s_mem[];  // sc.stack entries per lane, then 2 * p.k list words per lane
  int* lds = s_mem + threadIdx.x;
  int* list = s_mem + sc.stack * kBlock + threadIdx.x;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const size_t n = p.n;
  if (i >= p.n) return;
  const uint32_t k = p.k;
  const f3 o = f3{rays[i], rays[n + i], rays[2 * n + i]};
  const f3 d = f3{rays[3 * n + i], rays[4 * n + i], rays[5 * n + i]};
  const float inf = __builtin_inff();
  const float m = max_dist ? max_dist[i] : inf;
  // a ray with a NaN or infinite component hits nothing, by definition
  const bool finite = fabs_w(o.x) < inf && fabs_w(o.y) < inf && fabs_w(o.z) < inf && fabs_w(d.x) < inf &&
                      fabs_w(d.y) < inf && fabs_w(d.z) < inf;
  uint32_t cnt = 0, len = 0, n_nodes = 0, n_tests = 0;
  // ray_dist is never negative: no distance is below a limit that is zero, negative or NaN
  if (finite && m > 0.0f) {
    const float lim = __builtin_fminf(m, kRayMax);  // the reference accepts ray_dist < kRayMax only (hit_init)
    const uint32_t nlq = sc.n_lights + sc.n_quads;
    float dist;
    if (!p.tris_only) {
      for (uint32_t q = 0; q < nlq; ++q)
        if (mh_quad(o, d, sc.quads + 6 * q, lim, dist)) {
          ++cnt;
          mh_insert(list, k, len, dist, q);
        }
      for (uint32_t s = 0; s < sc.n_spheres; ++s)
        if (mh_sphere(o, d, sc.spheres + 2 * s, lim, dist)) {
          ++cnt;
          mh_insert(list, k, len, dist, nlq + sc.n_tris + s);
        }
    }
    if (TRIS) {
      const float l1 = fabs_w(o.x) + fabs_w(o.y) + fabs_w(o.z), nd = length(d);
      Trav t;
      trav_init<0, true>(sc, o, d, false, 0.0f, t);
      t.bt = mh_t_hi(l1, nd, m);
      // the scans may have filled the list already
      if (CULL && len == k) t.bt = mh_t_full(l1, nd, __int_as_float(list[(k - 1) * kBlock]));
      for (;;) {
        bool pop;
        int next = 0;
        if (t.lf < t.le) {
          if (STATS) ++n_tests;
          float tt;
          uint32_t idx;
          // accepted exactly as trav_step accepts it alone (bi = kNoHit: t <= bt, and bt only culls), then
          // the exact decision on its distance
          if (tri_test<false>(sc.tris, t.lf, o, d, t.ot, t.inv, t.bt, kNoHit, tt, idx)) {
            dist = distance(o + tt * d, o);
            if (dist < lim) {
              ++cnt;
              mh_insert(list, k, len, dist, nlq + idx);
              if (CULL && len == k) t.bt = mh_t_full(l1, nd, __int_as_float(list[(k - 1) * kBlock]));
            }
          }
          t.lf += kTriRecordBytes;
          if (t.lf < t.le) continue;
          pop = true;
        } else {
          if (STATS) ++n_nodes;
          uint32_t k0, k1, k2, k3;
          int r0, r1, r2, r3;
          node_keys<0>(sc, t, t.ref, k0, k1, k2, k3, r0, r1, r2, r3);
          if (CULL) {
            // trav_step's node step: nearest child first, so the list fills with near hits and the bound
            // shrinks early
            cas(k0, r0, k1, r1);
            cas(k2, r2, k3, r3);
            cas(k0, r0, k2, r2);
            cas(k1, r1, k3, r3);
            cas(k1, r1, k2, r2);
            lds[t.sp * kBlock] = r3;
            t.sp += k3 != kMissKey ? 1 : 0;
            lds[t.sp * kBlock] = r2;
            t.sp += k2 != kMissKey ? 1 : 0;
            lds[t.sp * kBlock] = r1;
            t.sp += k1 != kMissKey ? 1 : 0;
            next = r0;
            pop = k0 == kMissKey;
          } else {
            // occ_step's node step: the answer does not depend on the order of descent, and its stack
            // bound holds for any order
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
        }
        if (trav_next(t, lds, pop, next)) break;
      }
    }
  }
  if (STATS) {
    atomicAdd(&counts[0], (unsigned long long)n_nodes);
    atomicAdd(&counts[1], (unsigned long long)n_tests);
  }
  if (out.count) out.count[i] = cnt;
  for (uint32_t j = 0; j < k; ++j) {
    const bool have = j < len;
    if (out.prim) out.prim[j * n + i] = have ? (uint32_t)list[(k + j) * kBlock] : kNoHit;
    if (out.dist) out.dist[j * n + i] = have ? __int_as_float(list[j * kBlock]) : inf;
  }
}

template <bool STATS>
hipError_t launch(const DevScene& sc, const MultiHitPlan& p, const float* d_rays, const float* d_max_dist,
                  const wgt_multi_hit_buffers& out, unsigned long long* d_counts, hipStream_t stream) {
  const dim3 grid((p.n + kBlock - 1) / kBlock), block(kBlock);
  // without triangles there is no traversal, so no mode
  (sc.n_tris == 0              ? k_multi_hit<false, false, STATS>
   : p.mode == kMultiHitCount ? k_multi_hit<true, false, STATS>
                              : k_multi_hit<true, true, STATS>)
      <<<grid, block, p.lds, stream>>>(sc, p, d_rays, d_max_dist, out, d_counts);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_multi_hit(const DevScene& sc, const MultiHitPlan& p, const float* d_rays, const float* d_max_dist,
                            const wgt_multi_hit_buffers& out, unsigned long long* d_counts, hipStream_t stream) {
  if (p.n == 0) return hipSuccess;
  // the kernel's list and stack indices stay within what the plan sized
  // (a cull form reads entry k - 1)
  if (p.k > WGT_MULTI_HIT_MAX_K || p.mode > kMultiHitCull || (p.k == 0 && p.mode == kMultiHitCull) ||
      p.lds != multi_hit_lds_bytes(sc.stack, p.k) || p.lds > kLdsPerWorkgroup)
    return hipErrorInvalidValue;
  return d_counts ? launch<true>(sc, p, d_rays, d_max_dist, out, d_counts, stream)
                  : launch<false>(sc, p, d_rays, d_max_dist, out, nullptr, stream);
}

}  // namespace wgt
