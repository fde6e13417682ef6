// wgt_nearest_k.hip — k-nearest and within-radius closest-point queries on the resident triangle BVH
// (wgt_nearest_k_points), in a translation unit of their own as the other queries are.
//
// Record i = the number of triangles within max_dist[i] of point i and the k nearest of them by
// (d2, primitive id), d2 from nearest_on_tri on the resident record (wgt_nearest.h); wgt_nearest_k.h
// states the definition, which the host's brute force wgt_nearest_k_points_spec evaluates too.  Every
// triangle's d2 is computed per triangle, whatever the order, and membership and the list's order are
// exact comparisons on it, so the traversal answers what the brute force answers as long as it culls
// only boxes that hold no triangle that could still be counted or enter the list.
//
// The cull is k_nearest's (wgt_nearest.h proves it): a child box is dropped when its bound lb exceeds
// nearest_cull_bound(best), and then no triangle below it has a computed d2 <= best.
//   Count form: best = fl(m m) throughout.  A member has sqrt_rn(d2) < m, hence d2 < m^2 (1 + u)^2, which
//   the radius' bound covers as it does for k_nearest: no member lies below a dropped box, so every member
//   is tested, counted and offered to the list.
//   Cull form: the list keeps the first k of ALL triangles with a finite d2 by (d2, id); S is a prefix of
//   that order, so its first k are the list's entries whose root is below the radius, decided at the
//   write-out.  Until the list is full the bound is the radius' (a triangle outside the radius is in no
//   answer); from then it is min(radius', nearest_cull_bound(D)), D the k-th d2 of that moment, re-read
//   after every insertion.  A later triangle enters only with (d2, id) < (D, id_k), which needs d2 <= D:
//   the proof's case with best := D.  A box dropped under an earlier, larger D stays dropped rightly: D
//   only shrinks.
// Outside |px| + |py| + |pz| <= 2^40 nothing is culled: the lane scans every record, the definition verbatim.
//
// The form is k_nearest's: one point per lane, kBlock lanes per workgroup, the per-lane LDS stack, one
// node or one triangle per step, nearest_box_bound keys on the children, trav_next as the tail.  The
// lane's list lives in LDS behind the stack (nearest_k_lds_bytes): k d2s, then k ids, then (when pos or
// uv is asked for) k record offsets, at stride kBlock, so a lane's column never meets another's bank.
// The write-out after the traversal is planar, one coalesced store per plane and field; pos and uv are
// recomputed from the entry's record, as k_nearest recomputes its winner's.
#include "wgt_nearest_k.h"
#include "wgt_trav.h"

namespace wgt {

namespace {

__device__ __forceinline__ uint32_t nk_key(float lb, float cb) { return lb <= cb ? __float_as_uint(lb) : kMissKey; }

// The lane's list: entry j's d2 at list[j * kBlock], its id at list[(k + j) * kBlock] and, with REC, its
// record's byte offset at list[(2 k + j) * kBlock], j < len <= k, ascending by (d2, id).  Inserts
// (d2, id, rec) if it belongs among the first k; every index written is at most k - 1.
template <bool REC>
__device__ __forceinline__ void nk_insert(int* __restrict__ list, uint32_t k, uint32_t& len, float d2, uint32_t id,
                                          uint32_t rec) {
  if (k == 0) return;
  uint32_t j = len;
  if (len == k) {
    j = k - 1;
    if (!nearest_k_less(d2, id, __int_as_float(list[j * kBlock]), (uint32_t)list[(k + j) * kBlock])) return;
  } else {
    ++len;
  }
  while (j > 0) {
    const int D = list[(j - 1) * kBlock], I = list[(k + j - 1) * kBlock];
    if (!nearest_k_less(d2, id, __int_as_float(D), (uint32_t)I)) break;
    list[j * kBlock] = D;
    list[(k + j) * kBlock] = I;
    if (REC) list[(2 * k + j) * kBlock] = list[(2 * k + j - 1) * kBlock];
    --j;
  }
  list[j * kBlock] = __float_as_int(d2);
  list[(k + j) * kBlock] = (int)id;
  if (REC) list[(2 * k + j) * kBlock] = (int)rec;
}

// TRIS: the scene has triangles.  CULL: NearestKMode kNearestKCull, else kNearestKCount.  REC: pos or uv is
// asked for (the list's third plane).  STATS: the counting instantiation (wgt_nearest_k_points_stats) adds
// its lanes' node visits and triangle tests to counts[0] and counts[1].
template <bool TRIS, bool CULL, bool REC, bool STATS>
__global__ void __launch_bounds__(kBlock)
k_nearest_k(DevScene sc, NearestKPlan pl, const float* __restrict__ points, const float* __restrict__ max_dist,
            wgt_nearest_k_buffers out, unsigned long long* __restrict__ counts) {
  extern __shared__ int s_mem[];  // sc.stack entries per lane, then pl.words * pl.k list words per lane
  int* lds = s_mem + threadIdx.x;
  int* list = s_mem + sc.stack * kBlock + threadIdx.x;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const size_t n = pl.n;
  if (i >= pl.n) return;
  const uint32_t k = pl.k;
  const f3 p = f3{points[i], points[n + i], points[2 * n + i]};
  const float inf = __builtin_inff();
  const float m = max_dist ? max_dist[i] : inf;
  const float l1 = fabs_w(p.x) + fabs_w(p.y) + fabs_w(p.z);
  uint32_t cnt = 0, len = 0, n_nodes = 0, n_tests = 0;
  // no distance is below a radius that is zero, negative or NaN; a NaN or infinite point has no finite d2
  if (TRIS && m > 0.0f && l1 < inf) {
    // the radius' bound, and the current one: min(radius', the k-th d2's) once the list is full
    const float cbm = nearest_cull_bound(m * m);
    float cb = cbm;
    Trav t;
    t.ref = 0;
    t.lf = t.le = 0;
    t.sp = 0;
    // beyond the range the cull is derived for: every record, as one leaf range
    if (!(l1 <= kNearestCoordLimit)) t.le = sc.n_tris * kTriRecordBytes;
    for (;;) {
      bool pop;
      int next = 0;
      if (t.lf < t.le) {
        if (STATS) ++n_tests;
        const float4* __restrict__ r = (const float4*)((const char*)sc.tris + t.lf);
        const float4 A = r[0], B = r[1], C = r[2];
        const uint32_t idx = __float_as_uint(A.w);
        const float d2 = nearest_on_tri(p, xyz(A), xyz(B), xyz(C)).d2;
        if (CULL) {
          if (d2 < inf) {
            nk_insert<REC>(list, k, len, d2, idx, t.lf);
            if (len == k) cb = __builtin_fminf(cbm, nearest_cull_bound(__int_as_float(list[(k - 1) * kBlock])));
          }
        } else if (nearest_k_member(d2, m)) {
          ++cnt;
          nk_insert<REC>(list, k, len, d2, idx, t.lf);
        }
        t.lf += kTriRecordBytes;
        if (t.lf < t.le) continue;
        pop = true;
      } else {
        if (STATS) ++n_nodes;
        const float4* __restrict__ nd = (const float4*)((const char*)sc.nodes + (uint32_t)t.ref);  // ref: byte offset
        const float4 lx = nd[0], hx = nd[1], ly = nd[2], hy = nd[3], lz = nd[4], hz = nd[5];
        const float4 rf = nd[6];
        int r0 = __float_as_int(rf.x), r1 = __float_as_int(rf.y), r2 = __float_as_int(rf.z), r3 = __float_as_int(rf.w);
        uint32_t k0 = nk_key(nearest_box_bound(lx.x, hx.x, ly.x, hy.x, lz.x, hz.x, p), cb);
        uint32_t k1 = nk_key(nearest_box_bound(lx.y, hx.y, ly.y, hy.y, lz.y, hz.y, p), cb);
        uint32_t k2 = nk_key(nearest_box_bound(lx.z, hx.z, ly.z, hy.z, lz.z, hz.z, p), cb);
        uint32_t k3 = nk_key(nearest_box_bound(lx.w, hx.w, ly.w, hy.w, lz.w, hz.w, p), cb);
        if (CULL || pl.sort) {
          // k_nearest's node step: nearest child first, so the list fills with near triangles and the
          // bound shrinks early; a write for a dropped child lands above the top and is overwritten or
          // never read (trav_step)
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
          // occ_step's node step, for the count alone: the bound never changes, so the answer and the visits
          // do not depend on the order of descent, and the builder's stack bound holds for any order.  With
          // a list the plan asks for the sorted step (pl.sort): near triangles first reach the insertion
          // in nearly ascending order, which shifts least
          const bool h0 = k0 != kMissKey, h1 = k1 != kMissKey, h2 = k2 != kMissKey, h3 = k3 != kMissKey;
          const bool p1 = h0, p2 = h0 || h1, p3 = p2 || h2;  // an earlier slot is kept: this one is pushed
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
  if (STATS) {
    atomicAdd(&counts[0], (unsigned long long)n_nodes);
    atomicAdd(&counts[1], (unsigned long long)n_tests);
  }
  if (out.count) out.count[i] = cnt;
  const uint32_t nlq = sc.n_lights + sc.n_quads;
  for (uint32_t j = 0; j < k; ++j) {
    // the count form's entries are members already; the cull form's are cut at the radius here (S is a
    // prefix of the list's order)
    const float d2 = j < len ? __int_as_float(list[j * kBlock]) : inf;
    const float dist = sqrt_rn(d2);
    const bool have = (j < len) & (dist < m);
    if (out.prim) out.prim[j * n + i] = have ? nlq + (uint32_t)list[(k + j) * kBlock] : kNoHit;
    if (out.dist) out.dist[j * n + i] = have ? dist : inf;
    if (REC) {
      NearestTri c{};
      if (have) {
        const float4* __restrict__ r = (const float4*)((const char*)sc.tris + (uint32_t)list[(2 * k + j) * kBlock]);
        c = nearest_on_tri(p, xyz(r[0]), xyz(r[1]), xyz(r[2]));
      }
      if (out.pos) {
        out.pos[(3 * j + 0) * n + i] = have ? c.q.x : 0.0f;
        out.pos[(3 * j + 1) * n + i] = have ? c.q.y : 0.0f;
        out.pos[(3 * j + 2) * n + i] = have ? c.q.z : 0.0f;
      }
      if (out.uv) {
        out.uv[(2 * j + 0) * n + i] = have ? c.v : 0.0f;
        out.uv[(2 * j + 1) * n + i] = have ? c.w : 0.0f;
      }
    }
  }
}

template <bool REC, bool STATS>
hipError_t launch(const DevScene& sc, const NearestKPlan& p, const float* d_points, const float* d_max_dist,
                  const wgt_nearest_k_buffers& out, unsigned long long* d_counts, hipStream_t stream) {
  const dim3 grid((p.n + kBlock - 1) / kBlock), block(kBlock);
  // without triangles there is no traversal, so no mode
  (sc.n_tris == 0             ? k_nearest_k<false, false, REC, STATS>
   : p.mode == kNearestKCount ? k_nearest_k<true, false, REC, STATS>
                              : k_nearest_k<true, true, REC, STATS>)
      <<<grid, block, p.lds, stream>>>(sc, p, d_points, d_max_dist, out, d_counts);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_nearest_k(const DevScene& sc, const NearestKPlan& p, const float* d_points, const float* d_max_dist,
                            const wgt_nearest_k_buffers& out, unsigned long long* d_counts, hipStream_t stream) {
  if (p.n == 0) return hipSuccess;
  // the kernel's list and stack indices stay within what the plan sized (the cull form reads entry k - 1,
  // a pos or uv write-out the third plane)
  const bool rec = out.pos || out.uv;
  if (p.k > WGT_NEAREST_MAX_K || p.mode > kNearestKCull || (p.k == 0 && p.mode == kNearestKCull) ||
      p.words != (rec ? 3u : 2u) || p.lds != nearest_k_lds_bytes(sc.stack, p.k, p.words) ||
      p.lds > kNearestKLdsPerWorkgroup)
    return hipErrorInvalidValue;
  if (p.k == 0 && (out.prim || out.dist || rec)) return hipErrorInvalidValue;
  if (rec)
    return d_counts ? launch<true, true>(sc, p, d_points, d_max_dist, out, d_counts, stream)
                    : launch<true, false>(sc, p, d_points, d_max_dist, out, nullptr, stream);
  return d_counts ? launch<false, true>(sc, p, d_points, d_max_dist, out, d_counts, stream)
                  : launch<false, false>(sc, p, d_points, d_max_dist, out, nullptr, stream);
}

}  // namespace wgt
