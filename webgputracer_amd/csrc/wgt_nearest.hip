// wgt_nearest.hip — closest-point queries on the resident triangle BVH (wgt_nearest_points,
// DESIGN.md §4.13), in a translation unit of their own as the other queries are.
//
// Record i = the triangle nearest to point i: the minimum of (d2, primitive id) over the scene's
// triangles, d2 from nearest_on_tri on the resident record's v0, e1, e2 (wgt_nearest.h, the one
// statement the host's brute force wgt_nearest_points_spec evaluates too), reported iff
// sqrt_rn(d2) < max_dist[i].  Every triangle's d2 is computed per triangle, whatever the order, and
// the minimum with its tie rule does not depend on the order either, so the traversal answers what
// the brute force answers as long as it culls only boxes that hold no triangle that could still win.
//
// The culling argument (wgt_nearest.h states it operation by operation).  A child box's bound lb is
// computed from the same rounded differences and squares as d2, so lb <= d2 holds bit for bit for
// every triangle whose computed closest point q lies in the box, at any magnitude of p: rounding is
// monotone and p, q and the box planes are given floats.  tri_box's pad keeps q in the triangle's own
// box, which nests in every box above it, for the vertex and edge regions (their weights are in
// [0, 1] by the signs the region tests checked).  The face's weights can leave the triangle: the dot
// products of the region tests lose 5 u |e| (|p - q| + |e|), which moves q by up to 160 u sigma^2 times the
// triangle's extent plus 160 u sigma^2 |p - q| (sigma: longest edge over the height on it).  The first part
// is taken off every box (each gap shrinks by 2^-8 of the box's extent, nearest_gap); the second scales
// with the DISTANCE, not with |p| (a slack on |px| + |py| + |pz| would not cover a triangle 1e5 units from a
// point at the origin), so it is a factor on the bound: a box is culled when lb > best (1 + 2^-6)
// (nearest_cull_bound).  Both constants hold for sigma <= 20.  The radius culls with fl(m m) (1 + 2^-6),
// derived the same way; the reported decision is always the exact dist < max_dist.  Outside
// |px| + |py| + |pz| <= 2^40 nothing is culled: the lane scans every record, the definition verbatim.
//
// The form is k_occluded's: one query per lane, kBlock lanes per workgroup, the per-lane LDS stack of
// stack_lds_bytes(sc.stack), one node or one triangle per step, leaves opened as ranges (trav_next).
// A node step sorts its four (lb, ref) pairs by the bounds' bits (non-negative floats order as
// unsigned) with the five-cas network, descends into the nearest and pushes the others farthest first;
// a child with lb above the bound gets kMissKey and is dropped, an empty slot (lb = +inf) among them.
// The stack keeps refs only: a popped node's children are tested against the bound of that moment.
// The builder's stack bound holds for any descent order (occ_step's comment, wgt_occlusion.hip).
#include "wgt_nearest.h"
#include "wgt_trav.h"

namespace wgt {

namespace {

__device__ __forceinline__ uint32_t near_key(float lb, float cb) { return lb <= cb ? __float_as_uint(lb) : kMissKey; }

__device__ __forceinline__ void store_miss(const wgt_nearest_buffers& out, size_t n, size_t i) {
  if (out.prim) out.prim[i] = kNoHit;
  if (out.dist) out.dist[i] = __builtin_inff();
  if (out.pos) out.pos[i] = out.pos[n + i] = out.pos[2 * n + i] = 0.0f;
  if (out.uv) out.uv[i] = out.uv[n + i] = 0.0f;
}

// STATS: the counting instantiation (wgt_nearest_points_stats) adds its lanes' node visits and
// triangle tests to counts[0] and counts[1]; the plain one carries no counters.
template <bool TRIS, bool STATS>
__global__ void __launch_bounds__(kBlock)
k_nearest(DevScene sc, const float* __restrict__ points, const float* __restrict__ max_dist, uint32_t n,
          wgt_nearest_buffers out, unsigned long long* __restrict__ counts) {
  extern __shared__ int s_stack[];  // sc.stack entries per lane (stack_lds_bytes)
  int* lds = s_stack + threadIdx.x;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const f3 p = f3{points[i], points[(size_t)n + i], points[2 * (size_t)n + i]};
  const float inf = __builtin_inff();
  const float m = max_dist ? max_dist[i] : inf;
  const float l1 = fabs_w(p.x) + fabs_w(p.y) + fabs_w(p.z);
  // no distance is below a limit that is zero, negative or NaN; a NaN or infinite point has no finite d2
  if (!TRIS || !(m > 0.0f) || !(l1 < inf)) {
    store_miss(out, n, i);
    return;
  }
  uint32_t n_nodes = 0, n_tests = 0;
  float best = inf;
  uint32_t bi = kNoHit, brec = 0;
  // the radius' bound, and the current one: min(radius', best's)
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
      const NearestTri c = nearest_on_tri(p, xyz(A), xyz(B), xyz(C));
      if (nearest_better(c.d2, idx, best, bi)) {
        best = c.d2;
        bi = idx;
        brec = t.lf;
        cb = __builtin_fminf(cbm, nearest_cull_bound(best));
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
      uint32_t k0 = near_key(nearest_box_bound(lx.x, hx.x, ly.x, hy.x, lz.x, hz.x, p), cb);
      uint32_t k1 = near_key(nearest_box_bound(lx.y, hx.y, ly.y, hy.y, lz.y, hz.y, p), cb);
      uint32_t k2 = near_key(nearest_box_bound(lx.z, hx.z, ly.z, hy.z, lz.z, hz.z, p), cb);
      uint32_t k3 = near_key(nearest_box_bound(lx.w, hx.w, ly.w, hy.w, lz.w, hz.w, p), cb);
      cas(k0, r0, k1, r1);
      cas(k2, r2, k3, r3);
      cas(k0, r0, k2, r2);
      cas(k1, r1, k3, r3);
      cas(k1, r1, k2, r2);
      // push the kept children other than the nearest, farthest first; a write for a dropped child
      // lands above the top and is overwritten or never read (trav_step)
      lds[t.sp * kBlock] = r3;
      t.sp += k3 != kMissKey ? 1 : 0;
      lds[t.sp * kBlock] = r2;
      t.sp += k2 != kMissKey ? 1 : 0;
      lds[t.sp * kBlock] = r1;
      t.sp += k1 != kMissKey ? 1 : 0;
      next = r0;
      pop = k0 == kMissKey;
    }
    if (trav_next(t, lds, pop, next)) break;
  }
  if (STATS) {
    atomicAdd(&counts[0], (unsigned long long)n_nodes);
    atomicAdd(&counts[1], (unsigned long long)n_tests);
  }
  const float dist = sqrt_rn(best);
  if (!nearest_reported(bi, dist, m)) {
    store_miss(out, n, i);
    return;
  }
  if (out.prim) out.prim[i] = sc.n_lights + sc.n_quads + bi;
  if (out.dist) out.dist[i] = dist;
  if (out.pos || out.uv) {
    // the winner's weights and point again, from its record: five registers not carried through the loop
    const float4* __restrict__ r = (const float4*)((const char*)sc.tris + brec);
    const NearestTri c = nearest_on_tri(p, xyz(r[0]), xyz(r[1]), xyz(r[2]));
    if (out.pos) {
      out.pos[i] = c.q.x;
      out.pos[(size_t)n + i] = c.q.y;
      out.pos[2 * (size_t)n + i] = c.q.z;
    }
    if (out.uv) {
      out.uv[i] = c.v;
      out.uv[(size_t)n + i] = c.w;
    }
  }
}

}  // namespace

hipError_t launch_nearest(const DevScene& sc, const float* d_points, const float* d_max_dist, uint32_t n,
                          const wgt_nearest_buffers& out, unsigned long long* d_counts, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
  const bool tris = sc.n_tris > 0;
  (d_counts ? (tris ? k_nearest<true, true> : k_nearest<false, true>)
            : (tris ? k_nearest<true, false> : k_nearest<false, false>))
      <<<grid, block, stack_lds_bytes(sc.stack), stream>>>(sc, d_points, d_max_dist, n, out, d_counts);
  return hipGetLastError();
}

}  // namespace wgt
