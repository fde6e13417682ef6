// wgt_overlap.hip — triangle overlap queries on the resident triangle BVH (wgt_overlap_triangles,
// DESIGN.md §4.17), in a translation unit of their own as the other queries are.
//
// Record i = the resident triangles that query triangle i cuts: whether there is one, how many, and the k
// lowest primitive ids of them.  wgt_overlap.h states the definition (tri_overlap: the box clause on the
// triangle's padded box, then six segment tests), which the host's brute force
// wgt_overlap_triangles_spec evaluates too.  tri_overlap is decided per pair, whatever the order, and the
// answer is a set's size and its lowest ids, so the traversal answers what the brute force answers as long
// as it skips only triangles the box clause refuses.  It does: a child is kept iff the query's box overlaps
// the child's on all three axes (overlap_boxes, the box clause's own six comparisons), every node box is the
// exact union of the padded boxes below it, so a dropped child holds no triangle that passes the box clause.
// No rounding enters: minima, maxima and comparisons only.
//
// The form is k_nearest_k's count form: one query per lane, kBlock lanes per workgroup, the per-lane LDS
// stack, one node or one triangle per step, trav_next as the tail.  Nothing the traversal finds changes
// what it visits, so the node step descends in slot order with occ_step's push form, and the builder's
// stack bound holds for any order.  The lane's list of ids lives in LDS behind the stack
// (overlap_lds_bytes), ascending, one word per entry at stride kBlock.  The write-out is planar.
#include "wgt_overlap.h"
#include "wgt_trav.h"

namespace wgt {

namespace {

// TRIS: the scene has triangles.  ANY: only hit is asked for, the traversal ends at the first overlapping
// triangle.  STATS: the counting instantiation (wgt_overlap_triangles_stats) adds its lanes' node visits
// and triangle tests to counts[0] and counts[1].
template <bool TRIS, bool ANY, bool STATS>
__global__ void __launch_bounds__(kBlock)
k_overlap(DevScene sc, OverlapPlan pl, const float* __restrict__ q, wgt_overlap_buffers out,
          unsigned long long* __restrict__ counts) {
  extern __shared__ int s_mem[];  // sc.stack entries per lane, then pl.k list words per lane
  int* lds = s_mem + threadIdx.x;
  int* list = s_mem + sc.stack * kBlock + threadIdx.x;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const size_t n = pl.n;
  if (i >= pl.n) return;
  const uint32_t k = ANY ? 0u : pl.k;
  const f3 a0 = f3{q[i], q[n + i], q[2 * n + i]};
  const f3 a1 = f3{q[3 * n + i], q[4 * n + i], q[5 * n + i]};
  const f3 a2 = f3{q[6 * n + i], q[7 * n + i], q[8 * n + i]};
  uint32_t cnt = 0, len = 0, n_nodes = 0, n_tests = 0;
  // an invalid query has the empty answer before any triangle is looked at
  if (TRIS && overlap_query_ok(a0, a1, a2)) {
    f3 qlo, qhi;
    overlap_query_box(a0, a1, a2, qlo, qhi);
    Trav t;
    t.ref = 0;
    t.lf = t.le = 0;
    t.sp = 0;
    for (;;) {
      bool pop;
      int next = 0;
      if (t.lf < t.le) {
        if (STATS) ++n_tests;
        const float4* __restrict__ r = (const float4*)((const char*)sc.tris + t.lf);
        const float4 A = r[0], B = r[1], C = r[2], D = r[3];
        // the box clause first (row D and the fourth words of B and C: wgt_trav.h tri_test_rec), the six
        // segment tests only when it holds
        if (overlap_boxes(qlo, qhi, B.w, D.y, C.w, D.z, D.x, D.w) && overlap_segments(a0, a1, a2, xyz(A), xyz(B), xyz(C))) {
          ++cnt;
          if (ANY) break;
          ov_insert(list, k, len, __float_as_uint(A.w));
        }
        t.lf += kTriRecordBytes;
        if (t.lf < t.le) continue;
        pop = true;
      } else {
        if (STATS) ++n_nodes;
        const float4* __restrict__ nd = (const float4*)((const char*)sc.nodes + (uint32_t)t.ref);  // ref: byte offset
        const float4 lx = nd[0], hx = nd[1], ly = nd[2], hy = nd[3], lz = nd[4], hz = nd[5];
        const float4 rf = nd[6];
        const int r0 = __float_as_int(rf.x), r1 = __float_as_int(rf.y), r2 = __float_as_int(rf.z), r3 = __float_as_int(rf.w);
        // an empty slot is the point box at kEmptySlotCoord, above every valid query's box
        const bool h0 = overlap_boxes(qlo, qhi, lx.x, hx.x, ly.x, hy.x, lz.x, hz.x);
        const bool h1 = overlap_boxes(qlo, qhi, lx.y, hx.y, ly.y, hy.y, lz.y, hz.y);
        const bool h2 = overlap_boxes(qlo, qhi, lx.z, hx.z, ly.z, hy.z, lz.z, hz.z);
        const bool h3 = overlap_boxes(qlo, qhi, lx.w, hx.w, ly.w, hy.w, lz.w, hz.w);
        // occ_step's node step: the first kept slot is entered, the later ones are pushed, last first; a
        // write for a dropped child lands above the top and is overwritten or never read (trav_step)
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
      if (trav_next(t, lds, pop, next)) break;
    }
  }
  if (STATS) {
    atomicAdd(&counts[0], (unsigned long long)n_nodes);
    atomicAdd(&counts[1], (unsigned long long)n_tests);
  }
  if (out.hit) out.hit[i] = cnt > 0 ? 1 : 0;
  if (ANY) return;
  if (out.count) out.count[i] = cnt;
  const uint32_t nlq = sc.n_lights + sc.n_quads;
  if (out.prim)
    for (uint32_t j = 0; j < k; ++j) out.prim[j * n + i] = j < len ? nlq + (uint32_t)list[j * kBlock] : kNoHit;
}

template <bool STATS>
hipError_t launch(const DevScene& sc, const OverlapPlan& p, const float* d_tris, const wgt_overlap_buffers& out,
                  unsigned long long* d_counts, hipStream_t stream) {
  const dim3 grid((p.n + kBlock - 1) / kBlock), block(kBlock);
  // without triangles there is no traversal, so no form
  (sc.n_tris == 0 ? k_overlap<false, false, STATS> : p.any ? k_overlap<true, true, STATS> : k_overlap<true, false, STATS>)
      <<<grid, block, p.lds, stream>>>(sc, p, d_tris, out, d_counts);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_overlap(const DevScene& sc, const OverlapPlan& p, const float* d_tris, const wgt_overlap_buffers& out,
                          unsigned long long* d_counts, hipStream_t stream) {
  if (p.n == 0) return hipSuccess;
  // the kernel's list and stack indices stay within what the plan sized, and the form is the fields'
  const bool any = out.hit && !out.count && !out.prim;
  if (p.k > WGT_OVERLAP_MAX_K || (p.any != 0) != any || p.lds != overlap_lds_bytes(sc.stack, p.k) ||
      p.lds > kOverlapLdsPerWorkgroup)
    return hipErrorInvalidValue;
  if ((p.k == 0) != (out.prim == nullptr)) return hipErrorInvalidValue;
  if (!out.hit && !out.count && !out.prim) return hipErrorInvalidValue;
  return d_counts ? launch<true>(sc, p, d_tris, out, d_counts, stream) : launch<false>(sc, p, d_tris, out, nullptr, stream);
}

}  // namespace wgt
