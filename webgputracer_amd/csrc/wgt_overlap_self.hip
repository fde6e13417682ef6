// wgt_overlap_self.hip — self-intersection queries on the resident triangle BVH (wgt_overlap_self,
// DESIGN.md §4.18), in a translation unit of their own as the other queries are.
//
// Record s = the resident triangles that resident triangle s cuts, neighbours by the index buffer excluded:
// whether there is one, how many, and the k lowest primitive ids of them.  wgt_overlap_self.h states the
// definition (self_overlap: the id test, the adjacency test, the box clause on the two padded boxes, then the
// six segment tests with the lower id as the query), which the host's brute force wgt_overlap_self_spec
// evaluates too.  self_overlap is decided per unordered pair and the answer is a set's size and its lowest
// ids, so the traversal answers what the brute force answers as long as it skips only triangles the box
// clause refuses.  It does: the lane traverses with its own padded box (row D of its record), a child is kept
// iff that box overlaps the child's on all three axes (overlap_boxes), and every node box is the exact union
// of the padded boxes below it.  No rounding enters: minima, maxima and comparisons only.
//
// The form is k_overlap's: one triangle per lane, kBlock lanes per workgroup, the per-lane LDS stack, one node
// or one triangle per step, trav_next as the tail, slot-order descent with occ_step's push form, the lane's
// list of ids in LDS behind the stack.  Lane i serves the i-th record in leaf order, so the lanes of a wave
// hold spatially neighbouring triangles and walk nearly the same nodes; the answer is written at the
// record's id (word A.w), the upload index.
#include "wgt_overlap_self.h"
#include "wgt_trav.h"

namespace wgt {

namespace {

__device__ __forceinline__ f3 pick(bool c, f3 a, f3 b) { return f3{c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z}; }

// ANY: only hit is asked for, the traversal ends at the first member.  STATS: the counting instantiation
// (wgt_overlap_self_stats) adds its lanes' node visits and triangle tests to counts[0] and counts[1].
// index is null when the call has no index buffer: a wave-uniform branch, not an instantiation (one was
// tried: the same registers either way).
template <bool ANY, bool STATS>
__global__ void __launch_bounds__(kBlock)
k_overlap_self(DevScene sc, OverlapSelfPlan pl, const uint32_t* __restrict__ index, wgt_overlap_buffers out,
               unsigned long long* __restrict__ counts) {
  extern __shared__ int s_mem[];  // sc.stack entries per lane, then pl.k list words per lane
  int* lds = s_mem + threadIdx.x;
  int* list = s_mem + sc.stack * kBlock + threadIdx.x;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const size_t n = pl.n;
  if (i >= pl.n) return;
  const uint32_t k = ANY ? 0u : pl.k;
  // the lane's own record, the i-th in leaf order: its id, its triangle and its padded box
  const float4* __restrict__ me = (const float4*)((const char*)sc.tris + (size_t)i * kTriRecordBytes);
  const float4 mA = me[0], mB = me[1], mC = me[2], mD = me[3];
  const uint32_t s = __float_as_uint(mA.w);
  if (s >= pl.n) return;  // the records' ids are a permutation of the upload indices: nothing is written elsewhere
  const f3 sv0 = xyz(mA), se1 = xyz(mB), se2 = xyz(mC);
  const f3 qlo = f3{mB.w, mC.w, mD.x}, qhi = f3{mD.y, mD.z, mD.w};
  const bool indexed = index != nullptr;
  uint32_t l0 = 0, l1 = 0, l2 = 0;
  if (indexed) {
    const uint32_t* __restrict__ L = index + 3 * (size_t)s;
    l0 = L[0], l1 = L[1], l2 = L[2];
  }
  uint32_t cnt = 0, len = 0, n_nodes = 0, n_tests = 0;
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
      // the box clause first (row D and the fourth words of B and C), then the id test, the adjacency test
      // and the six segment tests with the roles chosen by id
      if (overlap_boxes(qlo, qhi, B.w, D.y, C.w, D.z, D.x, D.w)) {
        const uint32_t c = __float_as_uint(A.w);
        bool open = c != s;
        if (indexed && open && c < pl.n) {  // every id is below n: nothing is loaded from outside the buffer
          const uint32_t* __restrict__ L = index + 3 * (size_t)c;
          open = !self_adjacent(l0, l1, l2, L[0], L[1], L[2]);
        }
        if (open) {
          // the lower id's record gives the corners (self_segments rebuilds them), the higher id's is resident
          const bool low = c < s;
          if (self_segments(pick(low, xyz(A), sv0), pick(low, xyz(B), se1), pick(low, xyz(C), se2),
                            pick(low, sv0, xyz(A)), pick(low, se1, xyz(B)), pick(low, se2, xyz(C)))) {
            ++cnt;
            if (ANY) break;
            ov_insert(list, k, len, c);
          }
        }
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
      // an empty slot is the point box at kEmptySlotCoord, above every resident triangle's padded box
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
  if (STATS) {
    atomicAdd(&counts[0], (unsigned long long)n_nodes);
    atomicAdd(&counts[1], (unsigned long long)n_tests);
  }
  if (out.hit) out.hit[s] = cnt > 0 ? 1 : 0;
  if (ANY) return;
  if (out.count) out.count[s] = cnt;
  const uint32_t nlq = sc.n_lights + sc.n_quads;
  if (out.prim)
    for (uint32_t j = 0; j < k; ++j) out.prim[j * n + s] = j < len ? nlq + (uint32_t)list[j * kBlock] : kNoHit;
}

template <bool STATS>
hipError_t launch(const DevScene& sc, const OverlapSelfPlan& p, const uint32_t* d_index, const wgt_overlap_buffers& out,
                  unsigned long long* d_counts, hipStream_t stream) {
  const dim3 grid((p.n + kBlock - 1) / kBlock), block(kBlock);
  (p.any ? k_overlap_self<true, STATS> : k_overlap_self<false, STATS>)
      <<<grid, block, p.lds, stream>>>(sc, p, d_index, out, d_counts);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_overlap_self(const DevScene& sc, const OverlapSelfPlan& p, const uint32_t* d_index,
                               const wgt_overlap_buffers& out, unsigned long long* d_counts, hipStream_t stream) {
  if (p.n == 0) return hipSuccess;
  // one lane per resident record, the kernel's list and stack indices stay within what the plan sized, and
  // the form is the fields'
  const bool any = out.hit && !out.count && !out.prim;
  if (p.n != sc.n_tris || p.k > WGT_OVERLAP_MAX_K || (p.any != 0) != any || p.lds != overlap_lds_bytes(sc.stack, p.k) ||
      p.lds > kOverlapLdsPerWorkgroup)
    return hipErrorInvalidValue;
  if ((p.k == 0) != (out.prim == nullptr)) return hipErrorInvalidValue;
  if (!out.hit && !out.count && !out.prim) return hipErrorInvalidValue;
  return d_counts ? launch<true>(sc, p, d_index, out, d_counts, stream) : launch<false>(sc, p, d_index, out, nullptr, stream);
}

}  // namespace wgt
