// wgt_trav_ps.h — the speculative two-mode traversal of k_render_ps on wgt_trav.h's pieces:
// its LDS stacks (4-byte and 3-byte entries), the traversal state parked in LDS with the
// global part of a split stack (Park, park_fix), and the node and triangle steps.
#pragma once

#include "wgt_trav.h"

namespace wgt {

// Speculative two-mode traversal (k_render_ps).  A wave step is uniformly a
// NODE step (lanes with an internal node to visit) or a TRIANGLE step (lanes
// with a pending leaf), so a step issues one of the two code paths instead of
// both.  A lane that reaches a leaf parks it as its pending leaf and keeps
// descending (speculation, after Aila & Laine's speculative while-while); a
// second leaf found meanwhile waits on the stack (one entry beyond the
// builder's bound: DevScene::stack includes it).  Culling with a not yet
// updated best t is only less tight, never wrong: the closest hit is a minimum
// over (t, index) of every triangle whose boxes the ray enters.
//
// Lane state after every step: an internal node in t.ref, or kNoRef with a
// pending leaf (lf < le), or done (kNoRef, no pending leaf, empty stack).
constexpr int kNoRef = 0x7fffffff;

// The per-lane LDS traversal stack of k_render_ps, entry i of a lane at stride
// kBlock (conflict-free).  Stack32: one int per entry.  Stack24: a 16-bit and an
// 8-bit array (3 B per entry, the high byte sign-extending), which fits every ref
// of a tree with fewer than 2^16 nodes and 2^20 triangles (byte offsets < 2^23,
// leaf refs >= -2^23; DevScene::ps_waves) and lets LDS hold the full 31-entry
// bound of 24 waves per CU: 6 waves per SIMD without a narrower tree.
struct Stack32 {
  int* __restrict__ p;
  __device__ __forceinline__ int ld(int i) const { return p[i * kBlock]; }
  __device__ __forceinline__ void st(int i, int v) const { p[i * kBlock] = v; }
};
struct Stack24 {
  uint16_t* __restrict__ lo;
  int8_t* __restrict__ hi;
  __device__ __forceinline__ int ld(int i) const { return ((int)hi[i * kBlock] << 16) | (int)lo[i * kBlock]; }
  __device__ __forceinline__ void st(int i, int v) const {
    lo[i * kBlock] = (uint16_t)v;
    hi[i * kBlock] = (int8_t)(v >> 16);
  }
};
// Parked traversal state of k_render_ps (DevScene::ps_park): the
// lane's Trav lives in LDS words (stride kBlock, conflict-free) while its wave runs a
// service pass, so the service code does not hold the traversing lanes' 11 registers and
// needs no scratch.  Word 9 holds the LDS stack top in its low half and the depth of the
// lane's global stack (entries moved out of LDS, DevFrame::ps_spill) in its high half:
// the traversal phase reads and writes only the low half.  The open leaf is one word:
// the record offset (a multiple of kTriRecordBytes) plus the records left (<= 8).
struct Park {
  uint32_t* __restrict__ p;
  __device__ __forceinline__ uint32_t ld(int j) const { return p[j * kBlock]; }
  __device__ __forceinline__ void st(int j, uint32_t v) const { p[j * kBlock] = v; }
  __device__ __forceinline__ uint32_t sp() const { return ((const uint16_t*)(p + 9 * kBlock))[0]; }
  __device__ __forceinline__ void set_sp(uint32_t v) const { ((uint16_t*)(p + 9 * kBlock))[0] = (uint16_t)v; }
};
// the record offset's zero low bits (6 for 64-B records) hold the count (<= kLeafMax)
constexpr uint32_t kParkLeafMask = kTriRecordBytes - 1u;
static_assert((kTriRecordBytes & kParkLeafMask) == 0u && kParkLeafMask >= (uint32_t)kLeafMax,
              "the parked open leaf packs its count into the offset's low bits");
__device__ __forceinline__ uint32_t park_leaf(const Trav& t) { return t.lf | ((t.le - t.lf) / kTriRecordBytes); }
__device__ __forceinline__ void unpark_leaf(uint32_t w, Trav& t) {
  t.lf = w & ~kParkLeafMask;
  t.le = t.lf + (w & kParkLeafMask) * kTriRecordBytes;
}
// the whole state; the global depth (word 9's high half) is left as it is
__device__ __forceinline__ void park_put(const Park& P, const Trav& t) {
  P.st(0, __float_as_uint(t.inv.x)); P.st(1, __float_as_uint(t.inv.y)); P.st(2, __float_as_uint(t.inv.z));
  P.st(3, __float_as_uint(t.ot.x)); P.st(4, __float_as_uint(t.ot.y)); P.st(5, __float_as_uint(t.ot.z));
  P.st(6, __float_as_uint(t.bt)); P.st(7, t.bi); P.st(8, (uint32_t)t.ref);
  P.set_sp((uint32_t)t.sp);
  P.st(10, park_leaf(t));
}
__device__ __forceinline__ void park_get(const Park& P, Trav& t) {
  t.inv = f3{__uint_as_float(P.ld(0)), __uint_as_float(P.ld(1)), __uint_as_float(P.ld(2))};
  t.ot = f3{__uint_as_float(P.ld(3)), __uint_as_float(P.ld(4)), __uint_as_float(P.ld(5))};
  t.bt = __uint_as_float(P.ld(6));
  t.bi = P.ld(7);
  t.ref = (int)P.ld(8);
  t.sp = (int)P.sp();
  unpark_leaf(P.ld(10), t);
}

// Place `cand` (a child ref, or kNoRef = take the next stack entry): an internal node becomes
// t.ref; a leaf becomes the pending leaf when there is none, and the next stack entry is then
// placed the same way, or it waits on the stack when there is one, and the lane has no node.
// Nested ifs, the common case (an internal node) falling straight through: as a loop of up to
// three rounds left by break, continue and return, the same steps compiled to flags and copies
// of (ref, lf, le, sp) at every exit, and to a third round that no lane ever ran (the first leaf
// placed leaves a pending leaf, so the second round ends); DESIGN.md §4.2 item 33.
template <class STK>
__device__ __forceinline__ void trav_resolve(const DevScene& sc, Trav& t, int cand, const STK& lds) {
  if (cand == kNoRef) {
    if (t.sp == 0) {
      t.ref = kNoRef;
      return;
    }
    --t.sp;
    cand = lds.ld(t.sp);
  }
  if (cand < 0) {
    if (t.lf >= t.le) {  // no pending leaf: this one becomes it; look for a node once more
      t.lf = leaf_first(cand) * kTriRecordBytes;
      t.le = t.lf + leaf_count(cand) * kTriRecordBytes;
      cand = kNoRef;
      if (t.sp != 0) {
        const int next = lds.ld(t.sp - 1);
        if (next >= 0) {  // (a second leaf stays where it is)
          --t.sp;
          cand = next;
        }
      }
    } else {
      lds.st(t.sp, cand);  // a second leaf waits on the stack
      ++t.sp;
      cand = kNoRef;
    }
  }
  t.ref = cand;
}

__device__ __forceinline__ bool trav_done(const Trav& t) { return t.ref == kNoRef && t.lf >= t.le && t.sp == 0; }

// Parked k_render_ps: a lane leaves its traversal phase when a node step leaves fewer than
// 4 free LDS entries above its stack top (the next step's 3 pushes and a parked leaf), or
// when its LDS stack runs empty with entries still on its global stack.  Its service pass
// then moves stack entries between LDS and the lane's global stack (gs, stride `stride`)
// and the traversal resumes: the stack keeps its order, split over the two, so the
// traversal visits what the whole-LDS stack would (it only stops early when the LDS part
// runs empty, which any order of the exact min (t, index) search allows).
// Returns 1 for a spill, 2 for a refill.
template <class STK>
__device__ __forceinline__ uint32_t park_fix(const DevScene& sc, const Park& P, const STK& lds, uint32_t cap,
                                             int* __restrict__ gs, uint32_t stride) {
  const uint32_t w9 = P.ld(9);
  const uint32_t sp = w9 & 0xffffu, g = w9 >> 16;
  if (sp + 4u > cap) {  // overflow: all but the top `keep` entries move to the global stack
    const uint32_t keep = (cap - 3u) / 2u;  // 1 <= keep <= cap - 4 for cap >= kMinPsCap
    const uint32_t m = sp - keep;
    if (g + m > sc.stack) {
      // g + sp never exceeds the builder's bound sc.stack (the global stack's size); were
      // it to, the traversal ends here (a wrong image the parity tests catch) rather than
      // writing out of bounds or spilling forever
      P.st(8, (uint32_t)kNoRef);
      P.st(10, 0u);
      P.st(9, 0u);
      return 3u;
    }
    for (uint32_t i = 0; i < m; ++i) gs[(size_t)(g + i) * stride] = lds.ld((int)i);
    for (uint32_t i = 0; i < keep; ++i) lds.st((int)i, lds.ld((int)(i + m)));
    P.st(9, keep | (g + m) << 16);
    return 1u;
  }
  // the LDS part ran empty (nothing open, g > 0): the top m global entries come back, then
  // the pop the traversal stopped at; m - 1 <= cap - 4 leaves room for the next node step
  const uint32_t half = (cap - 3u) / 2u + 1u;
  const uint32_t m = g < half ? g : half;
  for (uint32_t i = 0; i < m; ++i) lds.st((int)i, gs[(size_t)(g - m + i) * stride]);
  Trav t;
  t.ref = kNoRef;
  unpark_leaf(P.ld(10), t);
  t.sp = (int)m;
  trav_resolve(sc, t, kNoRef, lds);
  P.st(8, (uint32_t)t.ref);
  P.st(10, park_leaf(t));
  P.st(9, (uint32_t)t.sp | (g - m) << 16);
  return 2u;
}

// Visit t.ref: bring the nearest hit child to slot 0 (three compare-exchanges: the
// pairs, then their minima), push the other three unordered, place the nearest.
// The full 5-exchange network cost 10 more VALU per node step for 0.6% fewer node
// visits.  Any order is exact (the closest hit is a minimum
// over (t, index)), and a missed child's kMissKey keeps it off the stack wherever it
// sits: each push advances the top only for a hit.
// ROOT: the step of a ray that has just started (t.ref = 0 for every lane): the node's
// address is uniform, so its loads are scalar (SMEM) loads shared by the wave.
template <bool STATS, int CN, class STK, bool ROOT = false>
__device__ __forceinline__ void node_step(const DevScene& sc, Trav& t, const STK& lds, TravStats& st) {
  if (STATS) st.nodes++;
  uint32_t k0, k1, k2, k3;
  int r0, r1, r2, r3;
  node_keys<CN>(sc, t, ROOT ? 0 : t.ref, k0, k1, k2, k3, r0, r1, r2, r3);
  cas(k0, r0, k1, r1);
  cas(k2, r2, k3, r3);
  cas(k0, r0, k2, r2);
  lds.st(t.sp, r3);
  t.sp += k3 != kMissKey ? 1 : 0;
  lds.st(t.sp, r2);
  t.sp += k2 != kMissKey ? 1 : 0;
  lds.st(t.sp, r1);
  t.sp += k1 != kMissKey ? 1 : 0;
  trav_resolve(sc, t, k0 != kMissKey ? r0 : kNoRef, lds);
}

// Test the next triangle of the pending leaf; a lane without a node to visit
// takes the next stack entry once its leaf is done.
template <bool STATS, int CN = 0, class STK>
__device__ __forceinline__ void tri_step(const DevScene& sc, f3 o, f3 d, Trav& t, const STK& lds,
                                         TravStats& st) {
  // 1/d: under CN t.inv holds s/d, and (s/d) * (1/s) is 1/d exactly
  const f3 inv = CN ? sc.rcstep * t.inv : t.inv;
#if WGT_TRI_PER_STEP > 1
  // up to WGT_TRI_PER_STEP triangles of the open leaf per step (a slot past the leaf's end
  // re-reads the first record and is ignored): the closest hit is a minimum over (t, index), so
  // testing them against the same bound and merging is exact.  Every slot's record is loaded
  // before any test: loaded inside tri_test, the second record's loads sat behind the first
  // test's early-out branches, two dependent round trips per step (round 6: sponza +1.5 %,
  // bunny +0.9 %)
  constexpr int K = WGT_TRI_PER_STEP;
  uint32_t n = 1;
  float4 R[K][4];
  // every record's address before any load: the empty asm ties the addresses together, so that
  // no record's loads can issue before the last address is known and the 4 K loads go out back
  // to back.  Without it the scheduler put the select of the second address behind the first
  // record's loads and a multiply of the first record, with the wait for its operand, before
  // the second record's loads: two round trips per step again (sponza -0.5 %)
  uint32_t ra[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint32_t a = t.lf + uint32_t(j) * kTriRecordBytes;
    ra[j] = (j == 0 || a < t.le) ? a : t.lf;
  }
#pragma unroll
  for (int j = 1; j < K; ++j) asm("" : "+v"(ra[0]), "+v"(ra[j]));
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const float4* __restrict__ q = (const float4*)((const char*)sc.tris + ra[j]);
    R[j][0] = q[0], R[j][1] = q[1], R[j][2] = q[2], R[j][3] = q[3];
  }
  // Every slot's Moller-Trumbore first, then one tail (tri_tail) for the slots that passed, lowest
  // slot first: a lane's slots meet the tail in the order, and against the bounds, that K whole
  // tests followed by a merge gave them.  Slot 0 is accepted against (bt, bi).  A later slot was
  // accepted against the same (bt, bi) and then merged by strict (t, index) order against the
  // bound the earlier slots left, which is never above (bt, bi): the two comparisons are the one
  // against the updated bound, the tail's own.  The tail's code exists once (the inlined whole
  // tests carried it K times, each behind its test's exits), and a wave runs it a second time
  // only when one of its lanes has two passing slots (DESIGN.md §4.2 item 34;
  // tests/tri_tail_restatement.py states both forms in numpy).
  float tm[K];
  uint32_t pass = 0u;  // bit j: slot j is live and passed Moller-Trumbore
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const bool live = j == 0 || t.lf + uint32_t(j) * kTriRecordBytes < t.le;
    // two exits (after u; after v and t): the fewest instructions short of the branch-free form
    const bool p = mt_test<true, 2>(o, d, xyz(R[j][0]), xyz(R[j][1]), xyz(R[j][2]), tm[j]);
    pass |= (p && live) ? 1u << j : 0u;
    if (j > 0) n += live ? 1u : 0u;
  }
#pragma nounroll
  while (pass != 0u) {
    // the record of the lowest slot that passed
    float iw = R[K - 1][0].w, lx = R[K - 1][1].w, ly = R[K - 1][2].w;
    float4 D = R[K - 1][3];
    float tj = tm[K - 1];
#pragma unroll
    for (int j = K - 2; j >= 0; --j) {
      const bool s = (pass & ((2u << j) - 1u)) == (1u << j);  // slot j is the lowest set
      iw = s ? R[j][0].w : iw, lx = s ? R[j][1].w : lx, ly = s ? R[j][2].w : ly;
      D.x = s ? R[j][3].x : D.x, D.y = s ? R[j][3].y : D.y, D.z = s ? R[j][3].z : D.z, D.w = s ? R[j][3].w : D.w;
      tj = s ? tm[j] : tj;
    }
    pass &= pass - 1u;
    const uint32_t idx = __float_as_uint(iw);
    // selects, not a branch around two moves
    const bool acc = tri_tail(f3{lx, ly, D.x}, f3{D.y, D.z, D.w}, t.ot, inv, t.bt, t.bi, tj, idx);
    t.bt = acc ? tj : t.bt;
    t.bi = acc ? idx : t.bi;
  }
  if (STATS) st.tris += n;
  t.lf += n * kTriRecordBytes;
#else
  if (STATS) st.tris++;
  float tt;
  uint32_t idx;
  if (tri_test<true>(sc.tris, t.lf, o, d, t.ot, inv, t.bt, t.bi, tt, idx)) {
    t.bt = tt;
    t.bi = idx;
  }
  t.lf += kTriRecordBytes;
#endif
  if (t.lf >= t.le && t.ref == kNoRef) trav_resolve(sc, t, kNoRef, lds);
}

}  // namespace wgt
