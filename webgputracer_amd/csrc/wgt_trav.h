// wgt_trav.h — the BVH4 traversal shared by every kernel that traces: the triangle test, the
// traversal state (Trav), the children's sort keys of both node forms, and the flat
// traversal (one ray per lane, one node or one triangle per step: trav_step) with the
// closest-hit query built on it (closest_hit) for k_render, k_trace_hits, k_gbuffer and
// k_occluded's fallback.  The speculative traversal of k_render_ps is wgt_trav_ps.h.
#pragma once

#include "wgt_hit.h"

namespace wgt {

struct TravStats {
  uint32_t nodes, tris, wave_steps, lane_steps;
  uint32_t spills, refills;  // parked k_render_ps: global-stack moves (park_fix)
  uint32_t overflows;        // parked k_render_ps: park_fix's overflow exit (never taken: tests assert 0)
};

// Counts one per wave (first active lane) and one per active lane.
__device__ __forceinline__ void simt_count(uint32_t& wave, uint32_t& lane) {
  const unsigned long long b = __ballot(1);
  if (__lane_id() == (unsigned)(__ffsll((long long)b) - 1)) ++wave;
  ++lane;
}

// One triangle test of a 64-B record (wgt_geom.h kTriRecordBytes) held in registers:
// Moller-Trumbore, then for every triangle that passes it the slab interval [bn, bf] of the
// triangle's own padded box: an empty interval rejects, and the hit parameter
// is t clamped to it (bn <= bf and no NaN, so the median of the three is the clamp: one
// v_med3_f32), rejected when the clamp leaves [kRayMin, kRayMax].  Only then the comparison
// with (bt, bi).  inv: 1/d.  Returns true with (tt, idx) when the triangle becomes the closest hit.
// SHORT: mt_test's short reciprocal (render rays only, wgt_geom.h).
// tri_tail is the part after Moller-Trumbore: tt comes in as its t and leaves clamped.
__device__ __forceinline__ bool tri_tail(f3 blo, f3 bhi, f3 ot, f3 inv, float bt, uint32_t bi, float& tt, uint32_t idx) {
  float bn, bf;
  slab(ot, inv, blo, bhi, bn, bf);
  tt = __builtin_amdgcn_fmed3f(tt, bn, bf);
  // One predicate, no branch (nested early-outs here cost the triangle step more exec-mask
  // bookkeeping than the three compares they saved).  The clamp cannot leave the range upwards
  // unnoticed: an accepted t is <= bt <= kRayMax (bt starts at kRayMax, or is a quad's t, an
  // earlier triangle's or the occlusion bound).  For an empty interval tt is meaningless and unused.
  return (bn <= bf) & (tt >= kRayMin) & ((tt < bt) | ((tt == bt) & (idx < bi)));
}
template <bool SHORT>
__device__ __forceinline__ bool tri_test_rec(float4 A, float4 B, float4 C, float4 D, f3 o, f3 d, f3 ot, f3 inv,
                                             float bt, uint32_t bi, float& tt, uint32_t& idx) {
  const f3 v0 = xyz(A), e1 = xyz(B), e2 = xyz(C);
  idx = __float_as_uint(A.w);
  const f3 blo = f3{B.w, C.w, D.x}, bhi = f3{D.y, D.z, D.w};
  if (!mt_test<SHORT>(o, d, v0, e1, e2, tt)) return false;
  return tri_tail(blo, bhi, ot, inv, bt, bi, tt, idx);
}
// The same for the record at byte offset lf: all four float4 loaded at once (the padded box D,
// for a candidate closest hit, used to be loaded in the branch, a second dependent round trip).
template <bool SHORT>
__device__ __forceinline__ bool tri_test(const float4* __restrict__ tris, uint32_t lf, f3 o, f3 d, f3 ot, f3 inv,
                                         float bt, uint32_t bi, float& tt, uint32_t& idx) {
  const float4* __restrict__ p = (const float4*)((const char*)tris + lf);
  return tri_test_rec<SHORT>(p[0], p[1], p[2], p[3], o, d, ot, inv, bt, bi, tt, idx);
}

// Resumable BVH4 traversal: closest triangle = min (t, index) with t < bound (or
// t <= bound and index < bi when bi = kNoHit).  Per-lane stack: DevScene::stack
// entries in LDS (stride kBlock, conflict-free).
struct Trav {
  f3 inv, ot;
  float bt;
  uint32_t bi;
  int ref;          // current internal node (when no leaf is open)
  uint32_t lf, le;  // open leaf: byte offsets of the next triangle record and of the leaf's end
  int sp;
};

// The node form CN: 0 = 128-B nodes, 1 = 80-B compact records.

// CN (compact nodes): t.inv holds s/d (s = the form's step, a power of two: exact), the
// factor of the fused slab step (cchild_key); the triangle box check multiplies
// it back by 1/s.
// EXACT: the IEEE 1/d (the ray queries' caller-supplied rays); else the short reciprocal (render rays).
template <int CN = 0, bool EXACT = false>
__device__ __forceinline__ void trav_init(const DevScene& sc, f3 o, f3 d, bool quad_hit, float qt, Trav& t) {
  t.inv = EXACT ? f3{safe_inv(d.x), safe_inv(d.y), safe_inv(d.z)}
                : f3{safe_inv_short(d.x), safe_inv_short(d.y), safe_inv_short(d.z)};
  t.ot = slab_offset(o, t.inv);
  if (CN) t.inv = sc.cstep * t.inv;
  // a triangle must satisfy t < t_quad to beat a quad hit (ray_dist is monotone in
  // t): with bi = kNoHit the rule "t < bt, or t == bt and index < bi" accepts
  // exactly t <= bt, so bt = the float below t_quad (t_quad > 0).  A box entered
  // at t_quad could only hold triangles with t >= t_quad, so culling it is exact.
  t.bt = quad_hit ? __uint_as_float(__float_as_uint(qt) - 1u) : kRayMax;
  t.bi = kNoHit;
  t.ref = 0;
  t.lf = t.le = 0;
  t.sp = 0;
}

// Sort key of one BVH4 child: the bits of the clamped entry distance max(near,
// kRayMin) (positive and not NaN, so its bits order as unsigned and never equal
// kMissKey); kMissKey if the ray misses the box or the box lies beyond the current
// closest hit.  Equal keys sort in either order (the ref moves with its key).  hit = max(near, kRayMin) <= min(far, bt) is the node test
// near <= far && near <= bt && far >= kRayMin, because bt >= kRayMin always
// (bt is kRayMax, a quad t or a triangle t, all >= kRayMin).
constexpr uint32_t kMissKey = 0xFFFFFFFFu;
// min(f, bt) for bt > 0 and f not NaN (no NaN ray traverses: wgt_kernels.hip resolves
// them without tracing, and closest_hit answers a NaN caller ray with nan_hit): the signed
// minimum of the bits orders every negative f below bt and positive floats as fminf
// does.  An integer minimum needs no canonicalised operand, where fminf of the
// loop-carried bt costs a v_max_f32 bt, bt per node step (IEEE mode).  Compact nodes only:
// the 128-B form's step measured 0.9 % slower with it (profiles/r06/ab_r06q.txt).
__device__ __forceinline__ float min_bt(float f, float bt) {
  return __int_as_float(__builtin_elementwise_min(__float_as_int(f), __float_as_int(bt)));
}
__device__ __forceinline__ uint32_t child_key(const Trav& t, float lx, float hx, float ly, float hy,
                                              float lz, float hz) {
  const float t0x = __builtin_fmaf(lx, t.inv.x, t.ot.x), t1x = __builtin_fmaf(hx, t.inv.x, t.ot.x);
  const float t0y = __builtin_fmaf(ly, t.inv.y, t.ot.y), t1y = __builtin_fmaf(hy, t.inv.y, t.ot.y);
  const float t0z = __builtin_fmaf(lz, t.inv.z, t.ot.z), t1z = __builtin_fmaf(hz, t.inv.z, t.ot.z);
  const float n = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(t0x, t1x), __builtin_fminf(t0y, t1y)),
                                  __builtin_fmaxf(__builtin_fminf(t0z, t1z), kRayMin));
  const float f = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(t0x, t1x), __builtin_fmaxf(t0y, t1y)),
                                  __builtin_fminf(__builtin_fmaxf(t0z, t1z), t.bt));
  return n <= f ? __float_as_uint(n) : kMissKey;
}
// Sort keys and refs of the 4 children of node `ref`, read from the 128-B nodes
// (CN = false) or from the compact nodes (CN = true, wgt_geom.h).
__device__ __forceinline__ float hcode(uint32_t w, uint32_t slot) {
  return (float)__builtin_bit_cast(_Float16, (uint16_t)((slot & 1u) ? (w >> 16) : (w & 0xffffu)));
}
// Compact node: per axis the ray's entry plane is the lo code for inv >= 0 and the
// hi code for inv < 0 (one select per two children), which equals the min / max
// form of child_key because the slab formula is monotone in the plane.  The slab
// distance of the plane org' + h*s is one fused step fma(h, s/d, c) with h taken
// from a half word (v_fma_mix_f32) and c = fma(org/s, s/d, ot) per node and axis;
// the builder's code margin makes the interval contain the exact one (wgt_geom.h,
// DESIGN.md §3.4).  An empty slot's +inf codes give n = +inf or f = -inf: a miss
// without a mask.
__device__ __forceinline__ uint32_t cchild_key(const Trav& t, const uint32_t* nw, const uint32_t* fw, f3 c,
                                               uint32_t slot) {
  const uint32_t k = slot >> 1;
  const float tnx = __builtin_fmaf(hcode(nw[0 + k], slot), t.inv.x, c.x);
  const float tfx = __builtin_fmaf(hcode(fw[0 + k], slot), t.inv.x, c.x);
  const float tny = __builtin_fmaf(hcode(nw[2 + k], slot), t.inv.y, c.y);
  const float tfy = __builtin_fmaf(hcode(fw[2 + k], slot), t.inv.y, c.y);
  const float tnz = __builtin_fmaf(hcode(nw[4 + k], slot), t.inv.z, c.z);
  const float tfz = __builtin_fmaf(hcode(fw[4 + k], slot), t.inv.z, c.z);
  const float n = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), __builtin_fmaxf(tnz, kRayMin));
  const float f = min_bt(__builtin_fminf(__builtin_fminf(tfx, tfy), tfz), t.bt);
  return n <= f ? __float_as_uint(n) : kMissKey;
}
template <int CN>
__device__ __forceinline__ void node_keys(const DevScene& sc, const Trav& t, int ref, uint32_t& k0, uint32_t& k1,
                                          uint32_t& k2, uint32_t& k3, int& r0, int& r1, int& r2, int& r3) {
  if (CN) {
    // 80-B record: origin, codes, refs
    const float4* __restrict__ n = (const float4*)((const char*)sc.cnodes + (uint32_t)ref);  // byte offset
    const int4 rf = __builtin_bit_cast(int4, n[4]);
    const float4 a = n[0];
    const uint4 x = __builtin_bit_cast(uint4, n[1]), y = __builtin_bit_cast(uint4, n[2]),
                z = __builtin_bit_cast(uint4, n[3]);
    // c = the slab distance of the node origin org' = (org/s) * s: fma(org/s, s/d, ot)
    const f3 c = f3{__builtin_fmaf(a.x, t.inv.x, t.ot.x), __builtin_fmaf(a.y, t.inv.y, t.ot.y),
                    __builtin_fmaf(a.z, t.inv.z, t.ot.z)};
    const bool sx = t.inv.x < 0.0f, sy = t.inv.y < 0.0f, sz = t.inv.z < 0.0f;
    const uint32_t nw[6] = {sx ? x.z : x.x, sx ? x.w : x.y, sy ? y.z : y.x,
                            sy ? y.w : y.y, sz ? z.z : z.x, sz ? z.w : z.y};
    const uint32_t fw[6] = {sx ? x.x : x.z, sx ? x.y : x.w, sy ? y.x : y.z,
                            sy ? y.y : y.w, sz ? z.x : z.z, sz ? z.y : z.w};
    r0 = rf.x, r1 = rf.y, r2 = rf.z, r3 = rf.w;
    k0 = cchild_key(t, nw, fw, c, 0u);
    k1 = cchild_key(t, nw, fw, c, 1u);
    k2 = cchild_key(t, nw, fw, c, 2u);
    k3 = cchild_key(t, nw, fw, c, 3u);
  } else {
    const float4* __restrict__ n = (const float4*)((const char*)sc.nodes + (uint32_t)ref);  // ref: byte offset
    const float4 lx = n[0], hx = n[1], ly = n[2], hy = n[3], lz = n[4], hz = n[5];
    const float4 rf = n[6];
    r0 = __float_as_int(rf.x), r1 = __float_as_int(rf.y), r2 = __float_as_int(rf.z), r3 = __float_as_int(rf.w);
    k0 = child_key(t, lx.x, hx.x, ly.x, hy.x, lz.x, hz.x);
    k1 = child_key(t, lx.y, hx.y, ly.y, hy.y, lz.y, hz.y);
    k2 = child_key(t, lx.z, hx.z, ly.z, hy.z, lz.z, hz.z);
    k3 = child_key(t, lx.w, hx.w, ly.w, hy.w, lz.w, hz.w);
  }
}

// Compare-exchange of (key, ref) pairs: the smaller key (and its ref) to a.
__device__ __forceinline__ void cas(uint32_t& ka, int& ra, uint32_t& kb, int& rb) {
  const bool sw = kb < ka;
  const uint32_t k = sw ? kb : ka;
  kb = sw ? ka : kb;
  ka = k;
  const int r = sw ? rb : ra;
  rb = sw ? ra : rb;
  ra = r;
}

// The end of a flat step (trav_step, k_occluded's occ_step) after its leaf-or-node branch:
// `next` is the child to enter, or with `pop` the step left none and the top stack entry is
// taken.  A leaf is opened as a range, a node becomes t.ref.  Returns true when the stack
// is empty: the traversal has finished.
__device__ __forceinline__ bool trav_next(Trav& t, int* __restrict__ lds, bool pop, int next) {
  if (pop) {
    if (t.sp == 0) return true;
    --t.sp;
    next = lds[t.sp * kBlock];
  }
  const bool leaf = next < 0;
  const uint32_t lfirst = leaf_first(next) * kTriRecordBytes;
  t.lf = leaf ? lfirst : t.lf;
  t.le = leaf ? lfirst + leaf_count(next) * kTriRecordBytes : t.le;
  t.ref = leaf ? t.ref : next;
  return false;
}

// One BVH4 node OR one triangle per call (a leaf is opened as a range and its
// triangles are tested one per step), so every lane's step costs about the same
// and a wave never pays for an 8-triangle leaf loop at every step.  A node step
// sorts its hit children by entry distance (5 compare-exchanges of (key, ref)), descends into
// the nearest and pushes the others farthest first.  The stack lives in LDS
// only, sized to the builder's exact worst case, so it cannot overflow.  Push /
// pop / descend are selects around one leaf-or-node branch to keep the
// exec-mask bookkeeping small.  Returns true when the traversal has finished.
template <bool STATS>
__device__ __forceinline__ bool trav_step(const DevScene& sc, f3 o, f3 d, Trav& t,
                                          int* __restrict__ lds, TravStats& st) {
  if (STATS) simt_count(st.wave_steps, st.lane_steps);
  bool pop;
  int next = 0;
  if (t.lf < t.le) {
    if (STATS) st.tris++;
    float tt;
    uint32_t idx;
    if (tri_test<false>(sc.tris, t.lf, o, d, t.ot, t.inv, t.bt, t.bi, tt, idx)) {  // IEEE: any caller ray
      t.bt = tt;
      t.bi = idx;
    }
    t.lf += kTriRecordBytes;
    if (t.lf < t.le) return false;
    pop = true;
  } else {
    if (STATS) st.nodes++;
    uint32_t k0, k1, k2, k3;
    int r0, r1, r2, r3;
    node_keys<false>(sc, t, t.ref, k0, k1, k2, k3, r0, r1, r2, r3);
    cas(k0, r0, k1, r1);
    cas(k2, r2, k3, r3);
    cas(k0, r0, k2, r2);
    cas(k1, r1, k3, r3);
    cas(k1, r1, k2, r2);
    // push the hit children other than the nearest, farthest first; a write for a
    // missed child lands above the top and is overwritten or never read
    lds[t.sp * kBlock] = r3;
    t.sp += k3 != kMissKey ? 1 : 0;
    lds[t.sp * kBlock] = r2;
    t.sp += k2 != kMissKey ? 1 : 0;
    lds[t.sp * kBlock] = r1;
    t.sp += k1 != kMissKey ? 1 : 0;
    next = r0;
    pop = k0 == kMissKey;
  }
  return trav_next(t, lds, pop, next);
}

// The closest hit of one ray, the reference's sample_hit (path_tracer.wgsl:290-310) with the
// triangles between quads and spheres: k_render (its STATS), and with EXACT (the IEEE forms,
// for any caller ray) k_trace_hits, k_gbuffer and k_occluded's fallback.  quad_scan_fast
// leaves (qprim, qt), all the traversal needs of the quad hit (trav_init reads whether there
// is one and its t), so the quad hit is rebuilt after the loop and the thirteen registers of
// Hit are not live across it: the order of k_render_ps's finalise.
template <bool TRIS, bool STATS, bool EXACT = false>
__device__ __forceinline__ void closest_hit(const DevScene& sc, f3 o, f3 d, int* __restrict__ lds,
                                            Hit& h, TravStats& st) {
  if (has_nan(o) || has_nan(d)) {
    nan_hit(sc, o, d, h);
    return;
  }
  float qt;
  uint32_t qprim;
  quad_scan_fast<EXACT>(sc, o, d, qprim, qt);
  Trav t;
  trav_init<0, EXACT>(sc, o, d, qprim != kNoHit, qt, t);
  if (TRIS) {
    while (!trav_step<STATS>(sc, o, d, t, lds, st)) {
    }
  }
  quad_rebuild(sc, o, d, qprim, qt, h);
  finish_hit(sc, o, d, t.bt, t.bi, h);
}

// The same without statistics (the ray queries).
template <bool TRIS, bool EXACT>
__device__ __forceinline__ void closest_hit(const DevScene& sc, f3 o, f3 d, int* __restrict__ lds, Hit& h) {
  TravStats st{};
  closest_hit<TRIS, false, EXACT>(sc, o, d, lds, h, st);
}

}  // namespace wgt
