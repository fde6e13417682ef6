// wgt_motion.hip — where a hit point lay on its triangle before the triangles moved
// (wgt_motion_snapshot, wgt_motion_reproject), in a translation unit of its own: nothing here is read
// by a render, query or refit kernel.
//
// A refit keeps the topology, the primitive ids and each record's leaf slot, so the triangle a pixel
// hit is found again in a copy taken before the update:
//   k_motion_snapshot   one lane per leaf slot: the record's v0, e1, e2 and its triangle's face normal
//                       to snap[original index], the slot to slot_of[original index]
//   k_motion_reproject  one lane per planar hit record: the hit point's coordinates (u, v) on the
//                       resident triangle, carried to the snapshot's triangle; a record that hit no
//                       triangle, or a triangle equal to its snapshot, passes through bit for bit
// The arithmetic is the specification's, operation by operation (tests/motion_restatement.py is the
// same in numpy, and the outputs are equal bit for bit): binary32, no fused multiply-add
// (-ffp-contract=off), the compiler's correctly rounded division, denormals kept.  No atomics, no LDS,
// no scratch; every index is checked against the scene's counts before it is used.
#include "wgt_motion.h"

#include "wgt_geom.h"

namespace wgt {

namespace {

constexpr int kMotionBlock = 256;
constexpr uint32_t kTriFloat4s = kTriRecordFloats / 4;

__device__ __forceinline__ f3 load_planar(const float* __restrict__ p, uint32_t n, uint32_t i) {
  return f3{p[i], p[(size_t)n + i], p[2 * (size_t)n + i]};
}
__device__ __forceinline__ void store_planar(float* __restrict__ p, uint32_t n, uint32_t i, f3 v) {
  p[i] = v.x;
  p[(size_t)n + i] = v.y;
  p[2 * (size_t)n + i] = v.z;
}
__device__ __forceinline__ bool same(f3 a, f3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

__global__ void __launch_bounds__(kMotionBlock)
k_motion_snapshot(const float4* __restrict__ tris, const float4* __restrict__ tshade, uint32_t n_tris,
                  float4* __restrict__ snap, uint32_t* __restrict__ slot_of) {
  const uint32_t s = blockIdx.x * kMotionBlock + threadIdx.x;
  if (s >= n_tris) return;
  const float4* rec = tris + (size_t)s * kTriFloat4s;
  const float4 a = rec[0], b = rec[1], c = rec[2];
  const uint32_t orig = __float_as_uint(a.w);
  if (orig >= n_tris) return;  // never: the upload's records hold a permutation of 0..n_tris-1
  const float4 fn = tshade[(size_t)orig * 2];
  float4* out = snap + (size_t)orig * kMotionSnapFloat4s;
  out[0] = make_float4(a.x, a.y, a.z, b.x);
  out[1] = make_float4(b.y, b.z, c.x, c.y);
  out[2] = make_float4(c.z, fn.x, fn.y, fn.z);
  slot_of[orig] = s;
}

// What every lane is given (kernel argument).
struct ReprojectArgs {
  const float4* tris;
  const float4* tshade;
  const float4* snap;
  const uint32_t* slot_of;
  uint32_t nlq, n_tris, n;
  const uint32_t* prim;
  const float* pos;
  const float* norm;
  const uint8_t* flags;
  float* pos_prev;
  float* norm_prev;
};

__global__ void __launch_bounds__(kMotionBlock) k_motion_reproject(ReprojectArgs a) {
  const uint32_t i = blockIdx.x * kMotionBlock + threadIdx.x;
  if (i >= a.n) return;
  const uint32_t prim = a.prim[i];
  const f3 pos = load_planar(a.pos, a.n, i), norm = load_planar(a.norm, a.n, i);
  f3 pp = pos, np = norm;  // not a triangle hit, or an unmoved triangle: as they came
  const uint32_t t = prim - a.nlq;
  if (prim >= a.nlq && t < a.n_tris) {
    const uint32_t s = a.slot_of[t];
    if (s < a.n_tris) {
      const float4* rec = a.tris + (size_t)s * kTriFloat4s;
      const float4 ra = rec[0], rb = rec[1], rc = rec[2], rf = a.tshade[(size_t)t * 2];
      const float4* sn = a.snap + (size_t)t * kMotionSnapFloat4s;
      const float4 s0 = sn[0], s1 = sn[1], s2 = sn[2];
      const f3 v0{ra.x, ra.y, ra.z}, e1{rb.x, rb.y, rb.z}, e2{rc.x, rc.y, rc.z}, fn{rf.x, rf.y, rf.z};
      const f3 pv0{s0.x, s0.y, s0.z}, pe1{s0.w, s1.x, s1.y}, pe2{s1.z, s1.w, s2.x}, pfn{s2.y, s2.z, s2.w};
      if (!(same(v0, pv0) && same(e1, pe1) && same(e2, pe2))) {
        const f3 d = pos - v0;
        const f3 nv = cross(e1, e2);
        const float nf = dot(nv, fn);
        const float u = dot(cross(d, e2), fn) / nf;
        const float v = dot(cross(e1, d), fn) / nf;
        pp = (pv0 + u * pe1) + v * pe2;
        np = (a.flags[i] & WGT_HIT_FRONT_FACE) ? pfn : -pfn;
      }
    }
  }
  store_planar(a.pos_prev, a.n, i, pp);
  store_planar(a.norm_prev, a.n, i, np);
}

}  // namespace

hipError_t launch_motion_snapshot(const DevScene& sc, float4* snap, uint32_t* slot_of, hipStream_t stream) {
  if (sc.n_tris == 0 || !sc.tris || !sc.tshade || !snap || !slot_of) return hipErrorInvalidValue;
  const uint32_t blocks = (sc.n_tris + kMotionBlock - 1) / kMotionBlock;
  k_motion_snapshot<<<blocks, kMotionBlock, 0, stream>>>(sc.tris, sc.tshade, sc.n_tris, snap, slot_of);
  return hipGetLastError();
}

hipError_t launch_motion_reproject(const DevScene& sc, const float4* snap, const uint32_t* slot_of, uint32_t n,
                                   const wgt_hit_buffers& g, const wgt_motion_buffers& out, hipStream_t stream) {
  // the callers' checks hold these: the kernel indexes in 32 bits and dereferences what it is given
  if (n == 0 || n > kMotionMaxRecords || sc.n_tris == 0 || !sc.tris || !sc.tshade || !snap || !slot_of)
    return hipErrorInvalidValue;
  if (!g.prim || !g.pos || !g.norm || !g.flags || !out.pos_prev || !out.norm_prev) return hipErrorInvalidValue;
  ReprojectArgs a{};
  a.tris = sc.tris;
  a.tshade = sc.tshade;
  a.snap = snap;
  a.slot_of = slot_of;
  a.nlq = sc.n_lights + sc.n_quads;
  a.n_tris = sc.n_tris;
  a.n = n;
  a.prim = g.prim;
  a.pos = g.pos;
  a.norm = g.norm;
  a.flags = g.flags;
  a.pos_prev = out.pos_prev;
  a.norm_prev = out.norm_prev;
  k_motion_reproject<<<(n + kMotionBlock - 1) / kMotionBlock, kMotionBlock, 0, stream>>>(a);
  return hipGetLastError();
}

}  // namespace wgt
