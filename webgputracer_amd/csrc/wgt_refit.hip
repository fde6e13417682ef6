// wgt_refit.hip — refit of the resident BVH to moved triangles (wgt_update_triangles), in a
// translation unit of its own: nothing here is read by a render or query kernel.
//
// The tree's topology stays, so the kernel forms, LDS sizes and refs do too; what depends on
// coordinates is recomputed with the host builder's own operations (host/bvh.cpp RefitBvh is the
// specification, and tests compare the device tree with it bit for bit):
//   k_refit_tris     the 64-B records (tri_box, wgt_geom.h) and the 32-B shading records
//   k_refit_verts    the same from moved vertices (wgt_update_vertices_device): the records and face normals
//                    as wgt_make_triangles builds them, the shading records' colour and emissive flag kept
//   k_refit_nodes    the 128-B nodes' boxes, one launch per tree level, deepest first: exact
//                    min/max unions, so neither the order of lanes nor of operands matters
//   k_refit_step     each node's smallest feasible step exponent (wgt_compact.h), one integer max
//   k_refit_compact  the 64-B node part of the 80-B records, wgt_compact.h's f64 arithmetic
// The runtime reads the root node back between the node and step kernels (the codes' margin
// follows from it, launch_plan.h compact_bound) and the exponent before the last one.
// Moved triangles in device memory are checked first by k_check_tris or k_check_verts: the host's
// limit check and scene_extent as two exact reductions, before any resident word is written.
#include "wgt_compact.h"
#include "wgt_internal.h"

namespace wgt {

namespace {

constexpr int kRefitBlock = 256;
constexpr uint32_t kNodeFloat4s = kNode4Floats / 4;
constexpr uint32_t kTriFloat4s = kTriRecordFloats / 4;

// The six plane rows of a node as 24 floats in wgt_compact.h's order.
__device__ __forceinline__ void load_rows(const float4* __restrict__ node, float* n) {
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    const float4 v = node[r];
    n[4 * r + 0] = v.x; n[4 * r + 1] = v.y; n[4 * r + 2] = v.z; n[4 * r + 3] = v.w;
  }
}

// Lane i rewrites leaf-ordered record i, which keeps its original index idx, from moved[idx], and
// that triangle's shading record (each original index occurs in exactly one record).
__global__ void __launch_bounds__(kRefitBlock)
k_refit_tris(float4* __restrict__ tris, float4* __restrict__ tshade, const float4* __restrict__ moved, uint32_t n_tris) {
  const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
  if (i >= n_tris) return;
  float4* rec = tris + (size_t)i * kTriFloat4s;
  const uint32_t idx = __float_as_uint(rec[0].w);
  if (idx >= n_tris) return;  // never: the upload's records hold a permutation of 0..n_tris-1
  const float4* t = moved + (size_t)idx * 5;  // wgt_triangle: v0, e1, e2, face_norm, (col, emissive)
  const float4 v0 = t[0], e1 = t[1], e2 = t[2], fn = t[3], ce = t[4];
  f3 lo, hi;
  tri_box(f3{v0.x, v0.y, v0.z}, f3{e1.x, e1.y, e1.z}, f3{e2.x, e2.y, e2.z}, lo, hi);
  rec[0] = make_float4(v0.x, v0.y, v0.z, __uint_as_float(idx));
  rec[1] = make_float4(e1.x, e1.y, e1.z, lo.x);
  rec[2] = make_float4(e2.x, e2.y, e2.z, lo.y);
  rec[3] = make_float4(lo.z, hi.x, hi.y, hi.z);
  tshade[(size_t)idx * 2] = make_float4(fn.x, fn.y, fn.z, ce.w);
  tshade[(size_t)idx * 2 + 1] = make_float4(ce.x, ce.y, ce.z, 0.0f);
}

// The Moller-Trumbore inputs of triangle t of moved vertices, as the host builds them
// (wgt_make_triangles without a translation: Vertex::Translate adds +0, which turns a -0
// coordinate into +0; then triangle.cpp's e1 = v1 - v0, e2 = v2 - v0).  False, and no vertex
// loaded, when an index is not below n_verts; t < n_tris.  The 36-B stride is read as dwords.
__device__ __forceinline__ bool gather_tri(const MovedVerts& in, uint32_t t, f3& v0, f3& e1, f3& e2) {
  uint32_t k[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint64_t at = (uint64_t)t * 3u + (uint32_t)c;
    const uint64_t v = in.index ? (uint64_t)in.index[at] : at;
    if (v >= in.n_verts) return false;
    k[c] = (uint32_t)v;
  }
  f3 p[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* v = in.verts + (size_t)k[c] * 3;
    p[c] = f3{v[0] + 0.0f, v[1] + 0.0f, v[2] + 0.0f};
  }
  v0 = p[0];
  e1 = p[1] - p[0];
  e2 = p[2] - p[0];
  return true;
}

// Lane i rewrites leaf-ordered record i as k_refit_tris does, from the vertices of its triangle idx,
// and the first half of that triangle's shading record: the face normal in include/wgt/vec.h's
// operations and order (glm::normalize(glm::cross(e1, e2)): cross, dot, 1 / sqrt, scale; a
// zero-area triangle's is NaN) beside the emissive flag it read there.  The colour half stays.
__global__ void __launch_bounds__(kRefitBlock)
k_refit_verts(float4* __restrict__ tris, float4* __restrict__ tshade, MovedVerts in) {
  const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
  if (i >= in.n_tris) return;
  float4* rec = tris + (size_t)i * kTriFloat4s;
  const uint32_t idx = __float_as_uint(rec[0].w);
  if (idx >= in.n_tris) return;  // never: the upload's records hold a permutation of 0..n_tris-1
  f3 v0, e1, e2;
  if (!gather_tri(in, idx, v0, e1, e2)) return;  // never: the check pass refused such an index
  f3 lo, hi;
  tri_box(v0, e1, e2, lo, hi);
  const f3 c = cross(e1, e2);
  const float inv = 1.0f / sqrt_rn(dot(c, c));
  rec[0] = make_float4(v0.x, v0.y, v0.z, __uint_as_float(idx));
  rec[1] = make_float4(e1.x, e1.y, e1.z, lo.x);
  rec[2] = make_float4(e2.x, e2.y, e2.z, lo.y);
  rec[3] = make_float4(lo.z, hi.x, hi.y, hi.z);
  float4* sh = tshade + (size_t)idx * 2;
  const float emissive = sh[0].w;
  sh[0] = make_float4(c.x * inv, c.y * inv, c.z * inv, emissive);
}

// The check of moved triangles before a refit from device memory.  One triangle's terms: bad = its
// index when check_scene_limits refuses it (v0, e1, e2 finite and within 2^40, edge components
// within 2^30; NaN fails every comparison), else kNoBadTriangle; ext = the bits of its term of
// scene_extent in f64, 0 for a refused one (the extent is not used then).
__device__ __forceinline__ unsigned long long abs_bits(double x) {
  return (unsigned long long)__double_as_longlong(__builtin_fabs(x));
}
__device__ __forceinline__ unsigned long long max_u64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
__device__ __forceinline__ void check_term(uint32_t i, f3 v0, f3 e1, f3 e2, uint32_t& bad, unsigned long long& ext) {
  const float v[3] = {v0.x, v0.y, v0.z}, a[3] = {e1.x, e1.y, e1.z}, b[3] = {e2.x, e2.y, e2.z};
  const float coord = (float)kCoordLimit, edge = (float)kEdgeLimit;  // powers of two: exact
  bool ok = true;
  unsigned long long m = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    ok = ok && __builtin_fabsf(v[c]) <= coord && __builtin_fabsf(a[c]) <= edge && __builtin_fabsf(b[c]) <= edge;
    const double d = v[c];
    m = max_u64(max_u64(m, abs_bits(d)), max_u64(abs_bits(d + a[c]), abs_bits(d + b[c])));
  }
  bad = ok ? kNoBadTriangle : i;
  ext = ok ? m : 0ull;
}
// ... reduced over the wave, then one vector atomic each per wave that has something to say:
// an integer min and an integer max, so the result does not depend on any order.  Every lane of
// the block calls it (lanes past the end with kNoBadTriangle and 0).
__device__ __forceinline__ void check_reduce(uint32_t bad, unsigned long long ext, RefitCheck* __restrict__ out) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    bad = min(bad, (uint32_t)__shfl_xor((int)bad, off, 64));
    ext = max_u64(ext, __shfl_xor(ext, off, 64));
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (bad != kNoBadTriangle) atomicMin(&out->first_bad, bad);
    if (ext != 0ull) atomicMax(&out->extent_bits, ext);
  }
}

__global__ void __launch_bounds__(kRefitBlock)
k_check_tris(const float4* __restrict__ moved, uint32_t n_tris, RefitCheck* __restrict__ out) {
  const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
  uint32_t bad = kNoBadTriangle;
  unsigned long long ext = 0;
  if (i < n_tris) {
    const float4* t = moved + (size_t)i * 5;
    const float4 v0 = t[0], e1 = t[1], e2 = t[2];
    check_term(i, f3{v0.x, v0.y, v0.z}, f3{e1.x, e1.y, e1.z}, f3{e2.x, e2.y, e2.z}, bad, ext);
  }
  check_reduce(bad, ext, out);
}

// The vertex form checks the record k_refit_verts will build; an index not below n_verts fails too.
__global__ void __launch_bounds__(kRefitBlock) k_check_verts(MovedVerts in, RefitCheck* __restrict__ out) {
  const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
  uint32_t bad = kNoBadTriangle;
  unsigned long long ext = 0;
  if (i < in.n_tris) {
    f3 v0, e1, e2;
    if (gather_tri(in, i, v0, e1, e2)) check_term(i, v0, e1, e2, bad, ext);
    else bad = i;
  }
  check_reduce(bad, ext, out);
}

// Lane j refits node order[j] of one level: a leaf slot's box is the union of its triangles'
// record boxes, an internal slot's the union of the live slots of the node it points to (one
// level down: refit by the previous launch).  Empty slots and refs stay.
__global__ void __launch_bounds__(kRefitBlock)
k_refit_nodes(float4* __restrict__ nodes, const float4* __restrict__ tris, const uint32_t* __restrict__ order,
              uint32_t count, uint32_t n_nodes, uint32_t n_tris) {
  const uint32_t j = blockIdx.x * kRefitBlock + threadIdx.x;
  if (j >= count) return;
  const uint32_t k = order[j];
  if (k >= n_nodes) return;  // never
  float4* node = nodes + (size_t)k * kNodeFloat4s;
  float n[24];
  load_rows(node, n);
  const float4 refs4 = node[6];
  const int refs[kBvhWidth] = {__float_as_int(refs4.x), __float_as_int(refs4.y), __float_as_int(refs4.z),
                               __float_as_int(refs4.w)};
#pragma unroll
  for (int s = 0; s < kBvhWidth; ++s) {
    if (!node_live(n, s)) continue;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    const int r = refs[s];
    if (r < 0) {
      const uint32_t first = leaf_first(r), cnt = leaf_count(r);
      if ((uint64_t)first + cnt > n_tris) continue;  // never: CheckRefs
      for (uint32_t t = 0; t < cnt; ++t) {
        const float4* rec = tris + (size_t)(first + t) * kTriFloat4s;
        const float lx = rec[1].w, ly = rec[2].w;
        const float4 d = rec[3];
        lo[0] = fminf(lo[0], lx); lo[1] = fminf(lo[1], ly); lo[2] = fminf(lo[2], d.x);
        hi[0] = fmaxf(hi[0], d.y); hi[1] = fmaxf(hi[1], d.z); hi[2] = fmaxf(hi[2], d.w);
      }
    } else {
      const uint32_t child = (uint32_t)r / (uint32_t)(kNode4Floats * 4);  // a byte offset in the device image
      if (child >= n_nodes) continue;  // never: CheckRefs
      float c[24];
      load_rows(nodes + (size_t)child * kNodeFloat4s, c);
#pragma unroll
      for (int cs = 0; cs < kBvhWidth; ++cs)
        if (node_live(c, cs)) {
#pragma unroll
          for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], node_lo(c, a, cs));
            hi[a] = fmaxf(hi[a], node_hi(c, a, cs));
          }
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      n[(2 * a) * 4 + s] = lo[a];
      n[(2 * a + 1) * 4 + s] = hi[a];
    }
  }
#pragma unroll
  for (int r = 0; r < 6; ++r) node[r] = make_float4(n[4 * r], n[4 * r + 1], n[4 * r + 2], n[4 * r + 3]);
}

// *max_exp = the largest, over the nodes, of compact_node_exp - kCompactMinExp (zeroed before the
// launch): one atomic per wave.
__global__ void __launch_bounds__(kRefitBlock)
k_refit_step(const float4* __restrict__ nodes, uint32_t n_nodes, double G, uint32_t* __restrict__ max_exp) {
  const uint32_t k = blockIdx.x * kRefitBlock + threadIdx.x;
  int e = 0;
  if (k < n_nodes) {
    float n[24];
    load_rows(nodes + (size_t)k * kNodeFloat4s, n);
    e = compact_node_exp(n, G) - kCompactMinExp;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) e = max(e, __shfl_xor(e, off, 64));
  if ((threadIdx.x & 63u) == 0u && e > 0) atomicMax(max_exp, (uint32_t)e);
}

// Lane k writes the node part (64 B) of compact record k; the record's refs stay.
__global__ void __launch_bounds__(kRefitBlock)
k_refit_compact(const float4* __restrict__ nodes, uint4* __restrict__ crecs, uint32_t n_nodes, float step, double G) {
  const uint32_t k = blockIdx.x * kRefitBlock + threadIdx.x;
  if (k >= n_nodes) return;
  float n[24];
  load_rows(nodes + (size_t)k * kNodeFloat4s, n);
  uint32_t q[kCNodeFloats];
  compact_node(n, step, G, q);
  uint4* rec = crecs + (size_t)k * kCRecordFloat4s;
#pragma unroll
  for (int r = 0; r < kCNodeFloats / 4; ++r) rec[r] = make_uint4(q[4 * r], q[4 * r + 1], q[4 * r + 2], q[4 * r + 3]);
}

dim3 refit_grid(uint32_t n) { return dim3((n + kRefitBlock - 1) / kRefitBlock); }

}  // namespace

// The scene's tree parts are written here and nowhere else after the upload; the caller has
// waited for every launch that reads them (wgt_update_triangles).
hipError_t launch_refit_tris(const DevScene& sc, const wgt_triangle* d_moved, hipStream_t stream) {
  if (sc.n_tris == 0) return hipSuccess;
  k_refit_tris<<<refit_grid(sc.n_tris), kRefitBlock, 0, stream>>>((float4*)sc.tris, (float4*)sc.tshade,
                                                                  (const float4*)d_moved, sc.n_tris);
  return hipGetLastError();
}

hipError_t launch_refit_verts(const DevScene& sc, const MovedVerts& in, hipStream_t stream) {
  if (in.n_tris != sc.n_tris) return hipErrorInvalidValue;  // never: the call's argument checks
  if (sc.n_tris == 0) return hipSuccess;
  k_refit_verts<<<refit_grid(sc.n_tris), kRefitBlock, 0, stream>>>((float4*)sc.tris, (float4*)sc.tshade, in);
  return hipGetLastError();
}

hipError_t launch_check_tris(const wgt_triangle* d_moved, uint32_t n_tris, RefitCheck* d_out, hipStream_t stream) {
  if (n_tris == 0) return hipSuccess;
  k_check_tris<<<refit_grid(n_tris), kRefitBlock, 0, stream>>>((const float4*)d_moved, n_tris, d_out);
  return hipGetLastError();
}

hipError_t launch_check_verts(const MovedVerts& in, RefitCheck* d_out, hipStream_t stream) {
  if (in.n_tris == 0) return hipSuccess;
  k_check_verts<<<refit_grid(in.n_tris), kRefitBlock, 0, stream>>>(in, d_out);
  return hipGetLastError();
}

hipError_t launch_refit_nodes(const DevScene& sc, const uint32_t* d_order, uint32_t count, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  k_refit_nodes<<<refit_grid(count), kRefitBlock, 0, stream>>>((float4*)sc.nodes, sc.tris, d_order, count, sc.n_nodes,
                                                               sc.n_tris);
  return hipGetLastError();
}

hipError_t launch_refit_step(const DevScene& sc, double G, uint32_t* d_max_exp, hipStream_t stream) {
  if (sc.n_nodes == 0) return hipSuccess;
  k_refit_step<<<refit_grid(sc.n_nodes), kRefitBlock, 0, stream>>>(sc.nodes, sc.n_nodes, G, d_max_exp);
  return hipGetLastError();
}

hipError_t launch_refit_compact(const DevScene& sc, float step, double G, hipStream_t stream) {
  if (sc.n_nodes == 0) return hipSuccess;
  k_refit_compact<<<refit_grid(sc.n_nodes), kRefitBlock, 0, stream>>>(sc.nodes, (uint4*)sc.cnodes, sc.n_nodes, step, G);
  return hipGetLastError();
}

}  // namespace wgt
