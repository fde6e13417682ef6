// wgt_rebuild.hip — the topology of a rebuilt triangle BVH, made on the device (wgt_rebuild_triangles,
// DESIGN.md §4.12), in a translation unit of its own: nothing here is read by a render or query kernel.
//
// host/bvh.cpp BuildMortonBvh is the specification, and tests compare the device tree with it bit for
// bit.  Every step is exact or order-free, so the result does not depend on the order of lanes:
//   k_rb_bounds  the centres' bounds: integer min/max atomics on order-preserving float bits, one per
//                wave after a butterfly
//   k_rb_keys    the 63-bit codes (wgt_morton.h, the host's own inline function) and the indices
//   rocprim      a stable radix sort of (code, index) pairs: ascending by (code, original index)
//   per level    k_rb_count: one lane per node, its three splits by binary search and its internal slots;
//                an exclusive scan, which numbers the children; k_rb_write: refs, padding, node
//                levels, the records' original indices, the next level's list, the counts
// The refit kernels (wgt_refit.hip) then compute the boxes, records and compact codes, unchanged.
#include <cstring>  // before rocprim: its headers use std::memcpy without including it

#include <rocprim/rocprim.hpp>

#include "wgt_rebuild.h"

namespace wgt {

namespace {

constexpr int kRbBlock = 256;
constexpr uint32_t kNodeFloat4s = kNode4Floats / 4;
constexpr uint32_t kTriFloat4s = kTriRecordFloats / 4;

dim3 rb_grid(uint32_t n) { return dim3((n + kRbBlock - 1) / kRbBlock); }

// Unsigned integers that order as the (non-NaN) floats do, and back.
__device__ __forceinline__ uint32_t float_order(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__device__ __forceinline__ float order_float(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? u & 0x7fffffffu : ~u);
}

// The centre of triangle i's padded box, as BuildMortonBvh takes it.
__device__ __forceinline__ void centre_of(const float4* __restrict__ moved, uint32_t i, float* c) {
  const float4* t = moved + (size_t)i * 5;
  const float4 v0 = t[0], e1 = t[1], e2 = t[2];
  f3 lo, hi;
  tri_box(f3{v0.x, v0.y, v0.z}, f3{e1.x, e1.y, e1.z}, f3{e2.x, e2.y, e2.z}, lo, hi);
  c[0] = morton_centre(lo.x, hi.x);
  c[1] = morton_centre(lo.y, hi.y);
  c[2] = morton_centre(lo.z, hi.z);
}

// Every lane of the block takes part (lanes past the end with the reductions' neutral values).
__global__ void __launch_bounds__(kRbBlock)
k_rb_bounds(const float4* __restrict__ moved, uint32_t n_tris, RebuildBounds* __restrict__ out) {
  const uint32_t i = blockIdx.x * kRbBlock + threadIdx.x;
  uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  if (i < n_tris) {
    float c[3];
    centre_of(moved, i, c);
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = float_order(c[a]);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], off, 64));
      hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], off, 64));
    }
  }
  if ((threadIdx.x & 63u) == 0u && hi[0] != 0u) {  // a wave with a triangle
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&out->lo[a], lo[a]);
      atomicMax(&out->hi[a], hi[a]);
    }
  }
}

__global__ void __launch_bounds__(kRbBlock)
k_rb_keys(const float4* __restrict__ moved, uint32_t n_tris, const RebuildBounds* __restrict__ bounds,
          unsigned long long* __restrict__ key, uint32_t* __restrict__ val) {
  const uint32_t i = blockIdx.x * kRbBlock + threadIdx.x;
  if (i >= n_tris) return;
  float c[3];
  centre_of(moved, i, c);
  uint32_t q[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) q[a] = morton_cell(c[a], order_float(bounds->lo[a]), order_float(bounds->hi[a]));
  key[i] = morton_code(q[0], q[1], q[2]);
  val[i] = i;
}

// Node k of the tree under construction: its slots' refs, `live` of them live (boxes 0 until the
// refit, so that node_live holds), the rest empty as EmitNode pads them; and its level.
__device__ __forceinline__ void write_node(const RebuildTree& t, uint32_t k, const int* nref, const int* cref, int live,
                                           uint32_t level) {
  float4* node = t.nodes + (size_t)k * kNodeFloat4s;
  const float e = kEmptySlotCoord;
  const float4 row = make_float4(0.0f, live > 1 ? 0.0f : e, live > 2 ? 0.0f : e, live > 3 ? 0.0f : e);
#pragma unroll
  for (int r = 0; r < 6; ++r) node[r] = row;
  int a[kBvhWidth], b[kBvhWidth];
#pragma unroll
  for (int s = 0; s < kBvhWidth; ++s) {
    a[s] = s < live ? nref[s] : nref[0];
    b[s] = s < live ? cref[s] : cref[0];
  }
  node[6] = make_float4(__int_as_float(a[0]), __int_as_float(a[1]), __int_as_float(a[2]), __int_as_float(a[3]));
  node[7] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  t.crecs[(size_t)k * kCRecordFloat4s + kCNodeFloats / 4] = make_uint4((uint32_t)b[0], (uint32_t)b[1], (uint32_t)b[2], (uint32_t)b[3]);
  t.node_level[k] = (uint8_t)level;
}

// The original indices of the leaf-ordered records [b, e): word 3, which the refit reads.
__device__ __forceinline__ void write_leaf_indices(const RebuildTree& t, const uint32_t* __restrict__ val, uint32_t b, uint32_t e) {
  for (uint32_t i = b; i < e && i < t.n_tris; ++i)
    reinterpret_cast<uint32_t*>(t.tris + (size_t)i * kTriFloat4s)[3] = val[i];
}

__global__ void k_rb_single(RebuildTree t, const uint32_t* __restrict__ val) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || t.n_tris == 0 || t.n_tris > (uint32_t)kLeafMax || t.node_cap == 0) return;
  const int ref[kBvhWidth] = {leaf_ref(0u, t.n_tris), 0, 0, 0};
  write_node(t, 0u, ref, ref, 1, 0u);
  write_leaf_indices(t, val, 0u, t.n_tris);
}

__global__ void __launch_bounds__(kRbBlock)
k_rb_count(const unsigned long long* __restrict__ code, const RebuildRange* __restrict__ list, uint32_t count,
           uint32_t leaf, uint4* __restrict__ cuts, uint32_t* __restrict__ n_internal) {
  const uint32_t j = blockIdx.x * kRbBlock + threadIdx.x;
  if (j > count) return;
  if (j == count) {  // the scan's last input: its output there is the level's total
    n_internal[j] = 0u;
    return;
  }
  const RebuildRange g = list[j];
  uint32_t cut[kBvhWidth + 1] = {g.b, g.e, g.e, g.e, g.e};
  const int slots = morton_slots(code, g.b, g.e, g.r, leaf, cut);
  uint32_t internal = 0;
#pragma unroll
  for (int s = 0; s < kBvhWidth; ++s)
    if (s < slots && cut[s + 1] - cut[s] > leaf) ++internal;
  cuts[j] = make_uint4(cut[1], cut[2], cut[3], (uint32_t)slots);
  n_internal[j] = internal;
}

__global__ void __launch_bounds__(kRbBlock)
k_rb_write(RebuildTree t, const RebuildRange* __restrict__ list, const uint4* __restrict__ cuts,
           const uint32_t* __restrict__ offset, const uint32_t* __restrict__ val, uint32_t first, uint32_t count,
           uint32_t level, RebuildRange* __restrict__ next, RebuildStats* __restrict__ stats) {
  const uint32_t j = blockIdx.x * kRbBlock + threadIdx.x;
  uint32_t path = 0, leaves = 0, max_leaf = 0;
  if (j < count && first + j < t.node_cap) {
    const RebuildRange g = list[j];
    const uint4 c = cuts[j];
    const uint32_t cut[kBvhWidth + 1] = {g.b, c.x, c.y, c.z, g.e};
    const int slots = (int)c.w;
    path = g.path + (uint32_t)(slots - 1);
    uint32_t child = offset[j];  // the place of this node's first internal slot in the next level
    int nref[kBvhWidth] = {0, 0, 0, 0}, cref[kBvhWidth] = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < kBvhWidth; ++s) {
      if (s >= slots) continue;
      const uint32_t b = cut[s], e = s + 1 == slots ? g.e : cut[s + 1], cnt = e - b;
      if (cnt <= t.leaf) {
        nref[s] = cref[s] = leaf_ref(b, cnt);
        write_leaf_indices(t, val, b, e);
        ++leaves;
        max_leaf = max(max_leaf, cnt);
      } else {
        const uint32_t k = first + count + child;
        if (k < t.node_cap) next[child] = RebuildRange{b, e, g.r - 2u, path};  // always: rebuild_node_cap
        nref[s] = (int)(k * (uint32_t)(kNode4Floats * 4));
        cref[s] = (int)(k * (uint32_t)(kCRecordFloat4s * 16));
        ++child;
      }
    }
    write_node(t, first + j, nref, cref, slots, level);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    path = max(path, (uint32_t)__shfl_xor((int)path, off, 64));
    max_leaf = max(max_leaf, (uint32_t)__shfl_xor((int)max_leaf, off, 64));
    leaves += (uint32_t)__shfl_xor((int)leaves, off, 64);
  }
  if ((threadIdx.x & 63u) == 0u && (path | leaves) != 0u) {
    atomicMax(&stats->stack_need, path);
    atomicMax(&stats->max_leaf, max_leaf);
    atomicAdd(&stats->n_leaves, leaves);
  }
}

__global__ void __launch_bounds__(kRbBlock) k_rb_iota(uint32_t* __restrict__ order, uint32_t n) {
  const uint32_t i = blockIdx.x * kRbBlock + threadIdx.x;
  if (i < n) order[i] = i;
}

}  // namespace

hipError_t rebuild_temp_bytes(uint32_t n_tris, uint32_t node_cap, size_t& bytes) {
  size_t sort = 0, scan = 0;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, sort, (const unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                           (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n_tris, 0u, 63u,
                                           (hipStream_t) nullptr);
  if (e != hipSuccess) return e;
  e = rocprim::exclusive_scan(nullptr, scan, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)node_cap + 1,
                              rocprim::plus<uint32_t>(), (hipStream_t) nullptr);
  bytes = sort > scan ? sort : scan;
  return e;
}

hipError_t launch_rebuild_bounds(const wgt_triangle* d_tris, uint32_t n_tris, RebuildBounds* d_bounds, hipStream_t stream) {
  if (n_tris == 0) return hipSuccess;
  k_rb_bounds<<<rb_grid(n_tris), kRbBlock, 0, stream>>>((const float4*)d_tris, n_tris, d_bounds);
  return hipGetLastError();
}

hipError_t launch_rebuild_keys(const wgt_triangle* d_tris, uint32_t n_tris, const RebuildBounds* d_bounds,
                               unsigned long long* d_key, uint32_t* d_val, hipStream_t stream) {
  if (n_tris == 0) return hipSuccess;
  k_rb_keys<<<rb_grid(n_tris), kRbBlock, 0, stream>>>((const float4*)d_tris, n_tris, d_bounds, d_key, d_val);
  return hipGetLastError();
}

hipError_t launch_rebuild_sort(void* d_temp, size_t temp_bytes, const unsigned long long* d_key_in,
                               unsigned long long* d_key_out, const uint32_t* d_val_in, uint32_t* d_val_out,
                               uint32_t n_tris, hipStream_t stream) {
  return rocprim::radix_sort_pairs(d_temp, temp_bytes, d_key_in, d_key_out, d_val_in, d_val_out, (size_t)n_tris, 0u, 63u,
                                   stream);
}

hipError_t launch_rebuild_single(const RebuildTree& t, const uint32_t* d_val, hipStream_t stream) {
  if (t.n_tris == 0 || t.n_tris > t.leaf || t.leaf > (uint32_t)kLeafMax) return hipErrorInvalidValue;  // never
  k_rb_single<<<1, 64, 0, stream>>>(t, d_val);
  return hipGetLastError();
}

hipError_t launch_rebuild_count(const unsigned long long* d_code, const RebuildRange* d_list, uint32_t count,
                                uint32_t leaf, uint4* d_cuts, uint32_t* d_count, hipStream_t stream) {
  k_rb_count<<<rb_grid(count + 1), kRbBlock, 0, stream>>>(d_code, d_list, count, leaf, d_cuts, d_count);
  return hipGetLastError();
}

hipError_t launch_rebuild_scan(void* d_temp, size_t temp_bytes, const uint32_t* d_count, uint32_t* d_offset,
                               uint32_t count, hipStream_t stream) {
  return rocprim::exclusive_scan(d_temp, temp_bytes, d_count, d_offset, 0u, (size_t)count + 1, rocprim::plus<uint32_t>(),
                                 stream);
}

hipError_t launch_rebuild_write(const RebuildTree& t, const RebuildRange* d_list, const uint4* d_cuts,
                                const uint32_t* d_offset, const uint32_t* d_val, uint32_t first, uint32_t count,
                                uint32_t level, RebuildRange* d_next, RebuildStats* d_stats, hipStream_t stream) {
  if (count == 0) return hipSuccess;
  if ((uint64_t)first + count > t.node_cap) return hipErrorInvalidValue;  // never: rebuild_node_cap
  k_rb_write<<<rb_grid(count), kRbBlock, 0, stream>>>(t, d_list, d_cuts, d_offset, d_val, first, count, level, d_next,
                                                      d_stats);
  return hipGetLastError();
}

hipError_t launch_rebuild_iota(uint32_t* d_order, uint32_t n, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  k_rb_iota<<<rb_grid(n), kRbBlock, 0, stream>>>(d_order, n);
  return hipGetLastError();
}

}  // namespace wgt
