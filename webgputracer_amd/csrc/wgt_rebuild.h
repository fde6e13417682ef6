// wgt_rebuild.h — the rebuild of the triangle BVH on the device (wgt_rebuild_triangles, DESIGN.md
// §4.12): what the runtime TU and wgt_rebuild.hip share.  The topology is host/bvh.cpp
// BuildMortonBvh's, made with wgt_morton.h's operations; the boxes, records and compact codes are
// then the refit's (wgt_refit.hip), unchanged.
#pragma once

#include "wgt_internal.h"
#include "wgt_morton.h"

namespace wgt {

// The centres' bounds per axis as order-preserving bits of the floats (float_order): unsigned
// integer min and max order as the values do.  lo starts at all ones, hi at zero.
struct RebuildBounds {
  uint32_t lo[3], hi[3];
  uint32_t pad[2];
};
// The counts of the tree, reduced over the levels (zero before the first): exact integer maxima and a sum.
struct RebuildStats {
  uint32_t stack_need, n_leaves, max_leaf, pad;
};
// A node still to be made: the keys [b, e) with r binary levels left, and the stack entries the
// path from the root to its parent pushes (the sum of slots - 1).
struct RebuildRange {
  uint32_t b, e, r, path;
};

// A tree under construction: sc's tree parts are writable here and nowhere else.
struct RebuildTree {
  float4* nodes;
  float4* tris;
  uint4* crecs;
  uint8_t* node_level;
  uint32_t n_tris, node_cap, leaf;
};

// Launchers implemented in wgt_rebuild.hip, in this order on one stream.
// rocprim's temporary storage for a sort of n keys and a scan of up to rebuild_node_cap(n) + 1 counts.
hipError_t rebuild_temp_bytes(uint32_t n_tris, uint32_t node_cap, size_t& bytes);
// *d_bounds (lo all ones, hi zero before the launch) = the centres' exact bounds.
hipError_t launch_rebuild_bounds(const wgt_triangle* d_tris, uint32_t n_tris, RebuildBounds* d_bounds, hipStream_t stream);
// key[i] = triangle i's code between those bounds, val[i] = i.
hipError_t launch_rebuild_keys(const wgt_triangle* d_tris, uint32_t n_tris, const RebuildBounds* d_bounds,
                               unsigned long long* d_key, uint32_t* d_val, hipStream_t stream);
// (key_out, val_out) = the pairs ascending by key, equal keys in their order (a stable radix sort).
hipError_t launch_rebuild_sort(void* d_temp, size_t temp_bytes, const unsigned long long* d_key_in,
                               unsigned long long* d_key_out, const uint32_t* d_val_in, uint32_t* d_val_out,
                               uint32_t n_tris, hipStream_t stream);
// The single-leaf root of n_tris <= leaf triangles, and its records' original indices.
hipError_t launch_rebuild_single(const RebuildTree& t, const uint32_t* d_val, hipStream_t stream);
// One level of `count` nodes d_list: their cuts (d_cuts[j] = cut 1..3 and the slot count) and
// d_count[j] = their internal slots, d_count[count] = 0.
hipError_t launch_rebuild_count(const unsigned long long* d_code, const RebuildRange* d_list, uint32_t count,
                                uint32_t leaf, uint4* d_cuts, uint32_t* d_count, hipStream_t stream);
// d_offset[0 .. count] = the exclusive sums of d_count[0 .. count]: d_offset[count] is the next level's size.
hipError_t launch_rebuild_scan(void* d_temp, size_t temp_bytes, const uint32_t* d_count, uint32_t* d_offset,
                               uint32_t count, hipStream_t stream);
// The level's nodes first .. first + count at `level`: refs in device-image form, empty slots padded,
// node_level, the records' original indices of leaf slots, the next level's list (its node first +
// count + d_offset[j] + the slot's place among the node's internal slots), and the counts into d_stats.
hipError_t launch_rebuild_write(const RebuildTree& t, const RebuildRange* d_list, const uint4* d_cuts,
                                const uint32_t* d_offset, const uint32_t* d_val, uint32_t first, uint32_t count,
                                uint32_t level, RebuildRange* d_next, RebuildStats* d_stats, hipStream_t stream);
// d_order[i] = i for i < n: the refit's level lists of a tree numbered breadth-first.
hipError_t launch_rebuild_iota(uint32_t* d_order, uint32_t n, hipStream_t stream);

}  // namespace wgt
