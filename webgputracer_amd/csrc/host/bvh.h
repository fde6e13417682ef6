// bvh.h — host BVH builder (binned SAH) producing the device layout of
// wgt_internal.h / wgt_geom.h.  New component: the reference has no BVH
// (SURVEY §0.2); the build is specified by DESIGN.md §3.4 / §4.2.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/wgt_api.h"
#include "../wgt_geom.h"

namespace wgt {

// Every parameter of a build.  The defaults are the product's (launch_plan.cpp checks the
// first two against wgt_internal.h); BvhOptionsFromEnv is the one reader of the knobs.
struct BvhOptions {
  uint32_t max_depth = 24;  // of the SAH BVH2: bounds the BVH4's depth and so the traversal stack
  // bounds stack_need: the collapse narrows stack-heavy nodes to meet it, and a BVH2 higher
  // than the limit (a 2-wide node pushes one entry per level) fails the build
  uint32_t stack_limit = 31;
  // > 0: the BVH2 is also collapsed under this smaller stack bound, and that tree is kept (BvhOut::narrow) if it
  // costs at most narrow_ratio times the wide one (SAH cost of the optimal trees, node count of the greedy ones)
  uint32_t narrow_limit = 0;
  double narrow_ratio = 1.03;
  // an upper bound on |coordinate| of every ray origin the compact nodes will see (camera and hit points); the
  // margin of their codes grows with it (CompactNode), and a camera beyond BvhOut::cbound reads the 128-B nodes
  double origin_bound = 0.0;
  int sah_bins = 128;          // SAH bins per axis, 2..256
  double sah_trav = 1.0;       // SAH cost of a BVH2 node visit (a triangle test costs 1)
  uint32_t sah_leaf = kLeafMax;  // the largest leaf the SAH may choose, 1..kLeafMax
  double dp_node = 1.0, dp_tri = 1.0;  // the optimal collapse's node-visit and triangle-test weights
  uint32_t dp_leaf = 0;  // the largest leaf it may make of a BVH2 subtree, 0..kLeafMax (0 keeps the BVH2 leaves)
  enum Collapse { kOptimal, kGreedy } collapse = kOptimal;
};

// The options of a build as an upload makes it: the caller's limits (stack_narrow is the bound
// WGT_NARROW turns on) and the defaults above, overridden by the environment's tuning knobs.
BvhOptions BvhOptionsFromEnv(uint32_t max_depth, uint32_t stack_max, uint32_t stack_narrow, double origin_bound);

// One 128-B BVH4 node (wgt_geom.h): children in SoA order, plane rows lo.x hi.x lo.y hi.y lo.z
// hi.z, then the refs, then a zero row.  F = float or const float.
template <class F>
struct Node4T {
  F* n;
  F& lo(int axis, int slot) const { return n[(2 * axis) * 4 + slot]; }
  F& hi(int axis, int slot) const { return n[(2 * axis + 1) * 4 + slot]; }
  int32_t ref(int slot) const { int32_t r; std::memcpy(&r, &n[24 + slot], 4); return r; }
  void set_ref(int slot, int32_t r) const { std::memcpy(&n[24 + slot], &r, 4); }
  F& pad(int slot) const { return n[28 + slot]; }
  bool live(int slot) const { return !(lo(0, slot) == kEmptySlotCoord && hi(0, slot) == kEmptySlotCoord); }
};
inline Node4T<float> Node4(std::vector<float>& nodes, size_t i) { return {&nodes[i * kNode4Floats]}; }
inline Node4T<const float> Node4(const std::vector<float>& nodes, size_t i) { return {&nodes[i * kNode4Floats]}; }

struct BvhOut {
  std::vector<float> nodes;   // kNode4Floats per BVH4 node (Node4), root = 0
  std::vector<uint32_t> cnodes;  // kCNodeFloats words per node: the compact form (wgt_geom.h)
  std::vector<int32_t> crefs;    // 4 child refs per node (the compact form's ref records)
  float cstep = 1.0f;            // scene-wide decode step of the compact nodes
  float cbound = 0.0f;           // M: the compact codes are exact for ray origins with |o| <= M
  std::vector<float> tris;    // kTriRecordFloats per triangle, leaf order (wgt_geom.h)
  std::vector<float> tshade;  // 8 floats per original triangle
  uint32_t n_nodes = 0, n_leaves = 0, max_depth = 0, max_leaf = 0;  // BVH4 nodes / depth
  uint32_t n_nodes2 = 0, depth2 = 0;  // the SAH BVH2 the BVH4 was collapsed from
  uint32_t stack_need = 0;            // worst-case traversal stack entries (exact for this tree)
  bool narrow = false;                // collapsed under BvhOptions::narrow_limit
  double sah_cost = 0.0;
};

// Builds over n >= 1 triangles; on failure err says why.
bool BuildBvh(const wgt_triangle* tris, uint32_t n, const BvhOptions& opt, BvhOut& out, std::string& err);

// Refits a built tree to n moved triangles (triangle i keeps its index; n as built): the topology
// stays (refs, leaf order, n_nodes, stack_need, depths), and tris, tshade, every live slot's box
// and the compact form (cnodes, cstep, cbound, for ray origins within origin_bound) are recomputed
// as the build computes them, so a refit to the build's own triangles reproduces it bit for bit.
// sah_cost stays the build's value: it describes the tree as built, not the refit one.  On failure
// (a non-finite triangle box, as in the build) err says why and bvh is unchanged.
bool RefitBvh(BvhOut& bvh, const wgt_triangle* tris, uint32_t n, double origin_bound, std::string& err);

// The leaf target of a rebuild, WGT_REBUILD_LEAF (4): 1..kLeafMax.
uint32_t RebuildLeafFromEnv();

// The tree of a rebuild, the specification of wgt_rebuild_triangles: an LBVH over
// 63-bit Morton codes of the triangles' centres (wgt_morton.h), emitted directly as a BVH4 of at most
// kRebuildLevels levels with leaves of at most `leaf` triangles, nodes numbered breadth-first; the
// boxes, records and compact form are RefitBvh's for that topology.  No BVH2 exists: n_nodes2, depth2
// and sah_cost stay 0.  level_count (may be null) receives the nodes of each level, root first.  On
// failure (no triangles, more than rebuild_max_tris(leaf), a non-finite triangle box) err says why.
bool BuildMortonBvh(const wgt_triangle* tris, uint32_t n, uint32_t leaf, double origin_bound, BvhOut& out,
                    std::vector<uint32_t>* level_count, std::string& err);

// The tree as the kernels read it: internal refs are byte offsets (one add to the uniform
// base instead of an index multiply), leaf refs are unchanged.
struct BvhImage {
  std::vector<float> nodes;      // the 128-B nodes, internal refs x 128
  std::vector<uint32_t> crecs;   // 80-B compact records: a node's cnodes words, then its crefs, internal ones x 80
  std::vector<uint8_t> level;    // each node's level: root 0, saturating at 255
};
BvhImage DeviceImage(const BvhOut& bvh);
// The inverse for n_nodes nodes of a device image: the export layouts of wgt_bvh_build (nodes_out)
// and wgt_bvh_build_compact (cnodes_out, crefs_out), refs as indices; any output may be null.
void ExportImage(const float* dev_nodes, const uint32_t* dev_crecs, uint32_t n_nodes, float* nodes_out,
                 uint32_t* cnodes_out, int32_t* crefs_out);

}  // namespace wgt
