// wgt_motion.h — what the motion passes' thin calls (wgt_runtime.cpp) and their kernels
// (wgt_motion.hip) share: the snapshot's layout and the two launchers.  A header of
// its own, as wgt_temporal.h: the render, query, refit and denoise kernels' translation units do not
// see it.
#pragma once

#include "wgt_internal.h"

namespace wgt {

// The snapshot of the resident triangles, per ORIGINAL triangle index t: 12 floats (v0, e1, e2, the
// face normal) as three float4s at snap[3 t], and the leaf slot of t's record at slot_of[t].
constexpr uint32_t kMotionSnapFloat4s = 3;
constexpr size_t kMotionSnapBytes = kMotionSnapFloat4s * 16 + 4;  // per triangle, both arrays
constexpr uint32_t kMotionMaxRecords = 1u << 25;                  // of one reproject

// Launchers implemented in wgt_motion.hip, each one pass on `stream`.
// snap[3 orig .. 3 orig + 2] and slot_of[orig] of every leaf slot's record (an original index that
// is not below n_tris is skipped, never stored through).
hipError_t launch_motion_snapshot(const DevScene& sc, float4* snap, uint32_t* slot_of, hipStream_t stream);
// pos_prev and norm_prev of n planar records (guides: prim, pos, norm, flags; device pointers).
hipError_t launch_motion_reproject(const DevScene& sc, const float4* snap, const uint32_t* slot_of, uint32_t n,
                                   const wgt_hit_buffers& guides, const wgt_motion_buffers& out, hipStream_t stream);

}  // namespace wgt
