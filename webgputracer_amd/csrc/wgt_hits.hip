// wgt_hits.hip — full hit records: the surface at the closest hit of caller-supplied rays
// (wgt_trace_hits) and of each pixel's first camera ray (wgt_render_gbuffer, a first-hit
// G-buffer), in a translation unit of their own, away from the render kernels and their
// register budgets.
//
// A record is the reference's HitInfo after sample_hit (path_tracer.wgsl:27-36, 290-310):
// distance, primitive, emissive, front face, position, oriented normal and colour — the
// fields of Hit (wgt_device.h), which k_trace computes too and drops but for two.  Both
// kernels here build it from the pieces sample_hit is built from, with the same operands,
// so prim and dist are k_trace's bit for bit; only the order of work differs (closest_hit).
#include "wgt_device.h"

namespace wgt {

namespace {

// sample_hit<TRIS, false, true> with the quad hit rebuilt after the traversal instead of
// before it: quad_scan_fast leaves (qprim, qt), all the traversal needs of the quad hit
// (trav_init reads whether there is one and its t), so the thirteen registers of Hit are
// not live across the loop when every field is stored afterwards.  This is the order of
// k_render_ps's finalise.  IEEE forms (EXACT) throughout, as k_trace: any caller ray.
template <bool TRIS>
__device__ __forceinline__ void closest_hit(const DevScene& sc, f3 o, f3 d, int* __restrict__ lds, Hit& h) {
  if (has_nan(o) || has_nan(d)) {
    nan_hit(sc, o, d, h);
    return;
  }
  float qt;
  uint32_t qprim;
  quad_scan_fast<true>(sc, o, d, qprim, qt);
  Trav t;
  trav_init<0, true>(sc, o, d, qprim != kNoHit, qt, t);
  if (TRIS) {
    TravStats st{};
    while (!trav_step<false>(sc, o, d, t, lds, st)) {
    }
  }
  quad_rebuild(sc, o, d, qprim, qt, h);
  finish_hit(sc, o, d, t, h);
}

// Record i of n, planar (wgt_hit_buffers): plain vector stores after the hit is final, each
// behind a wave-uniform null test (the pointers are kernel arguments).
__device__ __forceinline__ void store_f3(float* __restrict__ p, size_t n, size_t i, f3 v) {
  p[i] = v.x;
  p[n + i] = v.y;
  p[2 * n + i] = v.z;
}
__device__ __forceinline__ void store_hit(const wgt_hit_buffers& out, size_t n, size_t i, const Hit& h) {
  if (out.prim) out.prim[i] = h.prim;
  if (out.dist) out.dist[i] = h.dist;
  if (out.pos) store_f3(out.pos, n, i, h.pos);
  if (out.norm) store_f3(out.norm, n, i, h.norm);
  if (out.col) store_f3(out.col, n, i, h.col);
  if (out.flags) out.flags[i] = (uint8_t)((h.emissive ? WGT_HIT_EMISSIVE : 0u) | (h.front_face ? WGT_HIT_FRONT_FACE : 0u));
}

// Launch lane i runs ray i (the flat form, as k_trace and k_occluded: DESIGN.md §4.4a).
template <bool TRIS>
__global__ void __launch_bounds__(kBlock)
k_trace_hits(DevScene sc, const float* __restrict__ rays, uint32_t n, wgt_hit_buffers out) {
  extern __shared__ int s_stack[];  // sc.stack entries per lane (stack_lds_bytes)
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const f3 o = f3{rays[i], rays[(size_t)n + i], rays[2 * (size_t)n + i]};
  const f3 d = f3{rays[3 * (size_t)n + i], rays[4 * (size_t)n + i], rays[5 * (size_t)n + i]};
  Hit h;
  closest_hit<TRIS>(sc, o, d, s_stack + threadIdx.x, h);
  store_hit(out, n, i, h);
}

// One lane per pixel of the tile list, as k_render: the pixel and its seed from slot_setup,
// sample 0's ray from camera_ray (px.sij = 0: the first two rand() of the pixel's seed), so
// the record is that of the ray whose primitive the render reports as the pixel's hit ID.
// A pixel without samples (sqrt_spp = 0) gets hit_init's record (write_pixel's kNoHit) and
// a zero ray; a pixel of a tile outside the frame is not written, as the render leaves it.
// n = n_tiles * tw * th records, pixel offset po (slot_setup).
template <bool TRIS>
__global__ void __launch_bounds__(kBlock)
k_gbuffer(DevScene sc, DevFrame fr, const wgt_tile* __restrict__ tiles, wgt_hit_buffers out,
          float* __restrict__ rays) {
  extern __shared__ int s_stack[];  // sc.stack entries per lane (stack_lds_bytes)
  uint32_t po;
  Pixel px;
  if (!pixel_setup(fr, tiles, po, px)) return;
  const size_t n = (size_t)fr.n_tiles * fr.tw * fr.th;
  f3 ro{0.0f, 0.0f, 0.0f}, rd{0.0f, 0.0f, 0.0f};
  Hit h;
  if (px_done(fr, px)) {
    hit_init(h);
  } else {
    camera_ray(fr, px, ro, rd);
    closest_hit<TRIS>(sc, ro, rd, s_stack + threadIdx.x, h);
  }
  store_hit(out, n, po, h);
  if (rays) {
    store_f3(rays, n, po, ro);
    store_f3(rays + 3 * n, n, po, rd);
  }
}

}  // namespace

hipError_t launch_trace_hits(const DevScene& sc, const float* d_rays, uint32_t n, const wgt_hit_buffers& out,
                             hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
  if (sc.n_tris > 0) k_trace_hits<true><<<grid, block, stack_lds_bytes(sc.stack), stream>>>(sc, d_rays, n, out);
  else k_trace_hits<false><<<grid, block, stack_lds_bytes(sc.stack), stream>>>(sc, d_rays, n, out);
  return hipGetLastError();
}

hipError_t launch_gbuffer(const DevScene& sc, const DevFrame& fr, const wgt_tile* d_tiles,
                          const wgt_hit_buffers& out, float* d_rays, hipStream_t stream) {
  const uint32_t bx = (fr.tw + 7u) / 8u, by = (fr.th + 7u) / 8u;
  const uint64_t blocks = (uint64_t)bx * by * fr.n_tiles;
  if (blocks == 0) return hipSuccess;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  DevFrame fm = fr;  // + slot_setup's division multipliers, as launch_render
  fm.div_bx = 0xffffffffu / bx;
  fm.div_bpt = 0xffffffffu / (bx * by);
  const dim3 grid((uint32_t)blocks), block(kBlock);
  if (sc.n_tris > 0) k_gbuffer<true><<<grid, block, stack_lds_bytes(sc.stack), stream>>>(sc, fm, d_tiles, out, d_rays);
  else k_gbuffer<false><<<grid, block, stack_lds_bytes(sc.stack), stream>>>(sc, fm, d_tiles, out, d_rays);
  return hipGetLastError();
}

}  // namespace wgt
