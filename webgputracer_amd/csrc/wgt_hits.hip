// wgt_hits.hip — full hit records: the surface at the closest hit of caller-supplied rays
// (wgt_trace_hits) and of each pixel's first camera ray (wgt_render_gbuffer, a first-hit
// G-buffer), in a translation unit of their own, away from the render kernels and their
// register budgets.
//
// A record is the reference's HitInfo after sample_hit (path_tracer.wgsl:27-36, 290-310):
// distance, primitive, emissive, front face, position, oriented normal and colour: the
// fields of Hit (wgt_hit.h) as closest_hit (wgt_trav.h) leaves them, with the IEEE forms
// (EXACT) for any caller ray.  wgt_trace_rays is k_trace_hits with prim and dist alone, the
// instantiation without the surface fields (SURFACE = false).
#include "wgt_hit.h"
#include "wgt_pixel.h"
#include "wgt_trav.h"

namespace wgt {

namespace {

// Record i of n, planar (wgt_hit_buffers): plain vector stores after the hit is final, each
// behind a wave-uniform null test (the pointers are kernel arguments).
__device__ __forceinline__ void store_f3(float* __restrict__ p, size_t n, size_t i, f3 v) {
  p[i] = v.x;
  p[n + i] = v.y;
  p[2 * n + i] = v.z;
}
// SURFACE = false: prim and dist alone (launch_trace_hits), so that nothing else of the hit is computed.
template <bool SURFACE = true>
__device__ __forceinline__ void store_hit(const wgt_hit_buffers& out, size_t n, size_t i, const Hit& h) {
  if (out.prim) out.prim[i] = h.prim;
  if (out.dist) out.dist[i] = h.dist;
  if (!SURFACE) return;
  if (out.pos) store_f3(out.pos, n, i, h.pos);
  if (out.norm) store_f3(out.norm, n, i, h.norm);
  if (out.col) store_f3(out.col, n, i, h.col);
  if (out.flags) out.flags[i] = (uint8_t)((h.emissive ? WGT_HIT_EMISSIVE : 0u) | (h.front_face ? WGT_HIT_FRONT_FACE : 0u));
}

// Launch lane i runs ray i (the flat form, as k_occluded: DESIGN.md §4.4a).
template <bool TRIS, bool SURFACE>
__global__ void __launch_bounds__(kBlock)
k_trace_hits(DevScene sc, const float* __restrict__ rays, uint32_t n, wgt_hit_buffers out) {
  extern __shared__ int s_stack[];  // sc.stack entries per lane (stack_lds_bytes)
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const f3 o = f3{rays[i], rays[(size_t)n + i], rays[2 * (size_t)n + i]};
  const f3 d = f3{rays[3 * (size_t)n + i], rays[4 * (size_t)n + i], rays[5 * (size_t)n + i]};
  Hit h;
  closest_hit<TRIS, true>(sc, o, d, s_stack + threadIdx.x, h);
  store_hit<SURFACE>(out, n, i, h);
}

// One lane per pixel of the tile list, as k_render: the pixel and its seed from slot_setup,
// sample 0's ray from camera_ray (px.sij = 0: the first two rand() of the pixel's seed), so
// the record is that of the ray whose primitive the render reports as the pixel's hit ID.
// A pixel without samples (sqrt_spp = 0) gets hit_init's record (write_pixel's kNoHit) and
// a zero ray; a pixel of a tile outside the frame is not written, as the render leaves it.
// n = n_tiles * tw * th records, pixel offset po (slot_setup).
// SM: the G-buffer of a sampled frame (SampleArgs, the last kernel argument): sample 0's jitter depends on the pixel's
// side, which slot_setup takes from the map as the sampled render does; a pixel of side 0 is a
// pixel without samples.
template <bool TRIS, bool SM = false>
__global__ void __launch_bounds__(kBlock)
k_gbuffer(DevScene sc, DevFrame fr, const wgt_tile* __restrict__ tiles, wgt_hit_buffers out,
          float* __restrict__ rays, SampleArgs sm) {
  extern __shared__ int s_stack[];  // sc.stack entries per lane (stack_lds_bytes)
  uint32_t po;
  Pixel px;
  if (!slot_setup<SM>(fr, tiles, blockIdx.x, threadIdx.x, po, px, sm)) return;  // one pixel per lane
  const size_t n = (size_t)fr.n_tiles * fr.tw * fr.th;
  f3 ro{0.0f, 0.0f, 0.0f}, rd{0.0f, 0.0f, 0.0f};
  Hit h;
  if (px_done<SM>(fr, px)) {
    hit_init(h);
  } else {
    camera_ray<SM>(fr, px, ro, rd, sm);
    closest_hit<TRIS, true>(sc, ro, rd, s_stack + threadIdx.x, h);
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
  // the closest-hit query (wgt_trace_rays: prim and dist alone) loads no normal, colour or shading record
  const bool surface = out.pos || out.norm || out.col || out.flags;
  (sc.n_tris > 0 ? (surface ? k_trace_hits<true, true> : k_trace_hits<true, false>)
                 : (surface ? k_trace_hits<false, true> : k_trace_hits<false, false>))
      <<<grid, block, stack_lds_bytes(sc.stack), stream>>>(sc, d_rays, n, out);
  return hipGetLastError();
}

hipError_t launch_gbuffer(const DevScene& sc, const DevFrame& fr, const SampleArgs& sm, const wgt_tile* d_tiles,
                          const wgt_hit_buffers& out, float* d_rays, hipStream_t stream) {
  uint32_t blocks;
  DevFrame fm;  // + slot_setup's division multipliers
  const hipError_t eg = tile_grid(fr, blocks, fm);
  if (eg != hipSuccess || blocks == 0) return eg;
  const dim3 grid(blocks), block(kBlock);
  (sm.map ? (sc.n_tris > 0 ? k_gbuffer<true, true> : k_gbuffer<false, true>)
           : (sc.n_tris > 0 ? k_gbuffer<true> : k_gbuffer<false>))
      <<<grid, block, stack_lds_bytes(sc.stack), stream>>>(sc, fm, d_tiles, out, d_rays, sm);
  return hipGetLastError();
}

}  // namespace wgt
