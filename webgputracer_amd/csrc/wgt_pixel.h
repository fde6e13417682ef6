// wgt_pixel.h — a pixel's side of the render kernels: shading (raytrace() after the hit), the
// per-pixel state and its sample order, the pixel of a launch slot on the 8x8-block grid of a
// tile list (slot_setup, and the host's tile_grid that sizes it), the camera ray, the output
// stores and the counters.  k_gbuffer takes its pixels and camera rays from here too.
#pragma once

#include "wgt_trav.h"

namespace wgt {

struct Light {
  f3 pos, right, up;
};

// raytrace() after sample_hit (path_tracer.wgsl:267-287).  Returns path.end.
__device__ __forceinline__ bool shade(const DevScene& sc, const Light& L, const Hit& h, int depth,
                                      uint32_t& seed, f3& ro, f3& rd, f3& pc) {
  if (h.emissive) {
    if (depth != 0) {
      const float ff = h.front_face ? 1.0f : 0.0f;
      pc = (ff * h.col) * pc;
    } else {
      pc = h.col;
    }
    return true;
  }
  // sample_direction (path_tracer.wgsl:146-154).  The shading divisions stay IEEE: short forms
  // behind per-lane range tests measured slower
  const f3 w = normalize(h.norm);  // onb.w of build_onb_from_w(hit.norm)
  f3 sdir;
  // both branches draw two more rand() (r1 then r2) right away: drawn once here, the
  // same values in the same order
  const bool cosine = rand_next(seed) > 0.5f;
  const float r1 = rand_next(seed);
  const float r2 = rand_next(seed);
  if (cosine) {
    // sample_from_cosine: build_onb_from_w (:133-140) + rand_cos_dir (:123-131)
    const f3 a = (sign_w(w.x) * w.x) > 0.9f ? f3{0.0f, 1.0f, 0.0f} : f3{1.0f, 0.0f, 0.0f};
    // |w| = 1 +- 2^-22 and a is the axis w is furthest from: |w x a|^2 >= 0.19
    const f3 v = normalize_unit(cross(w, a));
    const f3 u = cross(w, v);
    const float z = sqrt_fast(1.0f - r2);
    const float phi = 2.0f * kPI * r1;
    float sphi, cphi;
    sincos_w(phi, sphi, cphi);
    const float sr2 = sqrt_fast(r2);
    const float lx2 = cphi * sr2;
    const float ly2 = sphi * sr2;
    sdir = (lx2 * u + ly2 * v) + z * w;
  } else {
    // sample_from_light (:163-168), not normalised
    sdir = ((L.pos + r1 * L.right) + r2 * L.up) - h.pos;
  }
  // mixture_pdf (:191-193) = 0.5*cosine_pdf + 0.5*light_area_pdf
  const float len = length(sdir);
  const f3 nd = sdir / len;  // normalize(dir): shared by cosine_pdf, the light cosine and :282
  const float cs = dot(nd, w);
  const float cpdf = cs <= 0.0f ? 0.0f : cs * k_1_PI;
  const float dist2 = len * len;
  const float light_cosine = fabs_w(nd.y) + kRayMin;
  const float lpdf = dist2 / (light_cosine * sc.light_area);
  const float pdf_val = 0.5f * cpdf + 0.5f * lpdf;
  // scattering_pdf (:217-220) normalises the already normalised direction again
  const f3 nd2 = normalize_unit(nd);  // nd = sdir / exact length: unit, NaN or 0
  const float cs2 = dot(h.norm, nd2);
  const float spdf = cs2 < 0.0f ? 0.0f : cs2 * k_1_PI;
  pc = (spdf * (pc * h.col)) / pdf_val;
  ro = h.pos;
  rd = nd;
  return false;
}

__device__ __forceinline__ uint8_t unorm8(float x) {
  float c = max0(x);
  c = c < 1.0f ? c : 1.0f;
  return (uint8_t)__builtin_floorf(c * 255.0f + 0.5f);
}

// Per-pixel state shared by both kernels.
struct Pixel {
  uint32_t xy;  // x | y << 16 (frames are at most 65535 x 65535, check_render_args): one register
  uint32_t seed;
  uint32_t sij;  // the sample's s_i | s_j << 16 (sqrt_spp < 2^16); index = s_i + s_j * sqrt_spp
  f3 col;
};
// SM (the sampled kernels, SampleArgs): the pixel's side k (its sqrt_spp, <= 255) comes from
// the sample map and lives in the same register: sij = s_i | s_j << 8 | k << 16 (s_i < k, s_j <= k
// fit 8 bits each); the cost pre-pass renders min(k, pq_lpt) there and keeps the map's k in bits 24-31.
// all sqrt_spp^2 samples done (sj reaches sqrt_spp; at once when spp = 0)
template <bool SM = false>
__device__ __forceinline__ uint32_t px_si(const Pixel& px) { return SM ? px.sij & 0xffu : px.sij & 0xffffu; }
template <bool SM = false>
__device__ __forceinline__ uint32_t px_sj(const Pixel& px) { return SM ? (px.sij >> 8) & 0xffu : px.sij >> 16; }
// the pixel's sample-grid side
template <bool SM = false>
__device__ __forceinline__ uint32_t px_side(const DevFrame& fr, const Pixel& px) {
  return SM ? (px.sij >> 16) & 0xffu : fr.sqrt_spp;
}
template <bool SM = false>
__device__ __forceinline__ bool px_done(const DevFrame& fr, const Pixel& px) { return px_sj<SM>(px) >= px_side<SM>(fr, px); }
// next (s_i, s_j) in the reference's loop order (path_tracer.wgsl:381-382)
template <bool SM = false>
__device__ __forceinline__ void px_next(const DevFrame& fr, Pixel& px) {
  if (SM) px.sij = px_si<SM>(px) + 1u == px_side<SM>(fr, px) ? (px.sij & 0xffffff00u) + 0x100u : px.sij + 1u;
  else px.sij = px_si(px) + 1u == fr.sqrt_spp ? (px.sij & 0xffff0000u) + 0x10000u : px.sij + 1u;
}
// sample 0 (the one whose first hit is the pixel's hit ID)
template <bool SM = false>
__device__ __forceinline__ bool px_first(const Pixel& px) { return SM ? (px.sij & 0xffffu) == 0u : px.sij == 0u; }

struct Counters {
  uint32_t q, tr, nan, lw, ll;
  uint32_t qref;  // rays whose quad scan took the reference path (quad_scan_fast's almost-ties)
  uint32_t px;  // pixels finished by this lane
};

// x / d for d >= 1 with m = (2^32 - 1) / d (host): mulhi(x, m) is x / d or up to two less
// (x m / 2^32 > x / d - x / 2^32 - x / (d 2^32) - 1 > x / d - 3 for x < 2^32), fixed by two steps.
__device__ __forceinline__ uint32_t udiv_by(uint32_t x, uint32_t d, uint32_t m) {
  uint32_t q = __umulhi(x, m);
  uint32_t r = x - q * d;
  if (r >= d) { ++q; r -= d; }
  if (r >= d) ++q;
  return q;
}

// The 8x8-block grid of a launch over fr's tile list (host): the block count, and in fm the
// frame with the multipliers (2^32 - 1) / d that slot_setup divides by (DevFrame::div_bx,
// div_bpt; left as they are for an empty grid).  Refuses more blocks than a grid dimension holds.
inline hipError_t tile_grid(const DevFrame& fr, uint32_t& blocks, DevFrame& fm) {
  const uint32_t bx = (fr.tw + 7u) / 8u, by = (fr.th + 7u) / 8u;
  const uint64_t nb = (uint64_t)bx * by * fr.n_tiles;
  if (nb > 0x7fffffffull) return hipErrorInvalidValue;
  blocks = (uint32_t)nb;
  fm = fr;
  if (nb != 0) {
    fm.div_bx = 0xffffffffu / bx;
    fm.div_bpt = 0xffffffffu / (bx * by);
  }
  return hipSuccess;
}

// Pixel of pixel slot (block, lane) = (slot >> 6, slot & 63): block b covers an
// 8x8 sub-block of tile b / (sub-blocks per tile).  false if the slot is outside
// its tile or the frame.  po = the pixel's offset in the tile-major output
// ((tile * th + ly) * tw + lx; the host keeps tiles * tw * th < 2^31).
// SM: the pixel's side from the sample map (global pixel coordinates, row-major); side_cap: the
// side the launch renders at most (255; the cost pre-pass: pq_lpt).
template <bool SM = false>
__device__ __forceinline__ bool slot_setup(const DevFrame& fr, const wgt_tile* __restrict__ tiles,
                                           uint32_t block, uint32_t lane, uint32_t& po, Pixel& px,
                                           const SampleArgs& sm = SampleArgs{}, uint32_t side_cap = 255u) {
  const uint32_t bx = (fr.tw + 7u) >> 3, by = (fr.th + 7u) >> 3;
  const uint32_t bpt = bx * by;
  // divisions by the host's multipliers (DevFrame::div_bx, div_bpt): no per-lane reciprocal kept
  // live through the kernel, where the compiler's division by a runtime value would hoist one
  const uint32_t tile = udiv_by(block, bpt, fr.div_bpt);
  const uint32_t rem = block - tile * bpt;
  const uint32_t ry = udiv_by(rem, bx, fr.div_bx);
  const uint32_t lx = (rem - ry * bx) * 8u + (lane & 7u);
  const uint32_t ly = ry * 8u + (lane >> 3);
  if (tile >= fr.n_tiles || lx >= fr.tw || ly >= fr.th) return false;
  const wgt_tile td = tiles[tile];
  const uint32_t x = td.x0 + lx, y = td.y0 + ly;
  if (x >= fr.W || y >= fr.H) return false;  // path_tracer.wgsl:377
  px.xy = x | y << 16;
  px.seed = x + y * fr.W + td.seed * fr.W * fr.H;  // path_tracer.wgsl:378
  if (SM) {
    const uint32_t k = sm.map[(size_t)y * fr.W + x];
    px.sij = (k < side_cap ? k : side_cap) << 16 | k << 24;
  } else {
    px.sij = 0u;
  }
  px.col = f3{0.0f, 0.0f, 0.0f};
  po = (tile * fr.th + ly) * fr.tw + lx;
  return true;
}

// setup_camera_ray + pixel_sample_square (path_tracer.wgsl:232-262) for the sample (s_i, s_j) of px.sij
template <bool SM = false>
__device__ __forceinline__ void camera_ray(const DevFrame& fr, Pixel& px, f3& ro, f3& rd,
                                           const SampleArgs& sm = SampleArgs{}) {
  const f3 origin = f3{fr.ox, fr.oy, fr.oz};
  const f3 du = f3{fr.dux, fr.duy, fr.duz};
  const f3 dv = f3{fr.dvx, fr.dvy, fr.dvz};
  const f3 pixel_center = (f3{fr.pox, fr.poy, fr.poz} + (float)(px.xy & 0xffffu) * du) + (float)(px.xy >> 16) * dv;
  // SM: the side's constants from the host's table (SampleArgs::tab), read per sample
  const float rss = SM ? sm.tab[px_side<SM>(fr, px)].x : fr.recip_sqrt_spp;
  const float sx = -0.5f + rss * ((float)px_si<SM>(px) + rand_next(px.seed));
  const float sy = -0.5f + rss * ((float)px_sj<SM>(px) + rand_next(px.seed));
  const f3 pixel_sample = pixel_center + (sx * du + sy * dv);
  ro = origin;
  rd = pixel_sample - origin;
}

// col += max(path.col, 0) / f32(spp) (path_tracer.wgsl:393) and advance to the next sample
template <bool SM = false>
__device__ __forceinline__ void end_sample(const DevFrame& fr, Pixel& px, f3 pc, const SampleArgs& sm = SampleArgs{}) {
  // x / 2^k == x * 2^-k exactly (one rounding of the same real value), so a
  // power-of-two spp multiplies
  const f3 m{max0(pc.x), max0(pc.y), max0(pc.z)};
  if (SM) {
    const float4 k = sm.tab[px_side<SM>(fr, px)];  // (recip_sqrt_spp, fspp, inv_fspp, 0) of this pixel's side
    px.col = px.col + (k.z != 0.0f ? k.z * m : m / k.y);
  } else {
    px.col = px.col + (fr.inv_fspp != 0.0f ? fr.inv_fspp * m : m / fr.fspp);
  }
  px_next<SM>(fr, px);
}

// The pixel's hit ID (path_tracer.wgsl:384-386): the primitive of sample 0's camera ray.
template <bool SM = false>
__device__ __forceinline__ void first_hit(const Pixel& px, int depth, uint32_t prim, uint32_t po,
                                          uint32_t* __restrict__ outhit) {
  if (outhit && depth == 0 && px_first<SM>(px)) outhit[po] = prim;
}

// NaN-absorbed for the rest of the path: 3 rand() per remaining bounce, colour NaN.
template <bool STATS, bool SM = false>
__device__ __forceinline__ void skip_nan_path(const DevScene& sc, const DevFrame& fr, Pixel& px,
                                              int depth, Counters& c) {
  px.seed = lcg_jump(px.seed, 3u * (uint32_t)(kRayDepth - depth));
  if (STATS) {
    c.q += (uint32_t)(kRayDepth - depth);
    c.nan += (uint32_t)(kRayDepth - depth);
  }
  // col += max(NaN, 0) / spp == col + 0
  px_next<SM>(fr, px);
}

template <bool SM = false>
__device__ __forceinline__ void write_pixel(const DevFrame& fr, uint32_t po, const Pixel& px, uchar4* out8,
                                            float4* out32, uint32_t* outhit) {
  if (out32) out32[po] = make_float4(px.col.x, px.col.y, px.col.z, 1.0f);
  if (out8) out8[po] = make_uchar4(unorm8(px.col.x), unorm8(px.col.y), unorm8(px.col.z), 255);
  // the hit ID is written when sample 0's first hit is known (first_hit); a
  // pixel without samples has none
  if (outhit && px_side<SM>(fr, px) == 0u) outhit[po] = kNoHit;
}

template <bool SM = false>
__device__ __forceinline__ void flush_counters(unsigned long long* __restrict__ counters,
                                               const Counters& c, const TravStats& st,
                                               uint32_t nsamp, unsigned long long smp = 0) {
  // c.px pixels, nsamp samples each (SM: smp samples, the sum of the finished pixels' k^2)
  atomicAdd(&counters[CNT_QUERIES], (unsigned long long)c.q);
  atomicAdd(&counters[CNT_TRACED], (unsigned long long)c.tr);
  atomicAdd(&counters[CNT_SAMPLES], SM ? smp : (unsigned long long)nsamp * c.px);
  atomicAdd(&counters[CNT_NAN], (unsigned long long)c.nan);
  atomicAdd(&counters[CNT_NODES], (unsigned long long)st.nodes);
  atomicAdd(&counters[CNT_TRIS], (unsigned long long)st.tris);
  atomicAdd(&counters[CNT_PIXELS], (unsigned long long)c.px);
  if (c.qref) atomicAdd(&counters[CNT_QUAD_REF], (unsigned long long)c.qref);
  atomicAdd(&counters[CNT_LOOP_WAVE], (unsigned long long)c.lw);
  atomicAdd(&counters[CNT_LOOP_LANE], (unsigned long long)c.ll);
  atomicAdd(&counters[CNT_TRAV_WAVE], (unsigned long long)st.wave_steps);
  atomicAdd(&counters[CNT_TRAV_LANE], (unsigned long long)st.lane_steps);
  if (st.spills) atomicAdd(&counters[CNT_STACK_SPILLS], (unsigned long long)st.spills);
  if (st.refills) atomicAdd(&counters[CNT_STACK_REFILLS], (unsigned long long)st.refills);
  if (st.overflows) atomicAdd(&counters[CNT_STACK_OVERFLOWS], (unsigned long long)st.overflows);
}

}  // namespace wgt
