// wgt_denoise_variance.hip — the variance-guided denoiser (wgt_denoise_variance,
// wgt_denoise_variance_async): wgt_denoise's edge-avoiding a-trous filter with a luminance weight
// scaled by each pixel's own variance, over the state wgt_temporal_accumulate wrote, in a translation
// unit of its own.
//
// The arithmetic is the specification's, operation by operation (tests/denoise_variance_restatement.py
// is the same in numpy, and the outputs are equal bit for bit): binary32, no fused multiply-add
// (-ffp-contract=off), the compiler's correctly rounded division, sqrt_rn, denormals kept.
//
//   k_dv_pack    : the mask, the albedo divisor, the first iterate (rgb / albedo, variance) and one
//                  packed guide record per pixel (DenoiseVariancePlan).  A pixel with a history of
//                  min_history frames or more takes its variance from its own moments
//   k_dv_spatial : the other valid pixels alone (the record's tag 2; every other lane returns at once):
//                  a 7 x 7 estimate of the variance from the neighbours' moments
//   k_dv_atrous_lds, k_dv_atrous : one iterate to the next, 25 taps at a step of 2^i pixels, colour
//                  and variance in one float4, so that a tap stays three 16-byte loads; the last pass
//                  remodulates and writes the outputs (the alpha comes from the record).  Before its
//                  taps a pixel reads the variance of its 3 x 3 unit-spaced neighbours (nine dword
//                  loads through the caches: they lie off the lattice tile for any step above 1) for
//                  its luminance tolerance.  The two forms and their switch are wgt_denoise's
//                  (DenoiseVariancePlan::tiled_max_step)
// A workgroup is 64 x 4 pixels.  Every kernel checks its pixel against W x H; taps outside the image
// are clamped into it (the gathers) or staged as not valid (the tile).  No atomics, no scratch; every
// index fits 32 bits (W * H <= 2^25, and the largest is 4 W H).
#include "wgt_denoise_variance.h"

#include "wgt_pixel.h"

namespace wgt {

namespace {

constexpr int kDvX = 64, kDvY = 4;
constexpr float kOkLimit = 0x1p100f;   // ok(v): every |component| <= 2^100 (NaN and inf fail)
constexpr float kAlbedoMin = 0x1p-8f;  // the demodulation divisor's floor
constexpr float kLumEps = 1e-6f;       // added to the luminance tolerance: a variance of 0 divides by it
constexpr float kTagValid = 1.0f, kTagShort = 2.0f;  // rec[2 i].w of a valid pixel (0: not valid)
constexpr float kNotValid = -1.0f;     // the iterate's .w of a pixel that is not valid

__device__ __forceinline__ bool ok1(float v) { return __builtin_fabsf(v) <= kOkLimit; }
__device__ __forceinline__ bool ok3(f3 v) { return ok1(v.x) && ok1(v.y) && ok1(v.z); }
__device__ __forceinline__ f3 load_planar(const float* __restrict__ p, uint32_t n, uint32_t i) {
  return f3{p[i], p[(size_t)n + i], p[2 * (size_t)n + i]};
}
__device__ __forceinline__ float albedo1(float c) { return c > kAlbedoMin ? c : kAlbedoMin; }
// The divisor a of a pixel: its albedo floored at 2^-8, or ones without demodulation.
__device__ __forceinline__ f3 albedo(const float* __restrict__ col, uint32_t n, uint32_t i, uint32_t demodulate) {
  if (!demodulate) return f3{1.0f, 1.0f, 1.0f};
  const f3 c = load_planar(col, n, i);
  return f3{albedo1(c.x), albedo1(c.y), albedo1(c.z)};
}
// §4.8's luminance
__device__ __forceinline__ float luminance(f3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
// (1 - x / 16)^16: e^-x with compact support, without a division or a library call.  NaN gives 0.
__device__ __forceinline__ float falloff(float x) {
  float t = max0(1.0f - x * 0.0625f);
  t = t * t;
  t = t * t;
  t = t * t;
  t = t * t;
  return t;
}
__device__ __forceinline__ f3 xyz(float4 v) { return f3{v.x, v.y, v.z}; }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : v >= hi ? hi - 1 : v; }

__device__ __forceinline__ bool pixel_of_block(uint32_t W, uint32_t H, uint32_t& x, uint32_t& y) {
  x = blockIdx.x * kDvX + threadIdx.x;
  y = blockIdx.y * kDvY + threadIdx.y;
  return x < W && y < H;
}

// The normal weight and the plane weight of tap q for pixel p: (h wn) wz without its h.
__device__ __forceinline__ float normal_weight(f3 np, f3 nq, uint32_t normal_power) {
  float wn = max0(dot(np, nq));
  for (uint32_t k = 0; k < normal_power; ++k) wn = wn * wn;
  return wn;
}
__device__ __forceinline__ float plane_weight(f3 np, f3 pp, f3 pq, float kz) {
  const float d = dot(np, pq - pp);
  return falloff((d * d) * kz);
}

__global__ void __launch_bounds__(kDvX * kDvY)
k_dv_pack(const float4* __restrict__ in, const float* __restrict__ len, const float* __restrict__ mom, wgt_hit_buffers g,
          uint32_t W, uint32_t H, uint32_t demodulate, float min_history, float4* __restrict__ rec,
          float4* __restrict__ it0) {
  uint32_t x, y;
  if (!pixel_of_block(W, H, x, y)) return;
  const uint32_t n = W * H, i = y * W + x;
  const float4 c = in[i];
  const float l = len[i], m1 = mom[i], m2 = mom[(size_t)n + i];
  const f3 pos = load_planar(g.pos, n, i), norm = load_planar(g.norm, n, i), col = load_planar(g.col, n, i);
  const bool valid = g.prim[i] != kNoHit && !(g.flags[i] & WGT_HIT_EMISSIVE) && ok3(pos) && ok3(norm) && ok3(col) &&
                     ok3(xyz(c)) && l >= 1.0f && ok1(m1) && ok1(m2);
  const bool longh = l >= min_history;
  const f3 a = albedo(g.col, n, i, demodulate);
  const float s = luminance(a);
  // the per-frame variance of raw luminance, brought into the filtered space; a short history's is
  // k_dv_spatial's to write
  const float v = longh ? max0(m2 - m1 * m1) / (s * s) : 0.0f;
  rec[2 * i] = make_float4(norm.x, norm.y, norm.z, valid ? (longh ? kTagValid : kTagShort) : 0.0f);
  rec[2 * i + 1] = make_float4(pos.x, pos.y, pos.z, c.w);  // the alpha rides along to the last pass
  // a pixel that is not valid carries its colour through the passes as it came
  it0[i] = valid ? make_float4(c.x / a.x, c.y / a.y, c.z / a.z, v) : make_float4(c.x, c.y, c.z, kNotValid);
}

// The spatial estimate of a short history's variance: the moments of the 7 x 7 unit-spaced window
// over valid pixels under the normal weight and pass 0's plane weight (no spline; the centre has
// weight 1), dy outer, dx inner.  Writes it0[i].w alone, which no other lane reads here.
__global__ void __launch_bounds__(kDvX * kDvY)
k_dv_spatial(const float4* __restrict__ rec, const float* __restrict__ len, const float* __restrict__ mom,
             const float* __restrict__ col, uint32_t W_, uint32_t H_, uint32_t demodulate, uint32_t normal_power, float kz,
             float min_history, float4* __restrict__ it0) {
  uint32_t x, y;
  if (!pixel_of_block(W_, H_, x, y)) return;
  const uint32_t n = W_ * H_, i = y * W_ + x;
  // a long history (and a pixel without one) leaves on its 4-byte length alone; the tag decides the rest
  const float l = len[i];
  if (!(l >= 1.0f) || l >= min_history) return;
  const float4 np4 = rec[2 * i];
  if (np4.w != kTagShort) return;
  const int W = (int)W_, H = (int)H_;
  const f3 np = xyz(np4), pp = xyz(rec[2 * i + 1]);
  float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
#pragma unroll 1
  for (int dy = -3; dy <= 3; ++dy) {
    const int qy = (int)y + dy;
    const bool in_y = qy >= 0 && qy < H;
    const uint32_t row = (uint32_t)clampi(qy, H) * W_;
    // a row's seven taps at once: a wave with one short pixel pays a load round trip per row, not per tap
#pragma unroll
    for (int dx = -3; dx <= 3; ++dx) {
      const int qx = (int)x + dx;
      const uint32_t q = row + (uint32_t)clampi(qx, W);
      const float4 nq4 = rec[2 * q];
      const bool centre = dx == 0 && dy == 0;
      const bool use = centre || (in_y && qx >= 0 && qx < W && nq4.w != 0.0f);
      const float wq = normal_weight(np, xyz(nq4), normal_power) * plane_weight(np, pp, xyz(rec[2 * q + 1]), kz);
      const float w = centre ? 1.0f : use ? wq : 0.0f;
      const float m1 = use ? mom[q] : 0.0f, m2 = use ? mom[(size_t)n + q] : 0.0f;
      s1 = s1 + w * m1;
      s2 = s2 + w * m2;
      sw = sw + w;
    }
  }
  const float M1 = s1 / sw, M2 = s2 / sw;
  const float vraw = max0(M2 - M1 * M1) * (min_history / l);
  const float s = luminance(albedo(col, n, i, demodulate));
  ((float*)it0)[4 * i + 3] = vraw / (s * s);
}

// The 5-tap B3 spline kernel (1/16, 1/4, 3/8, 1/4, 1/16) at offset d = -2..2; products of two are exact.
__device__ __forceinline__ constexpr float tap_weight(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }
// The 3-tap Gaussian (1/4, 1/2, 1/4) of the variance prefilter; its products are 1/4, 1/8, 1/16.
__device__ __forceinline__ constexpr float gauss_weight(int d) { return d == 0 ? 0.5f : 0.25f; }

// What every lane of an a-trous pass is given (kernel argument).
struct DvPass {
  uint32_t W, H;
  int step;               // 2^i
  float kz;               // (1 / sigma_pos^2) * 4^-i
  uint32_t normal_power;
  float sigma_lum;
  // the last pass alone: the albedo to multiply back and the outputs
  const float* col;
  uint32_t demodulate;
  float4* out32;
  uchar4* out8;
  float* var;
};

// kl of valid pixel (x, y): 1 / (sigma_lum sqrt(g) + 1e-6), g the 3 x 3 Gaussian of the iterate's
// variance at unit spacing over the in-image valid pixels, normalised by the weights used.
__device__ __forceinline__ float lum_scale(const DvPass& a, const float4* __restrict__ cur, int x, int y) {
  const int W = (int)a.W, H = (int)a.H;
  const float* const cw = (const float*)cur;
  float gs = 0.0f, gw = 0.0f;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    const int qy = y + dy;
    const bool in_y = qy >= 0 && qy < H;
    const uint32_t row = (uint32_t)clampi(qy, H) * a.W;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const int qx = x + dx;
      const float vq = cw[4 * (row + (uint32_t)clampi(qx, W)) + 3];
      const bool use = in_y && qx >= 0 && qx < W && vq >= 0.0f;
      const float w = gauss_weight(dy) * gauss_weight(dx);
      gs = gs + (use ? w * vq : 0.0f);
      gw = gw + (use ? w : 0.0f);
    }
  }
  const float g = gs / gw;
  return 1.0f / (a.sigma_lum * sqrt_rn(g) + kLumEps);
}

// One tap of pixel p (normal np, position pp, luminance lp, scale kl) on q's record and iterate:
// sum += w c, wsum += w, vsum += (w w) v.  `centre`: q is p itself (w = h); `usable`: q lies in the
// image and is valid, else the tap is added as +0, not skipped.
__device__ __forceinline__ void add_tap(const DvPass& a, f3 np, f3 pp, float lp, float kl, float4 nq4, float4 pq4,
                                        float4 cq4, float h, bool centre, bool usable, f3& sum, float& wsum,
                                        float& vsum) {
  const float wn = normal_weight(np, xyz(nq4), a.normal_power);
  const float wz = plane_weight(np, pp, xyz(pq4), a.kz);
  const float wl = falloff(__builtin_fabsf(luminance(xyz(cq4)) - lp) * kl);
  const bool use = centre || usable;
  const float w = centre ? h : use ? ((h * wn) * wz) * wl : 0.0f;
  const f3 cq = use ? xyz(cq4) : f3{0.0f, 0.0f, 0.0f};
  const float vq = use ? cq4.w : 0.0f;
  sum = sum + w * cq;
  wsum = wsum + w;
  vsum = vsum + (w * w) * vq;
}

// The end of a pass for pixel i: its next iterate (c: the pixel's iterate, for a valid pixel
// replaced by the weighted means), or in the last pass the remodulated outputs (alpha: the input's,
// from the pixel's record).
template <bool LAST>
__device__ __forceinline__ void end_pass(const DvPass& a, uint32_t i, bool valid, float4 c, f3 sum, float wsum,
                                         float vsum, float alpha, float4* __restrict__ next) {
  if (valid) {
    c.x = sum.x / wsum;
    c.y = sum.y / wsum;
    c.z = sum.z / wsum;
    c.w = vsum / (wsum * wsum);
  }
  if (!LAST) {
    next[i] = c;
    return;
  }
  if (valid) {
    const f3 al = albedo(a.col, a.W * a.H, i, a.demodulate);
    c.x = c.x * al.x;
    c.y = c.y * al.y;
    c.z = c.z * al.z;
  }
  if (a.out32) a.out32[i] = make_float4(c.x, c.y, c.z, alpha);
  if (a.out8) a.out8[i] = make_uchar4(unorm8(c.x), unorm8(c.y), unorm8(c.z), 255);  // write_pixel's store
  if (a.var) a.var[i] = valid ? c.w : 0.0f;
}

// Form (a), the gather: each lane loads its 25 taps through the caches.
template <bool LAST>
__global__ void __launch_bounds__(kDvX * kDvY)
k_dv_atrous(const float4* __restrict__ rec, const float4* __restrict__ cur, float4* __restrict__ next, DvPass a) {
  uint32_t x, y;
  if (!pixel_of_block(a.W, a.H, x, y)) return;
  const int W = (int)a.W, H = (int)a.H;
  const uint32_t i = y * a.W + x;
  const float4 np4 = rec[2 * i], pp4 = rec[2 * i + 1];
  const float4 c = cur[i];
  const bool valid = np4.w != 0.0f;
  f3 sum{0.0f, 0.0f, 0.0f};
  float wsum = 0.0f, vsum = 0.0f;
  if (valid) {
    const f3 np = xyz(np4), pp = xyz(pp4);
    const float lp = luminance(xyz(c)), kl = lum_scale(a, cur, (int)x, (int)y);
    // the specification's order: dy outer, dx inner.  A tap outside the image is loaded from the
    // clamped address.
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
      const int qy = (int)y + dy * a.step;
      const bool in_y = qy >= 0 && qy < H;
      const uint32_t row = (uint32_t)clampi(qy, H) * a.W;
      const float hy = tap_weight(dy);
#pragma unroll
      for (int dx = -2; dx <= 2; ++dx) {
        const int qx = (int)x + dx * a.step;
        const bool in_q = in_y && qx >= 0 && qx < W;
        const uint32_t q = row + (uint32_t)clampi(qx, W);
        const float4 nq4 = rec[2 * q];
        add_tap(a, np, pp, lp, kl, nq4, rec[2 * q + 1], cur[q], hy * tap_weight(dx), dx == 0 && dy == 0,
                in_q && nq4.w != 0.0f, sum, wsum, vsum);
      }
    }
  }
  end_pass<LAST>(a, i, valid, c, sum, wsum, vsum, pp4.w, next);
}

// Form (b), LDS-tiled, wgt_denoise's layout: a workgroup owns 64 contiguous x by kDvY consecutive rows
// of one lattice (the pixels with y = r (mod s)) and first stages the kDvY + 4 lattice rows its taps
// reach, 64 + 4 s records wide, in LDS as three float4 planes (normal + tag, position, iterate).
// Entries outside the image are staged as not valid.  The variance prefilter's unit-spaced
// neighbours are read from global memory.
constexpr int kDvTileRows = kDvY + 4;
constexpr uint32_t dv_tile_cols(int step) { return (uint32_t)(kDvX + 4 * step); }
constexpr size_t dv_tile_bytes(int step) { return (size_t)kDvTileRows * dv_tile_cols(step) * 3 * sizeof(float4); }

template <bool LAST>
__global__ void __launch_bounds__(kDvX * kDvY)
k_dv_atrous_lds(const float4* __restrict__ rec, const float4* __restrict__ cur, float4* __restrict__ next, DvPass a,
                uint32_t residues) {
  extern __shared__ float4 s_tile[];
  const int W = (int)a.W, H = (int)a.H, s = a.step;
  const int tw = (int)dv_tile_cols(s);
  float4* const s_n = s_tile;
  float4* const s_p = s_tile + kDvTileRows * tw;
  float4* const s_c = s_tile + 2 * kDvTileRows * tw;
  const int r = (int)(blockIdx.y % residues), jg = (int)(blockIdx.y / residues);
  const int x0 = (int)blockIdx.x * kDvX;
  // row m of the tile is lattice row kDvY jg + m - 2, column c is x0 - 2 s + c
  for (int m = (int)threadIdx.y; m < kDvTileRows; m += kDvY) {
    const int qy = r + s * (kDvY * jg + m - 2);
    for (int col = (int)threadIdx.x; col < tw; col += kDvX) {
      const int qx = x0 - 2 * s + col;
      float4 n4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), p4 = n4, c4 = n4;
      if (qy >= 0 && qy < H && qx >= 0 && qx < W) {
        const uint32_t q = (uint32_t)qy * a.W + (uint32_t)qx;
        n4 = rec[2 * q];
        p4 = rec[2 * q + 1];
        c4 = cur[q];
      }
      s_n[m * tw + col] = n4;
      s_p[m * tw + col] = p4;
      s_c[m * tw + col] = c4;
    }
  }
  __syncthreads();
  const int x = x0 + (int)threadIdx.x, y = r + s * (kDvY * jg + (int)threadIdx.y);
  if (x >= W || y >= H) return;
  const uint32_t i = (uint32_t)y * a.W + (uint32_t)x;
  const int m0 = (int)threadIdx.y + 2, c0 = (int)threadIdx.x + 2 * s;
  const float4 np4 = s_n[m0 * tw + c0], pp4 = s_p[m0 * tw + c0];
  const float4 c = s_c[m0 * tw + c0];
  const bool valid = np4.w != 0.0f;
  f3 sum{0.0f, 0.0f, 0.0f};
  float wsum = 0.0f, vsum = 0.0f;
  if (valid) {
    const f3 np = xyz(np4), pp = xyz(pp4);
    const float lp = luminance(xyz(c)), kl = lum_scale(a, cur, x, y);
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
      const int row = (m0 + dy) * tw + c0;
      const float hy = tap_weight(dy);
#pragma unroll
      for (int dx = -2; dx <= 2; ++dx) {
        const int e = row + dx * s;
        const float4 nq4 = s_n[e];
        add_tap(a, np, pp, lp, kl, nq4, s_p[e], s_c[e], hy * tap_weight(dx), dx == 0 && dy == 0, nq4.w != 0.0f, sum,
                wsum, vsum);
      }
    }
  }
  end_pass<LAST>(a, i, valid, c, sum, wsum, vsum, pp4.w, next);
}

}  // namespace

hipError_t launch_denoise_variance(const DenoiseVariancePlan& p, const wgt_temporal_state& st, const wgt_hit_buffers& g,
                                   void* ws, float4* out32, uchar4* out8, float* var, hipStream_t stream) {
  // the callers' checks hold these: the kernels index in 32 bits and dereference what they are given
  if (p.W == 0 || p.H == 0 || p.W > kDenoiseMaxDim || p.H > kDenoiseMaxDim || (uint64_t)p.W * p.H > kDenoiseMaxPixels ||
      p.iterations < 1 || p.iterations > kDenoiseMaxIterations || p.normal_power > kDenoiseMaxNormalPower ||
      p.tiled_max_step > kDenoiseMaxTiledStep)
    return hipErrorInvalidValue;
  if (!st.rgba32f || !st.len || !st.moments || !g.prim || !g.pos || !g.norm || !g.col || !g.flags || !ws ||
      (!out32 && !out8))
    return hipErrorInvalidValue;
  float4* const rec = (float4*)((char*)ws + p.off_rec);
  float4* it[2] = {(float4*)((char*)ws + p.off_it0), (float4*)((char*)ws + p.off_it1)};
  const dim3 block(kDvX, kDvY), grid((p.W + kDvX - 1) / kDvX, (p.H + kDvY - 1) / kDvY);
  k_dv_pack<<<grid, block, 0, stream>>>((const float4*)st.rgba32f, st.len, st.moments, g, p.W, p.H, p.demodulate, p.min_history, rec, it[0]);
  k_dv_spatial<<<grid, block, 0, stream>>>(rec, st.len, st.moments, g.col, p.W, p.H, p.demodulate, p.normal_power,
                                           p.kz[0], p.min_history, it[0]);
  for (uint32_t i = 0; i < p.iterations; ++i) {
    const float4* cur = it[i & 1];
    float4* next = it[(i + 1) & 1];
    const bool last = i + 1 == p.iterations;
    const int step = 1 << i;
    const DvPass a{p.W, p.H, step, p.kz[i], p.normal_power, p.sigma_lum, last ? g.col : nullptr,
                   last ? p.demodulate : 0u, last ? out32 : nullptr, last ? out8 : nullptr, last ? var : nullptr};
    if ((uint32_t)step <= p.tiled_max_step) {
      // one workgroup per 64 x, lattice residue r < min(s, H) and group of kDvY lattice rows
      const uint32_t residues = (uint32_t)step < p.H ? (uint32_t)step : p.H;
      const uint32_t lattice_rows = (p.H + (uint32_t)step - 1) / (uint32_t)step;
      const dim3 tgrid(grid.x, residues * ((lattice_rows + kDvY - 1) / kDvY));
      if (last) k_dv_atrous_lds<true><<<tgrid, block, dv_tile_bytes(step), stream>>>(rec, cur, next, a, residues);
      else k_dv_atrous_lds<false><<<tgrid, block, dv_tile_bytes(step), stream>>>(rec, cur, next, a, residues);
    } else if (last) {
      k_dv_atrous<true><<<grid, block, 0, stream>>>(rec, cur, next, a);
    } else {
      k_dv_atrous<false><<<grid, block, 0, stream>>>(rec, cur, next, a);
    }
  }
  return hipGetLastError();
}

}  // namespace wgt
