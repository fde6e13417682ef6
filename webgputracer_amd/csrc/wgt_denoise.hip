// wgt_denoise.hip — the denoiser (wgt_denoise, wgt_denoise_async): an edge-avoiding a-trous wavelet
// filter over a rendered image, guided by its first-hit G-buffer and demodulated by albedo, in a
// translation unit of its own: it runs after the render kernels, on their output.
//
// The arithmetic is the specification's, operation by operation (tests/denoise_restatement.py is
// the same in numpy, and the outputs are equal bit for bit): binary32, no fused multiply-add
// (-ffp-contract=off), the compiler's correctly rounded division, denormals kept.
//
//   k_dn_pack   : the mask, the albedo divisor and the first iterate; one packed guide record per
//                 pixel (DenoisePlan), so that a tap costs three 16-byte loads, not ten planar dwords
//   k_dn_atrous_lds, k_dn_atrous : one iterate to the next, 25 taps at a step of 2^i pixels; the last
//                 pass remodulates and writes the outputs.  Steps up to DenoisePlan::tiled_max_step
//                 stage their taps in LDS (measured faster up to a step of 8), larger steps gather
//                 each lane's taps through the caches
// A workgroup is 64 x 4 pixels: a wave's loads and stores of a row are 1 KiB contiguous.  Every
// kernel checks its pixel against W x H; taps outside the image are clamped into it (the gather) or
// staged as not valid (the tile).  No atomics, no scratch.
#include "wgt_denoise.h"

#include "wgt_pixel.h"

namespace wgt {

namespace {

constexpr int kDnX = 64, kDnY = 4;
constexpr float kOkLimit = 0x1p100f;   // ok(v): every |component| <= 2^100 (NaN and inf fail)
constexpr float kAlbedoMin = 0x1p-8f;  // the demodulation divisor's floor

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

__device__ __forceinline__ bool pixel_of_block(uint32_t W, uint32_t H, uint32_t& x, uint32_t& y) {
  x = blockIdx.x * kDnX + threadIdx.x;
  y = blockIdx.y * kDnY + threadIdx.y;
  return x < W && y < H;
}

__global__ void __launch_bounds__(kDnX * kDnY)
k_dn_pack(const float4* __restrict__ in, wgt_hit_buffers g, uint32_t W, uint32_t H, uint32_t demodulate,
          float4* __restrict__ rec, float4* __restrict__ it0) {
  uint32_t x, y;
  if (!pixel_of_block(W, H, x, y)) return;
  const uint32_t n = W * H, i = y * W + x;
  const float4 c = in[i];
  const f3 pos = load_planar(g.pos, n, i), norm = load_planar(g.norm, n, i), col = load_planar(g.col, n, i);
  const bool valid = g.prim[i] != kNoHit && !(g.flags[i] & WGT_HIT_EMISSIVE) && ok3(pos) && ok3(norm) && ok3(col) &&
                     ok3(xyz(c));
  const f3 a = albedo(g.col, n, i, demodulate);
  rec[2 * i] = make_float4(norm.x, norm.y, norm.z, valid ? 1.0f : 0.0f);
  rec[2 * i + 1] = make_float4(pos.x, pos.y, pos.z, 0.0f);
  // a pixel that is not valid carries its colour through the passes as it came
  it0[i] = valid ? make_float4(c.x / a.x, c.y / a.y, c.z / a.z, c.w) : c;
}

// The 5-tap B3 spline kernel (1/16, 1/4, 3/8, 1/4, 1/16) at offset d = -2..2; products of two are exact.
__device__ __forceinline__ constexpr float tap_weight(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// What every lane of an a-trous pass is given (kernel argument).
struct DnPass {
  uint32_t W, H;
  int step;               // 2^i
  float kz;               // (1 / sigma_pos^2) * 4^-i
  uint32_t normal_power;
  // the last pass alone: the albedo to multiply back and the outputs
  const float* col;
  uint32_t demodulate;
  float4* out32;
  uchar4* out8;
};

// One tap of pixel p (normal np, position pp) on q's record and iterate: sum += w c, wsum += w.
// `centre`: q is p itself (w = h, c = cur(p)); `usable`: q lies in the image and is valid, else the
// tap is added as (+0, +0), not skipped.
__device__ __forceinline__ void add_tap(const DnPass& a, f3 np, f3 pp, float4 nq4, float4 pq4, float4 cq4, float h,
                                        bool centre, bool usable, f3& sum, float& wsum) {
  float wn = max0(dot(np, xyz(nq4)));
  for (uint32_t k = 0; k < a.normal_power; ++k) wn = wn * wn;
  const float d = dot(np, xyz(pq4) - pp);
  const float wz = falloff((d * d) * a.kz);
  const bool use = centre || usable;
  const float w = centre ? h : use ? (h * wn) * wz : 0.0f;
  const f3 cq = use ? xyz(cq4) : f3{0.0f, 0.0f, 0.0f};
  sum = sum + w * cq;
  wsum = wsum + w;
}

// The end of a pass for pixel i: its next iterate (c: the pixel's iterate, for a valid pixel
// replaced by sum / wsum), or in the last pass the remodulated outputs.
template <bool LAST>
__device__ __forceinline__ void end_pass(const DnPass& a, uint32_t i, bool valid, float4 c, f3 sum, float wsum,
                                         float4* __restrict__ next) {
  if (valid) {
    c.x = sum.x / wsum;
    c.y = sum.y / wsum;
    c.z = sum.z / wsum;
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
  if (a.out32) a.out32[i] = c;
  if (a.out8) a.out8[i] = make_uchar4(unorm8(c.x), unorm8(c.y), unorm8(c.z), 255);  // write_pixel's store
}

// Form (a), the gather: each lane loads its 25 taps through the caches.
template <bool LAST>
__global__ void __launch_bounds__(kDnX * kDnY)
k_dn_atrous(const float4* __restrict__ rec, const float4* __restrict__ cur, float4* __restrict__ next, DnPass a) {
  uint32_t x, y;
  if (!pixel_of_block(a.W, a.H, x, y)) return;
  const int W = (int)a.W, H = (int)a.H;
  const uint32_t i = y * a.W + x;
  const float4 np4 = rec[2 * i];
  const float4 c = cur[i];
  const bool valid = np4.w != 0.0f;
  f3 sum{0.0f, 0.0f, 0.0f};
  float wsum = 0.0f;
  if (valid) {
    const f3 np = xyz(np4), pp = xyz(rec[2 * i + 1]);
    // the specification's order: dy outer, dx inner.  A tap outside the image is loaded from the
    // clamped address.
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
      const int qy = (int)y + dy * a.step;
      const bool in_y = qy >= 0 && qy < H;
      const uint32_t row = (uint32_t)(qy < 0 ? 0 : qy >= H ? H - 1 : qy) * a.W;
      const float hy = tap_weight(dy);
#pragma unroll
      for (int dx = -2; dx <= 2; ++dx) {
        const int qx = (int)x + dx * a.step;
        const bool in_q = in_y && qx >= 0 && qx < W;
        const uint32_t q = row + (uint32_t)(qx < 0 ? 0 : qx >= W ? W - 1 : qx);
        const float4 nq4 = rec[2 * q];
        add_tap(a, np, pp, nq4, rec[2 * q + 1], cur[q], hy * tap_weight(dx), dx == 0 && dy == 0,
                in_q && nq4.w != 0.0f, sum, wsum);
      }
    }
  }
  end_pass<LAST>(a, i, valid, c, sum, wsum, next);
}

// Form (b), LDS-tiled.  The taps of a pixel lie on its own lattice, the pixels with y = r (mod s)
// and any x.  A workgroup owns 64 contiguous x by kDnY consecutive rows of one such lattice (rows
// r + s (kDnY jg + k), k = 0 .. kDnY - 1) and first stages the kDnY + 4 lattice rows its taps reach,
// 64 + 4 s records wide, in LDS as three float4 planes (normal + valid, position, iterate): every tap
// is then three 16-byte LDS reads at a stride of 16 bytes per lane, and the global loads are
// contiguous in x.  Entries outside the image are staged as not valid.
constexpr int kDnTileRows = kDnY + 4;
constexpr uint32_t dn_tile_cols(int step) { return (uint32_t)(kDnX + 4 * step); }
constexpr size_t dn_tile_bytes(int step) { return (size_t)kDnTileRows * dn_tile_cols(step) * 3 * sizeof(float4); }

template <bool LAST>
__global__ void __launch_bounds__(kDnX * kDnY)
k_dn_atrous_lds(const float4* __restrict__ rec, const float4* __restrict__ cur, float4* __restrict__ next, DnPass a,
                uint32_t residues) {
  extern __shared__ float4 s_tile[];
  const int W = (int)a.W, H = (int)a.H, s = a.step;
  const int tw = (int)dn_tile_cols(s);
  float4* const s_n = s_tile;
  float4* const s_p = s_tile + kDnTileRows * tw;
  float4* const s_c = s_tile + 2 * kDnTileRows * tw;
  const int r = (int)(blockIdx.y % residues), jg = (int)(blockIdx.y / residues);
  const int x0 = (int)blockIdx.x * kDnX;
  // row m of the tile is lattice row kDnY jg + m - 2, column c is x0 - 2 s + c
  for (int m = (int)threadIdx.y; m < kDnTileRows; m += kDnY) {
    const int qy = r + s * (kDnY * jg + m - 2);
    for (int col = (int)threadIdx.x; col < tw; col += kDnX) {
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
  const int x = x0 + (int)threadIdx.x, y = r + s * (kDnY * jg + (int)threadIdx.y);
  if (x >= W || y >= H) return;
  const uint32_t i = (uint32_t)y * a.W + (uint32_t)x;
  const int m0 = (int)threadIdx.y + 2, c0 = (int)threadIdx.x + 2 * s;
  const float4 np4 = s_n[m0 * tw + c0];
  const float4 c = s_c[m0 * tw + c0];
  const bool valid = np4.w != 0.0f;
  f3 sum{0.0f, 0.0f, 0.0f};
  float wsum = 0.0f;
  if (valid) {
    const f3 np = xyz(np4), pp = xyz(s_p[m0 * tw + c0]);
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
      const int row = (m0 + dy) * tw + c0;
      const float hy = tap_weight(dy);
#pragma unroll
      for (int dx = -2; dx <= 2; ++dx) {
        const int e = row + dx * s;
        const float4 nq4 = s_n[e];
        add_tap(a, np, pp, nq4, s_p[e], s_c[e], hy * tap_weight(dx), dx == 0 && dy == 0, nq4.w != 0.0f, sum, wsum);
      }
    }
  }
  end_pass<LAST>(a, i, valid, c, sum, wsum, next);
}

}  // namespace

hipError_t launch_denoise(const DenoisePlan& p, const float4* in, const wgt_hit_buffers& g, void* ws, float4* out32,
                          uchar4* out8, hipStream_t stream) {
  if (p.W == 0 || p.H == 0 || p.W > kDenoiseMaxDim || p.H > kDenoiseMaxDim || (uint64_t)p.W * p.H > kDenoiseMaxPixels ||
      p.iterations < 1 || p.iterations > kDenoiseMaxIterations || p.normal_power > kDenoiseMaxNormalPower ||
      p.tiled_max_step > kDenoiseMaxTiledStep)
    return hipErrorInvalidValue;  // the callers' checks hold these: the kernels index in 32 bits
  float4* const rec = (float4*)((char*)ws + p.off_rec);
  float4* it[2] = {(float4*)((char*)ws + p.off_it0), (float4*)((char*)ws + p.off_it1)};
  const dim3 block(kDnX, kDnY), grid((p.W + kDnX - 1) / kDnX, (p.H + kDnY - 1) / kDnY);
  k_dn_pack<<<grid, block, 0, stream>>>(in, g, p.W, p.H, p.demodulate, rec, it[0]);
  for (uint32_t i = 0; i < p.iterations; ++i) {
    const float4* cur = it[i & 1];
    float4* next = it[(i + 1) & 1];
    const bool last = i + 1 == p.iterations;
    const int step = 1 << i;
    const DnPass a{p.W, p.H, step, p.kz[i], p.normal_power, last ? g.col : nullptr, last ? p.demodulate : 0u,
                   last ? out32 : nullptr, last ? out8 : nullptr};
    if ((uint32_t)step <= p.tiled_max_step) {
      // one workgroup per 64 x, lattice residue r < min(s, H) and group of kDnY lattice rows
      const uint32_t residues = (uint32_t)step < p.H ? (uint32_t)step : p.H;
      const uint32_t lattice_rows = (p.H + (uint32_t)step - 1) / (uint32_t)step;
      const dim3 tgrid(grid.x, residues * ((lattice_rows + kDnY - 1) / kDnY));
      if (last) k_dn_atrous_lds<true><<<tgrid, block, dn_tile_bytes(step), stream>>>(rec, cur, next, a, residues);
      else k_dn_atrous_lds<false><<<tgrid, block, dn_tile_bytes(step), stream>>>(rec, cur, next, a, residues);
    } else if (last) {
      k_dn_atrous<true><<<grid, block, 0, stream>>>(rec, cur, next, a);
    } else {
      k_dn_atrous<false><<<grid, block, 0, stream>>>(rec, cur, next, a);
    }
  }
  return hipGetLastError();
}

}  // namespace wgt
