// wgt_temporal.hip — temporal accumulation (wgt_temporal_accumulate, wgt_temporal_accumulate_async):
// each pixel of the current frame is reprojected into the previous frame through its first-hit
// position, gathers the caller's history there (bilinear, four taps, each accepted by its normal,
// its plane distance and optionally its primitive) and blends the current colour into it; in a
// translation unit of its own: it runs after the render kernels, on their outputs.
//
// The arithmetic is the specification's, operation by operation (tests/temporal_restatement.py is
// the same in numpy, and the outputs are equal bit for bit): binary32, no fused multiply-add
// (-ffp-contract=off), the compiler's correctly rounded division, denormals kept.
//
//   k_temporal : one pass, one lane per pixel, a 64 x 4 workgroup (a wave's row is contiguous).  The
//                previous frame's planar guides are gathered directly: a tap is tested cheapest
//                first (weight, bounds, length, primitive and flags, normal, position, colour) and
//                the loads of a tap that fails are skipped, which the running sums cannot tell from
//                adding +0.  No atomics, no scratch, no LDS; every index is checked against W x H.
//   k_temporal_motion : the same pixel code for wgt_temporal_accumulate_motion: the
//                history is looked up through the pixel's pos_prev and norm_prev, 24 B more per pixel.
#include "wgt_temporal.h"

#include "wgt_pixel.h"

namespace wgt {

namespace {

constexpr int kTaX = 64, kTaY = 4;
constexpr float kOkLimit = 0x1p100f;  // ok(v): every |component| <= 2^100 (NaN and inf fail)

__device__ __forceinline__ bool ok1(float v) { return __builtin_fabsf(v) <= kOkLimit; }
__device__ __forceinline__ bool ok3(f3 v) { return ok1(v.x) && ok1(v.y) && ok1(v.z); }
__device__ __forceinline__ f3 load_planar(const float* __restrict__ p, uint32_t n, uint32_t i) {
  return f3{p[i], p[(size_t)n + i], p[2 * (size_t)n + i]};
}
__device__ __forceinline__ f3 v3(const float (&a)[3]) { return f3{a[0], a[1], a[2]}; }

// project(camera, p): where p lands on the camera's image, in pixels (integers are pixel centres),
// and whether it lies in front of it.
__device__ __forceinline__ bool project(const TemporalCam& cam, f3 p, float& x, float& y) {
  const f3 q = p - v3(cam.o);
  const float z = dot(q, v3(cam.nrm));
  const float s = cam.k / z;
  const f3 r = s * q - v3(cam.c);
  x = dot(r, v3(cam.iu));
  y = dot(r, v3(cam.iv));
  return s > 0.0f && s <= kOkLimit;
}

// What every lane is given (kernel argument).
struct TaArgs {
  TemporalPlan p;
  const float4* in;
  wgt_hit_buffers g;
  // the previous frame (null pointers in the first-frame form)
  const float4* prev_rgba;
  const float* prev_len;
  const float* prev_mom;
  wgt_hit_buffers gp;
  float4* out_rgba;
  float* out_len;
  float* out_mom;
  uchar4* out8;
};

// One pixel.  MOTION (wgt_temporal_accumulate_motion): the previous camera projects the pixel's
// pos_prev, and a tap is tested against norm_prev and the plane through pos_prev (pos_prev and
// norm_prev: planar over W x H, read only where there is a previous frame); else both are the
// pixel's own position and normal, and the two pointers are unused.
template <bool MOMENTS, bool MOTION>
__device__ __forceinline__ void temporal_pixel(const TaArgs a, const float* __restrict__ pos_prev,
                                               const float* __restrict__ norm_prev) {
  const uint32_t W = a.p.W, H = a.p.H;
  const uint32_t X = blockIdx.x * kTaX + threadIdx.x, Y = blockIdx.y * kTaY + threadIdx.y;
  if (X >= W || Y >= H) return;
  const uint32_t n = W * H, i = Y * W + X;
  const float4 c = a.in[i];
  const uint32_t prim = a.g.prim[i];
  const f3 pos = load_planar(a.g.pos, n, i), norm = load_planar(a.g.norm, n, i), cur{c.x, c.y, c.z};
  const bool valid = prim != kNoHit && !(a.g.flags[i] & WGT_HIT_EMISSIVE) && ok3(pos) && ok3(norm) && ok3(cur);
  if (!valid) {  // lights, misses, NaN: the colour as it came, no history kept
    a.out_rgba[i] = c;
    a.out_len[i] = 0.0f;
    if (MOMENTS) {
      a.out_mom[i] = 0.0f;
      a.out_mom[(size_t)n + i] = 0.0f;
    }
    if (a.out8) a.out8[i] = make_uchar4(unorm8(c.x), unorm8(c.y), unorm8(c.z), 255);
    return;
  }
  float wsum = 0.0f, lsum = 0.0f, m1sum = 0.0f, m2sum = 0.0f;
  f3 csum{0.0f, 0.0f, 0.0f};
  if (!a.p.first) {
    float xc, yc, xp, yp;
    const f3 pp = MOTION ? load_planar(pos_prev, n, i) : pos, np = MOTION ? load_planar(norm_prev, n, i) : norm;
    const bool fc = project(a.p.cam, pos, xc, yc);
    const bool fp = project(a.p.cam_prev, pp, xp, yp) && (!MOTION || (ok3(pp) && ok3(np)));
    const float hx = (float)X + (xp - xc), hy = (float)Y + (yp - yc);
    if (fc && fp && hx > -1.0f && hx < (float)W && hy > -1.0f && hy < (float)H) {
      const float x0f = __builtin_floorf(hx), y0f = __builtin_floorf(hy);
      const float fx = hx - x0f, fy = hy - y0f;
      const int x0 = (int)x0f, y0 = (int)y0f;  // -1 .. W - 1 and -1 .. H - 1
#pragma unroll
      for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const float b = (k ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
          const int tx = x0 + k, ty = y0 + j;
          if (!(b > 0.0f) || tx < 0 || tx >= (int)W || ty < 0 || ty >= (int)H) continue;
          const uint32_t q = (uint32_t)ty * W + (uint32_t)tx;
          const float lt = a.prev_len[q];
          if (!(lt >= 1.0f)) continue;
          const uint32_t pq = a.gp.prim[q];
          if (pq == kNoHit || (a.gp.flags[q] & WGT_HIT_EMISSIVE) || (a.p.match_prim && pq != prim)) continue;
          const f3 nt = load_planar(a.gp.norm, n, q);
          if (!ok3(nt) || !(dot(np, nt) >= a.p.normal_min)) continue;
          const f3 pt = load_planar(a.gp.pos, n, q);
          if (!ok3(pt) || !(__builtin_fabsf(dot(np, pt - pp)) <= a.p.plane_tol)) continue;
          const float4 ct = a.prev_rgba[q];
          if (!ok3(f3{ct.x, ct.y, ct.z})) continue;
          wsum = wsum + b;
          csum = csum + b * f3{ct.x, ct.y, ct.z};
          lsum = lsum + b * lt;
          if (MOMENTS) {
            m1sum = m1sum + b * a.prev_mom[q];
            m2sum = m2sum + b * a.prev_mom[(size_t)n + q];
          }
        }
      }
    }
  }
  const float l = (0.2126f * cur.x + 0.7152f * cur.y) + 0.0722f * cur.z;
  f3 o = cur;
  const float ll = l * l;
  float len = 1.0f, m1 = l, m2 = ll;
  if (wsum >= kTemporalMinWeight) {
    const f3 hist = csum / wsum;
    const float hlen = lsum / wsum;
    const float up = hlen + 1.0f;
    len = up < a.p.max_history ? up : a.p.max_history;
    const float al = 1.0f / len;
    o = hist + al * (cur - hist);
    if (MOMENTS) {
      const float h1 = m1sum / wsum, h2 = m2sum / wsum;
      m1 = h1 + al * (l - h1);
      m2 = h2 + al * (ll - h2);
    }
  }
  a.out_rgba[i] = make_float4(o.x, o.y, o.z, c.w);
  a.out_len[i] = len;
  if (MOMENTS) {
    a.out_mom[i] = m1;
    a.out_mom[(size_t)n + i] = m2;
  }
  if (a.out8) a.out8[i] = make_uchar4(unorm8(o.x), unorm8(o.y), unorm8(o.z), 255);  // write_pixel's store
}

template <bool MOMENTS>
__global__ void __launch_bounds__(kTaX * kTaY) k_temporal(TaArgs a) {
  temporal_pixel<MOMENTS, false>(a, nullptr, nullptr);
}
// ... with the motion buffers beside the same arguments: k_temporal's own are laid out as before
template <bool MOMENTS>
__global__ void __launch_bounds__(kTaX * kTaY)
k_temporal_motion(TaArgs a, const float* __restrict__ pos_prev, const float* __restrict__ norm_prev) {
  temporal_pixel<MOMENTS, true>(a, pos_prev, norm_prev);
}

}  // namespace

hipError_t launch_temporal(const TemporalPlan& p, const float4* in, const wgt_hit_buffers& g,
                           const wgt_motion_buffers* motion, const wgt_temporal_state* prev, const wgt_hit_buffers* gprev,
                           const wgt_temporal_state& out, uchar4* out8, hipStream_t stream) {
  // the callers' checks hold these: the kernel indexes in 32 bits and dereferences what it is given
  if (p.W == 0 || p.H == 0 || p.W > 32768u || p.H > 32768u || (uint64_t)p.W * p.H > (1u << 25)) return hipErrorInvalidValue;
  if (!in || !g.prim || !g.pos || !g.norm || !g.flags || !out.rgba32f || !out.len) return hipErrorInvalidValue;
  if (!p.first && (!prev || !gprev || !prev->rgba32f || !prev->len || !gprev->prim || !gprev->pos || !gprev->norm ||
                   !gprev->flags || (out.moments && !prev->moments)))
    return hipErrorInvalidValue;
  if (!p.first && motion && (!motion->pos_prev || !motion->norm_prev)) return hipErrorInvalidValue;
  TaArgs a{};
  a.p = p;
  a.in = in;
  a.g = g;
  if (!p.first) {
    a.prev_rgba = (const float4*)prev->rgba32f;
    a.prev_len = prev->len;
    a.prev_mom = prev->moments;
    a.gp = *gprev;
  }
  a.out_rgba = (float4*)out.rgba32f;
  a.out_len = out.len;
  a.out_mom = out.moments;
  a.out8 = out8;
  const dim3 block(kTaX, kTaY), grid((p.W + kTaX - 1) / kTaX, (p.H + kTaY - 1) / kTaY);
  if (motion && !p.first) {  // the first-frame form reads no previous frame: the plain kernel
    if (out.moments) k_temporal_motion<true><<<grid, block, 0, stream>>>(a, motion->pos_prev, motion->norm_prev);
    else k_temporal_motion<false><<<grid, block, 0, stream>>>(a, motion->pos_prev, motion->norm_prev);
  } else if (out.moments) k_temporal<true><<<grid, block, 0, stream>>>(a);
  else k_temporal<false><<<grid, block, 0, stream>>>(a);
  return hipGetLastError();
}

}  // namespace wgt
