// wgt_hit.h — the hit record and the primitives tested without a tree: the quad and sphere
// tests, the quad scans (reference order, and the scan without per-quad distances), the hit
// of a NaN ray, and the merge of a finished traversal's triangle into the hit (finish_hit).
// Each function restates one piece of resources/shader/path_tracer.wgsl (cited per
// function), so every kernel that uses them computes bit-identical results.
#pragma once

#include "wgt_geom.h"
#include "wgt_internal.h"

namespace wgt {

struct Hit {
  float dist;
  uint32_t prim;
  bool emissive;
  bool front_face;
  f3 pos, norm, col;
};

__device__ __forceinline__ f3 xyz(float4 v) { return f3{v.x, v.y, v.z}; }

__device__ __forceinline__ void hit_init(Hit& h) {
  // HitInfo() zero-initialised, then path_tracer.wgsl:292-296
  h.dist = kRayMax;
  h.prim = kNoHit;
  h.emissive = false;
  h.front_face = false;
  h.pos = f3{0.0f, 0.0f, 0.0f};
  h.norm = f3{0.0f, 0.0f, 0.0f};
  h.col = f3{0.0f, 0.0f, 0.0f};
}

// Accept quad q at parameter t with distance ray_dist (tail of intersect_quad).
__device__ __forceinline__ void quad_accept(f3 o, f3 d, const float4* __restrict__ q, uint32_t id,
                                            float t, float ray_dist, Hit& h) {
  const f3 qn = xyz(q[3]);
  const bool ff = dot(d, qn) < 0.0f;
  const float4 c = q[5];
  h.dist = ray_dist;
  h.prim = id;
  h.emissive = c.w > 0.0f;
  h.front_face = ff;
  h.pos = o + t * d;
  h.norm = ff ? qn : -qn;
  h.col = xyz(c);
}

// path_tracer.wgsl:314-338.  `qt` receives t of the accepted quad: the triangle
// search bound, and what finalize needs to rebuild the quad hit bit for bit.
// EXACT: the compiler's IEEE division for t, for rays outside the render limits
// that make div_rn exact here (the ray queries' caller-supplied rays, wgt_math.h).
template <bool EXACT = false>
__device__ __forceinline__ void isect_quad(f3 o, f3 d, const float4* __restrict__ q, uint32_t id,
                                           Hit& h, float& qt) {
  const f3 qn = xyz(q[3]);
  const float denom = dot(qn, d);
  if (fabs_w(denom) < kRayMin) return;
  const float4 wd = q[4];
  const float num = wd.w - dot(qn, o);
  const float t = EXACT ? num / denom : div_rn(num, denom);
  if (t < kRayMin || kRayMax < t) return;
  // ray_dist is monotone non-decreasing in t >= 0 (each rounded step is), so t >=
  // qt (the accepted quad's t) implies ray_dist >= h.dist: the `>=` rejection
  // below, decided before the square root.  qt is +inf until a quad is accepted.
  if (t >= qt) return;
  const f3 pos = o + t * d;
  const float ray_dist = distance(pos, o);
  if (ray_dist >= h.dist) return;
  const f3 hit_vec = pos - xyz(q[0]);
  const f3 w = xyz(wd);
  const float a = dot(w, cross(hit_vec, xyz(q[2])));
  const float b = dot(w, cross(xyz(q[1]), hit_vec));
  // (a < 0) || (1 < a) || (b < 0) || (1 < b), NaN included: IEEE minNum/maxNum
  // return the non-NaN operand, and with both NaN every compare is false
  if ((__builtin_fminf(a, b) < 0.0f) || (1.0f < __builtin_fmaxf(a, b))) return;
  quad_accept(o, d, q, id, t, ray_dist, h);
  qt = t;
}

// path_tracer.wgsl:340-369 (sphere_uv is dead downstream: not computed)
__device__ __forceinline__ void isect_sphere(f3 o, f3 d, const float4* __restrict__ s, uint32_t id,
                                             Hit& h) {
  const float4 cr = s[0];
  const f3 center = xyz(cr);
  const f3 oc = o - center;
  const float a = dot(d, d);
  const float half_b = dot(oc, d);
  const float c = dot(oc, oc) - cr.w * cr.w;
  const float disc = half_b * half_b - a * c;
  if (disc < 0.0f) return;
  const float sqrt_d = sqrt_rn(disc);
  float root = (-half_b - sqrt_d) / a;
  if (root < kRayMin || kRayMax < root) {
    root = (-half_b + sqrt_d) / a;
    if (root < kRayMin || kRayMax < root) return;
  }
  const f3 pos = o + root * d;
  const float ray_dist = distance(pos, o);
  if (ray_dist >= h.dist) return;
  const f3 sn = (pos - center) / cr.w;
  const bool ff = dot(d, sn) < 0.0f;
  const float4 col = s[1];
  h.dist = ray_dist;
  h.prim = id;
  h.emissive = col.w > 0.0f;
  h.front_face = ff;
  h.pos = pos;
  h.norm = ff ? sn : -sn;
  h.col = xyz(col);
}

template <bool EXACT = false>
__device__ __forceinline__ void quad_scan(const DevScene& sc, f3 o, f3 d, Hit& h, float& qt) {
  hit_init(h);
  qt = __builtin_inff();
  const uint32_t nlq = sc.n_lights + sc.n_quads;
  for (uint32_t k = 0; k < nlq; ++k) {
    isect_quad<EXACT>(o, d, sc.quads + 6 * k, k, h, qt);
  }
}

// The quad scan of the persistent kernel: quad_scan's result (the accepted quad and its t) without
// the per-quad distance and its square root ("quad distance").
//
// quad_scan accepts quad k when it is valid (t in range, inside the quad) and its rounded distance
// f(t_k) = distance(o + t_k d, o) is below the best so far (kRayMax at first), so it returns the FIRST
// quad (scan order) whose f equals the minimum of f over the valid quads, provided that minimum is
// below kRayMax.  f is non-decreasing in t (every rounded step is), so the valid quad of smallest t
// (first on equal t) attains the minimum; this scan tracks that quad (t < qt, no distance) and the
// t of the best it replaced, `prev`: the smallest t of the valid quads before it in scan order.  Its
// answer is quad_scan's unless f(prev) == f(t) (an earlier quad ties in distance) or f(t) >= kRayMax.
// Both are excluded by a test on the max norms D = max|d_i|, L = max|o_i| (|.| <= ||.|| <= sqrt(3) |.|):
//   * f(t) < kRayMax when t D < 2^62, for ANY origin (render rays have L < 2^41 under the scene
//     limits; the ray queries' caller rays are not bounded).  With x_i = fl(t d_i), |x_i| <= t D (1 + eps),
//     eps = 2^-24: fl(o_i + x_i) is the float nearest o_i + x_i and o_i is a float |x_i| away from
//     it, so |fl(o_i + x_i) - o_i| <= 2 |x_i| whatever o_i is, and each component of pos - o is
//     within 2 t D (1 + 3 eps) < 2^63 (1 + 3 eps).  The three squares then sum to at most 12 t^2 D^2
//     (1 + 8 eps) < 0.75 2^128 (1 + 8 eps): no partial sum overflows, and f(t) <= sqrt(12) 2^62
//     (1 + 6 eps) = 1.6e19 < 1e20.  The bound was 2^64 until tests/test_gpu_query_range.py sent
//     diagonal rays from 2^63.5 away: from the render limits' L < 2^41 it followed that each
//     component is within t D (1 + 3 eps) + eps L, which gives f(t) < 1e20 but forgot the sum of the
//     squares, 3 (2^63.5)^2 > FLT_MAX: the reference computes an infinite distance and rejects the
//     quad, and this scan returned it;
//   * f(t) < f(prev) when g = (prev - t) - 2^-19 (prev + t) > 0, g D > 2^-18 L and prev D >= 2^-49: each
//     component of pos - o is t d_i within eps (3 |t d_i| + |o_i|), so ||pos - o|| is t ||d|| within
//     eps (3 t ||d|| + ||o||); the test (computed in fp32, whose roundings its factor-2 margins absorb)
//     gives (prev - t) ||d|| - 2^-20 (prev + t) ||d|| > 2^-19 ||o||, so the two exact norms differ by
//     >= 2^-21 prev ||d||, more than the dot product's and square root's roundings (2.6 eps relative,
//     2^-74 absolute from denormal squares) can close when prev ||d|| >= 2^-50.
// A lane that fails the test (an almost-tie: rays near the line where two quads meet) takes the
// reference scan, quad_scan; returns false for such a lane.  EXACT: as quad_scan<EXACT>.
template <bool EXACT = false>
__device__ __forceinline__ bool quad_scan_fast(const DevScene& sc, f3 o, f3 d, uint32_t& prim, float& qt) {
  prim = kNoHit;
  qt = __builtin_inff();
  float prev = __builtin_inff();
  const uint32_t nlq = sc.n_lights + sc.n_quads;
  for (uint32_t k = 0; k < nlq; ++k) {
    const float4* __restrict__ q = sc.quads + 6 * k;
    const f3 qn = xyz(q[3]);
    const float denom = dot(qn, d);
    if (fabs_w(denom) < kRayMin) continue;
    const float4 wd = q[4];
    const float num = wd.w - dot(qn, o);
    const float t = EXACT ? num / denom : div_rn(num, denom);
    if (t < kRayMin || kRayMax < t) continue;
    if (t >= qt) continue;
    const f3 pos = o + t * d;
    const f3 hit_vec = pos - xyz(q[0]);
    const f3 w = xyz(wd);
    const float a = dot(w, cross(hit_vec, xyz(q[2])));
    const float b = dot(w, cross(xyz(q[1]), hit_vec));
    if ((__builtin_fminf(a, b) < 0.0f) || (1.0f < __builtin_fmaxf(a, b))) continue;
    prev = qt;
    qt = t;
    prim = k;
  }
  bool exact = true;
  if (prim != kNoHit) {
    const float D = __builtin_fmaxf(__builtin_fmaxf(fabs_w(d.x), fabs_w(d.y)), fabs_w(d.z));
    const float L = __builtin_fmaxf(__builtin_fmaxf(fabs_w(o.x), fabs_w(o.y)), fabs_w(o.z));
    exact = qt * D < 0x1p62f;
    if (prev != __builtin_inff()) {
      const float g = (prev - qt) - 0x1p-19f * (prev + qt);
      exact = exact && g * D > 0x1p-18f * L && prev * D >= 0x1p-49f;
    }
  }
  if (!exact) {
    Hit h;
    quad_scan<EXACT>(sc, o, d, h, qt);
    prim = h.prim;
  }
  return exact;
}

// The quad part of a hit rebuilt from (prim, t): the same operations as isect_quad.
__device__ __forceinline__ void quad_rebuild(const DevScene& sc, f3 o, f3 d, uint32_t prim, float t,
                                             Hit& h) {
  hit_init(h);
  if (prim == kNoHit) return;
  const f3 pos = o + t * d;
  quad_accept(o, d, sc.quads + 6 * prim, prim, t, distance(pos, o), h);
}

__device__ __forceinline__ uint32_t last_prim(const DevScene& sc) {
  return sc.n_lights + sc.n_quads + sc.n_tris + sc.n_spheres - 1u;
}

// A NaN ray's hit: the last sphere (every rejection test is false for NaN).
__device__ __forceinline__ void nan_hit(const DevScene& sc, f3 o, f3 d, Hit& h) {
  hit_init(h);
  const uint32_t k = sc.n_spheres - 1;
  isect_sphere(o, d, sc.spheres + 2 * k, sc.n_lights + sc.n_quads + sc.n_tris + k, h);
}

// Merge the triangle result into the quad hit, then scan the spheres: the end of
// sample_hit (path_tracer.wgsl:305-309) with triangles between quads and spheres.
// PRELOAD: the triangle's shading record is read before the quad hit is rebuilt (the
// caller issues both loads together, preload_tshade) instead of after the distance
// comparison that needs it: one memory round trip per finalise instead of two.
// The triangle result of a finished traversal: (bt, bi), bi = kNoHit when no
// triangle was accepted (Trav::bt, Trav::bi of wgt_trav.h).
__device__ __forceinline__ void preload_tshade(const DevScene& sc, uint32_t bi, float4& s0, float4& s1) {
  const uint32_t i = bi != kNoHit ? bi : 0u;  // record 0 for a ray without a triangle hit: unused
  s0 = sc.tshade[2 * i];
  s1 = sc.tshade[2 * i + 1];
}
__device__ __forceinline__ void finish_hit(const DevScene& sc, f3 o, f3 d, float bt, uint32_t bi, Hit& h,
                                           const float4* pre = nullptr) {
  const uint32_t nlq = sc.n_lights + sc.n_quads;
  if (bi != kNoHit) {
    const f3 pos = o + bt * d;
    const float ray_dist = distance(pos, o);
    if (!(ray_dist >= h.dist)) {
      const float4 s0 = pre ? pre[0] : sc.tshade[2 * bi], s1 = pre ? pre[1] : sc.tshade[2 * bi + 1];
      const f3 fn = xyz(s0);
      const bool ff = dot(d, fn) < 0.0f;
      h.dist = ray_dist;
      h.prim = nlq + bi;
      h.emissive = s0.w > 0.0f;
      h.front_face = ff;
      h.pos = pos;
      h.norm = ff ? fn : -fn;
      h.col = xyz(s1);
    }
  }
  for (uint32_t k = 0; k < sc.n_spheres; ++k)
    isect_sphere(o, d, sc.spheres + 2 * k, nlq + sc.n_tris + k, h);
}

}  // namespace wgt
