// wgt_compact.h — the arithmetic of the compact node form (wgt_geom.h), shared by the host
// builder (host/bvh.cpp CompactForm) and the device refit (wgt_refit.hip): one statement of
// every f64 operation, so that the codes either side computes are the same bits.  Plain IEEE
// +, -, *, / and conversions, no contraction (-ffp-contract=off), no library calls.
//
// The kernel evaluates a child plane's slab distance as fma(h, s/d, c) with c = fma(org/s,
// s/d, ot) per node and axis (one fused step instead of decoding the plane first), so the
// codes keep a margin G from the exact child bounds: a lo code's plane org' + h*s (org' =
// the stored org/s times s) lies <= lo - G, a hi code's >= hi + G.  G = 2^-21 * M, with M
// >= |org'| and >= |ray origin| (BvhOptions::origin_bound), covers the rounding of c
// (DESIGN.md §3.4): every decoded interval then contains, bit for bit, the slab interval
// fma(b, 1/d, ot) of every triangle box b below the child.  Codes are the tightest binary16
// values with the margin (non-negative half bit patterns order like their values, so a
// binary search finds them).
#pragma once

#include "wgt_geom.h"

namespace wgt {

// A 128-B node as 32 floats (wgt_geom.h): plane rows lo.x hi.x lo.y hi.y lo.z hi.z of 4 slots.
WGT_HD float node_lo(const float* n, int axis, int slot) { return n[(2 * axis) * 4 + slot]; }
WGT_HD float node_hi(const float* n, int axis, int slot) { return n[(2 * axis + 1) * 4 + slot]; }
WGT_HD bool node_live(const float* n, int slot) {
  return !(node_lo(n, 0, slot) == kEmptySlotCoord && node_hi(n, 0, slot) == kEmptySlotCoord);
}

constexpr double kCompactInf = __builtin_huge_val();

// The next float below f (nextafter(f, -inf)) of a non-NaN f.
WGT_HD float float_below(float f) {
  const uint32_t b = __builtin_bit_cast(uint32_t, f);
  if (f == 0.0f) return __builtin_bit_cast(float, 0x80000001u);
  return __builtin_bit_cast(float, f > 0.0f ? b - 1u : b + 1u);
}

// The union of the node's live slots on one axis.
WGT_HD void node_axis_union(const float* n, int a, double& ulo, double& uhi) {
  ulo = kCompactInf;
  uhi = -kCompactInf;
  for (int i = 0; i < kBvhWidth; ++i)
    if (node_live(n, i)) {
      const double l = (double)node_lo(n, a, i), h = (double)node_hi(n, a, i);
      ulo = l < ulo ? l : ulo;
      uhi = uhi < h ? h : uhi;
    }
}

WGT_HD double cdec(uint32_t h, double s, double orgd) { return orgd + (double)half_bits_to_float(h) * s; }

// The 16 words of one node's compact form for the step s and margin G.
WGT_HD void compact_node(const float* n, float s, double G, uint32_t* q) {
  for (int a = 0; a < 3; ++a) {
    double ulo, uhi;
    node_axis_union(n, a, ulo, uhi);
    // org/s as a float whose value times s is <= ulo - G
    const double target = (ulo - G) / (double)s;
    float f = (float)target;
    while ((double)f > target) f = float_below(f);
    q[a] = __builtin_bit_cast(uint32_t, f);
    const double orgd = (double)f * (double)s;
    uint32_t lo_h[kBvhWidth], hi_h[kBvhWidth];
    for (int i = 0; i < kBvhWidth; ++i) {
      lo_h[i] = hi_h[i] = 0x7c00u;  // an empty slot: +inf planes on every axis, never entered
      if (!node_live(n, i)) continue;
      const double blo = (double)node_lo(n, a, i) - G, bhi = (double)node_hi(n, a, i) + G;
      uint32_t l = 0, r = 0x7bffu;  // largest h with plane <= blo (h = 0 is: orgd <= ulo - G)
      while (l < r) {
        const uint32_t m = (l + r + 1) / 2;
        if (cdec(m, s, orgd) <= blo) l = m; else r = m - 1;
      }
      lo_h[i] = l;
      l = 0; r = 0x7bffu;  // smallest h with plane >= bhi (compact_step_ok guarantees h = 65504 is)
      while (l < r) {
        const uint32_t m = (l + r) / 2;
        if (cdec(m, s, orgd) >= bhi) r = m; else l = m + 1;
      }
      hi_h[i] = l;
    }
    q[4 + 4 * a + 0] = lo_h[0] | (lo_h[1] << 16);
    q[4 + 4 * a + 1] = lo_h[2] | (lo_h[3] << 16);
    q[4 + 4 * a + 2] = hi_h[0] | (hi_h[1] << 16);
    q[4 + 4 * a + 3] = hi_h[2] | (hi_h[3] << 16);
  }
  q[3] = 0u;  // reserved
}

// Code 65504 reaches the node's upper bounds plus the margins with the step s (the origin
// sits up to G + one float step of org/s below the lower bound).  Monotone in s.
WGT_HD bool compact_step_ok(const float* n, float s, double G) {
  for (int a = 0; a < 3; ++a) {
    double ulo, uhi;
    node_axis_union(n, a, ulo, uhi);
    const double org_low = ulo - G - (__builtin_fabs(ulo - G) * 0x1p-23 + (double)s * 0x1p-126);
    if (!(org_low + 65504.0 * (double)s >= uhi + G)) return false;
  }
  return true;
}

// 2^e as a float, -126 <= e <= 128 (128: +inf, which every node accepts).
WGT_HD float pow2f(int e) { return __builtin_bit_cast(float, (uint32_t)(e + 127) << 23); }
constexpr int kCompactMinExp = -24, kCompactMaxExp = 128;
// The exponent of the smallest step 2^e, e >= kCompactMinExp, this node accepts; the scene's
// step is the largest over its nodes.
WGT_HD int compact_node_exp(const float* n, double G) {
  int e = kCompactMinExp;
  while (e < kCompactMaxExp && !compact_step_ok(n, pow2f(e), G)) ++e;
  return e;
}

}  // namespace wgt
