// wgt_morton.h — the arithmetic of the Morton-order rebuild, shared by the host
// specification (host/bvh.cpp BuildMortonBvh) and the device build (wgt_rebuild.hip): one statement
// of the key, of a split and of a node's slots, so that the topology either side makes is the same.
// The key's f64 operations are plain IEEE -, /, * and conversions, no contraction, no library calls.
#pragma once

#include "wgt_geom.h"

namespace wgt {

constexpr uint32_t kMortonBits = 21;    // per axis: 63-bit codes
constexpr uint32_t kRebuildLevels = 10;  // BVH4 levels of a rebuilt tree at the most: 20 binary levels
constexpr uint32_t kRebuildLeafDefault = 4;

// The largest triangle count a rebuild takes for the leaf target L: L * 4^kRebuildLevels.
constexpr uint64_t rebuild_max_tris(uint32_t L) { return (uint64_t)L << (2 * kRebuildLevels); }

// A triangle's centre on one axis, as the host builder's Prim::c.
WGT_HD float morton_centre(float lo, float hi) { return 0.5f * lo + 0.5f * hi; }

// The 21-bit cell of centre c between the centres' exact bounds cmin <= c <= cmax on one axis.
WGT_HD uint32_t morton_cell(float c, float cmin, float cmax) {
  const double d = (double)cmax - (double)cmin;
  if (!(d > 0.0)) return 0u;
  const uint32_t q = (uint32_t)(((double)c - (double)cmin) / d * 2097152.0);
  return q < (1u << kMortonBits) - 1u ? q : (1u << kMortonBits) - 1u;
}

// Bit k of v at bit 3k.
WGT_HD unsigned long long morton_spread(uint32_t v) {
  unsigned long long x = v & 0x1fffffu;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}
// x's bit k at 3k + 2, y's at 3k + 1, z's at 3k.
WGT_HD unsigned long long morton_code(uint32_t qx, uint32_t qy, uint32_t qz) {
  return morton_spread(qx) << 2 | morton_spread(qy) << 1 | morton_spread(qz);
}

// split(b, e, r) of the e - b >= 2 sorted codes [b, e) with r binary levels left, for the leaf
// target L: the first key whose code has the highest bit in which the range's first and last codes
// differ, when neither part then exceeds what r - 1 levels hold (L * 2^(r-1)); else the median.
WGT_HD uint32_t morton_split(const unsigned long long* code, uint32_t b, uint32_t e, uint32_t r, uint32_t L) {
  const unsigned long long first = code[b], diff = first ^ code[e - 1];
  if (diff != 0ull) {
    const int h = 63 - __builtin_clzll(diff);
    const unsigned long long bound = (first >> h | 1ull) << h;  // the common prefix, bit h set, zeros below
    uint32_t lo = b + 1, hi = e - 1;                            // the least p with code[p] >= bound: b < p <= e - 1
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (code[mid] >= bound) hi = mid; else lo = mid + 1;
    }
    const uint32_t big = lo - b > e - lo ? lo - b : e - lo;
    if ((uint64_t)big <= (uint64_t)L << (r - 1)) return lo;
  }
  return b + (e - b + 1) / 2;
}

// The slots of the node over [b, e), e - b > L, with r >= 2 levels left: cut[0] = b < ... < cut[n] = e
// are the 2..4 parts in key order (cut[n + 1 .. 4] = e too); returns n.  One split, then each part of
// more than L keys again.  Constant indices only: the device keeps cut in registers.
WGT_HD int morton_slots(const unsigned long long* code, uint32_t b, uint32_t e, uint32_t r, uint32_t L, uint32_t* cut) {
  const uint32_t p = morton_split(code, b, e, r, L);
  const bool left = p - b > L, right = e - p > L;
  const uint32_t pl = left ? morton_split(code, b, p, r - 1, L) : p;
  const uint32_t pr = right ? morton_split(code, p, e, r - 1, L) : e;
  cut[0] = b;
  cut[1] = left ? pl : p;
  cut[2] = left ? p : pr;
  cut[3] = left ? pr : e;
  cut[4] = e;
  return 2 + (left ? 1 : 0) + (right ? 1 : 0);
}

}  // namespace wgt
