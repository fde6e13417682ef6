// wgt_radiance.hip — radiance queries (wgt_trace_radiance): compute_sample's path loop
// (path_tracer.wgsl:386-393) on the caller's rays, one RNG state per ray, in a translation unit of
// its own, away from the render kernels and their register budgets.
//
// Work item i is a ray (o, d) with a start state s: `samples` paths from (o, d), each the renderer's
// raytrace() per bounce (closest_hit or the phase-split steps, then shade, wgt_pixel.h), the
// NaN skip-ahead as in the render kernels, col += max(path.col, 0) / f32(samples) per path.  Outputs:
// the colour, the primitive of the first path's first hit, the final state.
//
// Two forms, bit-identical:
//  * k_radiance (flat): one ray per lane, k_render's loop with the ray read from the input where
//    k_render calls camera_ray.  Scenes without triangles, WGT_KERNEL=1, and the reference form.
//  * k_radiance_ps (persistent, phase-split): k_render_ps's structure on a ray queue in index
//    order: the grid is the resident wave capacity, idle lanes take consecutive ray indices from a
//    launch-wide counter (one atomic per wave refill), the service phase writes a finished ray,
//    refills, reloads the ray for the next sample, finalises, shades, scans the quads and tests the
//    root; the traversal phase runs node_step and tri_step (wgt_trav_ps.h).  No LPT order, no cost
//    pre-pass, no parked state: the whole stack is in LDS.
#include <type_traits>

#include "wgt_hit.h"
#include "wgt_pixel.h"
#include "wgt_radiance.h"
#include "wgt_trav.h"
#include "wgt_trav_ps.h"

namespace wgt {

namespace {

__device__ __forceinline__ void load_ray(const float* __restrict__ rays, size_t n, size_t i, f3& o, f3& d) {
  o = f3{rays[i], rays[n + i], rays[2 * n + i]};
  d = f3{rays[3 * n + i], rays[4 * n + i], rays[5 * n + i]};
}

// col += max(path.col, 0) / f32(samples) (path_tracer.wgsl:393): x / 2^k == x * 2^-k exactly, so a
// power-of-two count multiplies (end_sample's rule, wgt_pixel.h)
__device__ __forceinline__ void add_sample(const RadianceArgs& a, f3& col, f3 pc) {
  const f3 m{max0(pc.x), max0(pc.y), max0(pc.z)};
  col = col + (a.inv_fs != 0.0f ? a.inv_fs * m : m / a.fs);
}

// Ray i's outputs: plain vector stores, each behind a wave-uniform null test (the pointers are
// kernel arguments of their own, __restrict__: their stores clobber nothing the scene's
// wave-uniform loads read, which therefore stay scalar loads).
__device__ __forceinline__ void store_ray(float* __restrict__ rgb, uint32_t* __restrict__ prim,
                                          uint32_t* __restrict__ seed_out, size_t n, size_t i, f3 col,
                                          uint32_t first, uint32_t seed) {
  if (rgb) {
    rgb[i] = col.x;
    rgb[n + i] = col.y;
    rgb[2 * n + i] = col.z;
  }
  if (prim) prim[i] = first;
  if (seed_out) seed_out[i] = seed;
}

// counts[0..3] = sample_hit calls, those on rays without NaN, paths, those on NaN rays (O_CNT_*)
struct RadCounts {
  uint32_t q, tr, nan;
};
__device__ __forceinline__ void flush_counts(unsigned long long* __restrict__ counters, const RadCounts& c,
                                             unsigned long long paths) {
  atomicAdd(&counters[0], (unsigned long long)c.q);
  atomicAdd(&counters[1], (unsigned long long)c.tr);
  atomicAdd(&counters[2], paths);
  atomicAdd(&counters[3], (unsigned long long)c.nan);
}
// NaN-absorbed for the rest of the path (skip_nan_path, wgt_pixel.h): 3 rand() per remaining bounce
template <bool STATS>
__device__ __forceinline__ void skip_nan(uint32_t& seed, int depth, RadCounts& c) {
  seed = lcg_jump(seed, 3u * (uint32_t)(kRayDepth - depth));
  if (STATS) {
    c.q += (uint32_t)(kRayDepth - depth);
    c.nan += (uint32_t)(kRayDepth - depth);
  }
}

template <bool TRIS, bool STATS>
__global__ void __launch_bounds__(kBlock)
k_radiance(DevScene sc, RadianceArgs a, const float* __restrict__ rays, const uint32_t* __restrict__ seeds,
           float* __restrict__ rgb, uint32_t* __restrict__ prim, uint32_t* __restrict__ seed_out,
           unsigned long long* __restrict__ counters) {
  extern __shared__ int s_stack[];  // sc.stack entries per lane (stack_lds_bytes)
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= a.n) return;
  int* lds = s_stack + threadIdx.x;
  const Light L{xyz(sc.quads[0]), xyz(sc.quads[1]), xyz(sc.quads[2])};
  uint32_t seed = seeds ? seeds[i] : a.seed0 + i;
  uint32_t first = kNoHit;
  f3 col{0.0f, 0.0f, 0.0f};
  f3 ro{}, rd{}, pc{};
  int depth = 0;
  uint32_t j = 0;  // the sample
  TravStats st{};
  RadCounts c{0u, 0u, 0u};

  while (j < a.samples) {
    if (depth == 0) {
      load_ray(rays, a.n, i, ro, rd);
      pc = f3{1.0f, 1.0f, 1.0f};
    }
    const bool nanray = has_nan(ro) || has_nan(rd);
    if (nanray && !sc.last_sphere_emissive) {
      if (depth == 0 && j == 0u) first = last_prim(sc);
      skip_nan<STATS>(seed, depth, c);  // col += max(NaN, 0) / samples == col + 0
      ++j;
      depth = 0;
      continue;
    }
    Hit h;
    closest_hit<TRIS, false>(sc, ro, rd, lds, h, st);
    if (STATS) {
      ++c.q;
      if (nanray) ++c.nan; else ++c.tr;
    }
    if (depth == 0 && j == 0u) first = h.prim;
    const bool end = shade(sc, L, h, depth, seed, ro, rd, pc);
    ++depth;
    if (end || depth == kRayDepth) {
      add_sample(a, col, pc);
      ++j;
      depth = 0;
    }
  }
  store_ray(rgb, prim, seed_out, a.n, i, col, first, seed);
  if (STATS) flush_counts(counters, c, a.samples);
}

// gate: the launch runs only when *gate == gate_want (a wave-uniform scalar load), else every wave
// returns at once: launch_radiance queues the compact and the 128-B instantiation behind
// k_radiance_bound's answer, which the host never reads (the call returns once queued).
template <bool STATS, int CN, int W>
__global__ void __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(W)))
k_radiance_ps(DevScene sc, RadianceArgs a, const float* __restrict__ rays, const uint32_t* __restrict__ seeds,
              float* __restrict__ rgb, uint32_t* __restrict__ prim, uint32_t* __restrict__ seed_out,
              unsigned long long* __restrict__ counters, uint32_t* __restrict__ queue,
              const uint32_t* __restrict__ gate, uint32_t gate_want) {
  if (gate && *gate != gate_want) return;
  extern __shared__ int s_stack[];  // sc.stack entries per lane, ps_lds
  constexpr PsLds row = ps_lds({true, W, false, 1});
  // 6 waves per SIMD: 3-byte entries (DevScene::ps_waves guarantees the refs fit)
  using STK = typename std::conditional<row.entry == 3, Stack24, Stack32>::type;
  const uint32_t cap = sc.stack;  // the whole stack in LDS: no traversal exceeds the builder's bound
  STK lds;
  if constexpr (row.entry == 3) {
    lds.lo = (uint16_t*)s_stack + threadIdx.x;
    lds.hi = (int8_t*)((uint16_t*)s_stack + cap * (row.hi / 2)) + threadIdx.x;
  } else {
    lds.p = s_stack + threadIdx.x;
  }
  const uint32_t lane = threadIdx.x;
  const Light L{xyz(sc.quads[0]), xyz(sc.quads[1]), xyz(sc.quads[2])};
  const uint32_t n = a.n;
  uint32_t i = 0;  // the lane's ray
  uint32_t seed = 0, first = kNoHit, j = 0;
  f3 col{}, ro{}, rd{}, pc{};
  // the path depth and the pending hit's quad (quad_scan_fast; kNoHit + 1 = 0 for none), one
  // register: depth | (q_prim + 1) << 6, as k_render_ps
  uint32_t dq = 0;
  TravStats st{};
  RadCounts c{0u, 0u, 0u};
  uint32_t done = 0;  // STATS: rays this lane finished
  // invariant: trav == !trav_done(t); a lane starts done
  Trav t;
  t.ref = kNoRef;
  t.lf = t.le = 0u;
  t.sp = 0;
  float q_t = kRayMax;
  bool have = false;       // lane holds a ray
  bool exhausted = false;  // the queue is empty for this lane
  bool trav = false, pending = false, fin = false;
  bool nanray = false;  // the pending hit is a NaN ray's (emissive last sphere), resolved at finalise

  for (;;) {
    // ------------------------------------------------------------ service phase
    for (;;) {
      if (fin) {  // a finished ray: write it (here, outside the sample loop)
        store_ray(rgb, prim, seed_out, n, i, col, first, seed);
        if (STATS) ++done;
        fin = false;
      }
      // refill: lanes without a ray take consecutive indices, one atomic per wave
      const unsigned long long idle = __ballot(!have && !exhausted);
      if (idle != 0ull) {
        const uint32_t n_idle = (uint32_t)__popcll(idle);
        if (n_idle >= a.refill || __ballot(have) == 0ull) {
          const int leader = __ffsll((long long)idle) - 1;
          uint32_t base = 0;
          if ((int)lane == leader) base = atomicAdd(queue, n_idle);
          base = __builtin_amdgcn_readlane(base, leader);  // leader is wave-uniform
          if (!have && !exhausted) {
            const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
            // (the host keeps n + 64 * waves within 32 bits: the counter does not wrap)
            if (slot >= n) {
              exhausted = true;
            } else {
              have = true;
              i = slot;
              seed = seeds ? seeds[slot] : a.seed0 + slot;
              first = kNoHit;
              j = 0u;
              col = f3{0.0f, 0.0f, 0.0f};
              dq = 0u;
            }
          }
        }
      }
      const bool need = have && !trav;
      if (!__any(need)) {
        if (__ballot(!have && !exhausted) != 0ull && __ballot(trav) == 0ull) continue;  // refill again
        break;
      }
      if (need) {
        if (pending) {
          // finalise: rebuild the quad hit, merge triangles, scan spheres, shade
          Hit h;
          if (nanray) {
            nan_hit(sc, ro, rd, h);
            if (STATS) { ++c.q; ++c.nan; }
            nanray = false;
          } else {
            float4 pre[2];
            preload_tshade(sc, t.bi, pre[0], pre[1]);
            quad_rebuild(sc, ro, rd, (dq >> 6) - 1u, q_t, h);
            finish_hit(sc, ro, rd, t.bt, t.bi, h, pre);
            if (STATS) { ++c.q; ++c.tr; }
          }
          if ((dq & 63u) == 0u && j == 0u) first = h.prim;
          const bool end = shade(sc, L, h, (int)(dq & 63u), seed, ro, rd, pc);
          dq = (dq & 63u) + 1u;  // the quad is used: q_prim + 1 = 0
          if (end || dq == (uint32_t)kRayDepth) {
            add_sample(a, col, pc);
            ++j;
            dq = 0u;
          }
          pending = false;
        }
        // start the next ray of this lane's query
        for (;;) {
          if (j >= a.samples) {
            have = false;
            fin = true;
            break;
          }
          if ((dq & 63u) == 0u) {
            load_ray(rays, n, i, ro, rd);  // re-read per sample: not live across the path
            pc = f3{1.0f, 1.0f, 1.0f};
          }
          if (has_nan(ro) || has_nan(rd)) {
            if (!sc.last_sphere_emissive) {
              if ((dq & 63u) == 0u && j == 0u) first = last_prim(sc);
              skip_nan<STATS>(seed, (int)(dq & 63u), c);
              ++j;
              dq = 0u;
              continue;
            }
            // emissive last sphere: the NaN ray's hit is resolved and shaded at the next finalise
            nanray = true;
            pending = true;
            break;
          }
          uint32_t q_prim;
          quad_scan_fast(sc, ro, rd, q_prim, q_t);
          trav_init<CN>(sc, ro, rd, q_prim != kNoHit, q_t, t);
          dq = (dq & 63u) | (q_prim + 1u) << 6;
          // the root node is tested here: rays that miss every root child never enter the traversal phase
          node_step<STATS, CN, STK, true>(sc, t, lds, st);
          if (trav_done(t)) pending = true;
          else trav = true;
          break;
        }
      }
      if ((uint32_t)__popcll(__ballot(trav)) >= a.to_trav) break;
    }
    if (__ballot(have || !exhausted) == 0ull) break;
    // --------------------------------------------------------- traversal phase
    uint32_t to_service = a.to_service;
    if (a.svc_frac) {
      const uint32_t live = (uint32_t)__popcll(__ballot(have));
      const uint32_t sparse = (live * a.svc_frac) >> 6;
      to_service = sparse < to_service ? sparse : to_service;
    }
    // 1/d and the slab offsets are recomputed here from the ray (trav_init's operations:
    // bit-identical), so that they are dead through the service phase (k_render_ps)
    {
      const f3 inv = f3{safe_inv_short(rd.x), safe_inv_short(rd.y), safe_inv_short(rd.z)};
      t.ot = slab_offset(ro, inv);
      t.inv = CN ? sc.cstep * inv : inv;
    }
    for (;;) {
      // one uniform mode per step: triangle steps once enough lanes hold a pending leaf, else node steps
      const bool can_node = t.ref != kNoRef;  // implies trav (invariant above)
      const bool can_tri = t.lf < t.le;       // implies trav
      const uint32_t nn = (uint32_t)__popcll(__ballot(can_node));
      const uint32_t nl = (uint32_t)__popcll(__ballot(can_tri));
      const bool tri_mode = nn == 0 || nl * 100u >= nn * a.tri_ratio;
      if (tri_mode) {
        if (can_tri) tri_step<STATS, CN>(sc, ro, rd, t, lds, st);
      } else {
        if (can_node) node_step<STATS, CN>(sc, t, lds, st);
      }
      if (trav && trav_done(t)) {
        trav = false;
        pending = true;
      }
      const uint32_t ntrav = (uint32_t)__popcll(__ballot(trav));
      if (ntrav == 0) break;
      if (ntrav <= to_service && __any(!trav && (have || !exhausted))) break;
    }
  }
  if (STATS) flush_counts(counters, c, (unsigned long long)done * a.samples);
}

// *flag = 1 when a ray's origin lies beyond the compact codes' bound (DevScene::cbound): its
// depth-0 traversal then needs the 128-B nodes (hit points, the later origins, are always within).
// A NaN origin compares false: such a ray does not traverse.
__global__ void __launch_bounds__(256)
k_radiance_bound(const float* __restrict__ rays, uint32_t n, float bound, uint32_t* __restrict__ flag) {
  bool out = false;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    out = out || fabsf(rays[i]) > bound || fabsf(rays[(size_t)n + i]) > bound || fabsf(rays[2 * (size_t)n + i]) > bound;
  if (out) *flag = 1u;  // every writer stores the same word
}

using PsKernel = void (*)(DevScene, RadianceArgs, const float*, const uint32_t*, float*, uint32_t*, uint32_t*,
                          unsigned long long*, uint32_t*, const uint32_t*, uint32_t);
template <bool STATS>
PsKernel ps_kernel(uint32_t waves, int cn) {
  static constexpr PsKernel k[2][2] = {{k_radiance_ps<STATS, 0, 5>, k_radiance_ps<STATS, 1, 5>},
                                       {k_radiance_ps<STATS, 0, 6>, k_radiance_ps<STATS, 1, 6>}};
  return k[waves == 6][cn != 0];
}

}  // namespace

hipError_t radiance_resident_waves(const DevScene& sc, int device, uint32_t& waves) {
  const PsForm form{true, sc.ps_waves, false, sc.stack};
  int per_cu = 1 << 30, cus = 0;
  for (int cn = 0; cn < 2; ++cn) {
    int n = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(
        &n, reinterpret_cast<const void*>(ps_kernel<false>(form.waves, cn)), kBlock, ps_lds(form).total);
    if (e != hipSuccess) return e;
    per_cu = n < per_cu ? n : per_cu;
  }
  const hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  if (e != hipSuccess) return e;
  waves = (uint32_t)((per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 1));
  return hipSuccess;
}

hipError_t launch_radiance(const DevScene& sc, const RadianceArgs& a, const float* d_rays, const uint32_t* d_seeds,
                           const wgt_radiance_buffers& out, unsigned long long* d_counts, uint32_t resident,
                           uint32_t* d_ws, hipStream_t stream) {
  if (a.n == 0) return hipSuccess;
  const dim3 block(kBlock);
  if (!a.persistent) {
    const dim3 grid((a.n - 1u) / kBlock + 1u);  // n > 0; no 32-bit overflow at any n
    using Kernel = void (*)(DevScene, RadianceArgs, const float*, const uint32_t*, float*, uint32_t*, uint32_t*,
                            unsigned long long*);
    static constexpr Kernel k[2][2] = {{k_radiance<false, false>, k_radiance<false, true>},
                                       {k_radiance<true, false>, k_radiance<true, true>}};
    k[sc.n_tris > 0][d_counts != nullptr]<<<grid, block, stack_lds_bytes(sc.stack), stream>>>(
        sc, a, d_rays, d_seeds, out.rgb, out.prim, out.seed_out, d_counts);
    return hipGetLastError();
  }
  // the persistent form: d_ws[0] the ray queue's counter, d_ws[1] k_radiance_bound's flag
  if (sc.n_tris == 0 || resident == 0 || !d_ws) return hipErrorInvalidValue;
  const PsForm form{true, sc.ps_waves, false, sc.stack};
  const size_t lds = ps_lds(form).total;
  const uint32_t waves = (a.n - 1u) / kBlock + 1u;  // n > 0; no 32-bit overflow at any n
  const dim3 grid(waves < resident ? waves : resident);
  hipError_t e = hipMemsetAsync(d_ws, 0, 8, stream);
  if (e != hipSuccess) return e;
  const auto run = [&](int cn, const uint32_t* gate, uint32_t want) {
    (d_counts ? ps_kernel<true>(form.waves, cn) : ps_kernel<false>(form.waves, cn))<<<grid, block, lds, stream>>>(
        sc, a, d_rays, d_seeds, out.rgb, out.prim, out.seed_out, d_counts, d_ws, gate, want);
    return hipGetLastError();
  };
  if (!a.compact) return run(0, nullptr, 0u);
  const uint32_t nb = (a.n - 1u) / 256u + 1u;
  k_radiance_bound<<<nb < 1024u ? nb : 1024u, 256, 0, stream>>>(d_rays, a.n, sc.cbound, d_ws + 1);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if ((e = run(1, d_ws + 1, 0u)) != hipSuccess) return e;
  return run(0, d_ws + 1, 1u);
}

}  // namespace wgt
