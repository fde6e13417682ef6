// wgt_runtime.cpp — the C-ABI (include/wgt_api.h) over HIP: device context and
// stream (replacing Renderer::InitDevice, render.cpp:49-147), scene upload with
// BVH build (replacing Scene::InitBuffers, scene.cpp:161-165), the render launch
// (replacing the compute pass of Renderer::OnRender, render.cpp:461-491) and the
// readback (replacing saveTexture's copyTextureToBuffer + mapAsync,
// save_texture.h:10-87).  What the calls decide without the device is host/launch_plan.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/wgt_api.h"
#include "host/launch_plan.h"
#include "wgt_compact.h"
#include "wgt_error.h"
#include "wgt_internal.h"

using namespace wgt;

namespace {
thread_local std::string g_err;

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};
}  // namespace

namespace wgt {
void set_thread_error(const std::string& msg) { g_err = msg; }
}  // namespace wgt

struct wgt_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  bool has_scene = false;
  DevScene sc{};
  void* scene_mem = nullptr;
  wgt_scene_info info{};
  uint32_t ps_resident = 0;
  uint32_t rad_resident = 0;  // radiance_resident_waves of the scene, asked at its first radiance query (0: not yet)
  // wgt_update_triangles: the extent of the scene's lights, quads and spheres (they do not move), and
  // what the first refit of a scene prepares (an upload's cost and layout do not change): the level
  // lists of the tree (refit_levels) on the device, then one word for the step exponent
  double fixed_extent = 0.0;
  std::vector<uint32_t> level_begin;
  DevBuf level_order;
  float refit_host_ms = 0.0f, refit_device_ms = 0.0f;  // of the last update or rebuild (wgt_update_timing)
  // wgt_rebuild_triangles: a rebuilt tree lives in an allocation of its own, tree[tree_cur] (-1: the
  // upload's tree, in scene_mem); the other one is the spare the next rebuild builds into, so a steady
  // stream of rebuilds allocates nothing.  fixed_bytes: the scene's lights, quads and spheres, padded
  DevBuf tree[2];
  int tree_cur = -1;
  size_t fixed_bytes = 0;
  // wgt_motion_snapshot: n_tris x 48 B (v0, e1, e2, face normal by original index), then n_tris leaf
  // slots; allocated by the first snapshot after an upload, dropped by the next upload
  DevBuf motion;
  bool has_snapshot = false;
  // the sampled kernels' table of each side's constants (sample_constants), uploaded with the context
  DevBuf sample_tab;
  // scratch for the synchronous entry points: the renders' tile list, outputs and counters; the
  // queries' rays, prim and dist (closest hits and hit records alike); the occlusion queries'
  // limits and answers; the hit records' pos | norm | col (9 planes) and flags; the G-buffer's rays;
  // a refit's moved triangles; the device check's result (RefitCheck); a reproject's pos_prev | norm_prev;
  // a sampled call's sample map; a rebuild's keys, lists and sort storage (RebuildScratch); a radiance
  // query's seeds and final seeds (its colours use kHitVec), and the persistent radiance kernel's two
  // scheduling words (every launch of the context uses them, in launch_on's order); a multi-hit query's
  // counts (kOut32) and its k planes of prim and dist (kPrim, kDist)
  enum Scratch { kTiles, kOut8, kOut32, kHit, kCounters, kRays, kPrim, kDist, kOccLimit, kOccOut, kHitVec,
                 kHitFlags, kGbRays, kMoved, kCheck, kMotionOut, kSampleMap, kRebuild, kRadSeeds, kRadSeedOut, kRadWs,
                 kScratchBufs };
  DevBuf buf[kScratchBufs];
  // Scheduling workspaces of the persistent kernel (queues, LPT costs and order),
  // used round-robin by its launches.  A launch waits (on the device) only for the
  // previous launch that used the same slot, so consecutive frames issued on two
  // streams overlap: the next frame's pre-pass and first waves fill the CUs that the
  // previous frame's end-of-launch drain leaves idle.
  static constexpr int kMaxWsSlots = 4;
  struct WsSlot {
    DevBuf ws;
    hipEvent_t ev = nullptr;  // recorded after the slot's last launch
    uint32_t clean_nb = 0;    // launch_render: the block count its last LPT launch left zero
  };
  WsSlot slots[kMaxWsSlots];
  uint32_t next_slot = 0;
  // wgt_pipeline_stream: streams for frames issued round-robin, each created with a
  // full CU mask, which gives it a hardware queue of its own (two plain streams may
  // share one, and launches on one hardware queue never overlap)
  hipStream_t pipe[kMaxWsSlots] = {};
  // The pixel queue's order per view (launch_plan.h OrderPlanner): the plan of
  // each launch, the kOrderBufs shared orders of order_cap words each in one allocation, and per
  // buffer the event recorded right after the sort that wrote it
  static_assert(kMaxWsSlots == OrderPlanner::kSlots, "the planner tracks readers by workspace slot");
  OrderPlanner order;
  DevBuf order_mem;
  uint32_t order_cap = 0;
  hipEvent_t order_ev[kOrderBufs] = {};
  // recorded after every other launch that reads the scene (trace queries); each such
  // launch first waits for the previous one.  The scene
  // and the workspaces are freed (re-upload, destroy, regrow) only after this event
  // and every slot's event have completed
  hipEvent_t use_ev = nullptr;
  std::vector<hipEvent_t> evpool;  // per-launch timing (profile runs only)
};

namespace {

int fail(wgt_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  g_err = msg;
  return code;
}

#define WGT_HIP(ctx, expr)                                                                    \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return fail((ctx), WGT_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));       \
  } while (0)

// Run `launch` (-> hipError_t) on stream s after every earlier such launch of the context (any
// stream), and record it in use_ev: every launch that reads the scene other than launch_render
// (which orders itself by workspace slot, render_frame).
template <class Launch>
int launch_on(wgt_ctx* ctx, hipStream_t s, const char* name, Launch&& launch) {
  if (!ctx->use_ev) WGT_HIP(ctx, hipEventCreateWithFlags(&ctx->use_ev, hipEventDisableTiming));
  else WGT_HIP(ctx, hipStreamWaitEvent(s, ctx->use_ev, 0));
  const hipError_t e = launch();
  if (e != hipSuccess) return fail(ctx, WGT_E_HIP, std::string(name) + ": " + hipGetErrorString(e));
  WGT_HIP(ctx, hipEventRecord(ctx->use_ev, s));
  return WGT_OK;
}
// Host wait for every launch of the context (before freeing what they read).
int use_drain(wgt_ctx* ctx) {
  if (ctx->use_ev) WGT_HIP(ctx, hipEventSynchronize(ctx->use_ev));
  for (auto& sl : ctx->slots)
    if (sl.ev) WGT_HIP(ctx, hipEventSynchronize(sl.ev));
  WGT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return WGT_OK;
}

void free_buf(DevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
}
int ensure(wgt_ctx* ctx, DevBuf& b, size_t bytes) {
  if (b.bytes >= bytes) return WGT_OK;
  if (b.p) {
    // launches on any stream may still use the old buffer: it is freed only once they have ended
    if (int rc = use_drain(ctx)) return rc;
    free_buf(b);
  }
  size_t want = std::max<size_t>(bytes, 256);
  WGT_HIP(ctx, hipMalloc(&b.p, want));
  b.bytes = want;
  return WGT_OK;
}
// The context's scratch buffer `which`, grown to `bytes`, in p.
template <class T>
int scratch(wgt_ctx* ctx, wgt_ctx::Scratch which, size_t bytes, T*& p) {
  const int rc = ensure(ctx, ctx->buf[which], bytes);
  p = (T*)ctx->buf[which].p;
  return rc;
}
// ... filled with `bytes` of host data, on the context's stream
template <class T>
int stage(wgt_ctx* ctx, wgt_ctx::Scratch which, const void* src, size_t bytes, const T*& p) {
  T* d;
  if (int rc = scratch(ctx, which, bytes, d)) return rc;
  WGT_HIP(ctx, hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  p = d;
  return WGT_OK;
}
int fetch(wgt_ctx* ctx, void* dst, const void* d_src, size_t bytes) {
  WGT_HIP(ctx, hipMemcpyAsync(dst, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  return WGT_OK;
}
int sync_stream(wgt_ctx* ctx) {
  WGT_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return WGT_OK;
}
hipStream_t stream_or_own(wgt_ctx* ctx, void* stream) { return stream ? (hipStream_t)stream : ctx->stream; }

// The synchronous image passes: one allocation of the call's own, laid out by `lay` (launch_plan.h
// StageLayout); its sources uploaded on the context's stream, then `pass(at)` (the asynchronous form on
// the parts, at(k) the device address of part k or null), then its destinations fetched.  The stream is
// drained before the allocation is freed, whatever was queued; the first error is the call's.
template <class Pass>
int run_staged(wgt_ctx* ctx, const StageLayout& lay, Pass&& pass) {
  char* base = nullptr;
  if (hipMalloc((void**)&base, lay.bytes()) != hipSuccess) {
    (void)hipGetLastError();
    return fail(ctx, WGT_E_NOMEM, "device allocation of " + std::to_string(lay.bytes()) + " bytes failed");
  }
  int rc = WGT_OK;
  for (int k = 0; k < lay.n && rc == WGT_OK; ++k) {
    const StagePart& p = lay.part[k];
    if (p.src && hipMemcpyAsync(lay.at(base, k), p.src, p.bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
      rc = fail(ctx, WGT_E_HIP, std::string("hipMemcpyAsync of ") + lay.what + " input failed");
  }
  if (rc == WGT_OK) rc = pass([&](int k) { return lay.at(base, k); });
  for (int k = 0; k < lay.n && rc == WGT_OK; ++k)
    if (lay.part[k].dst) rc = fetch(ctx, lay.part[k].dst, lay.at(base, k), lay.part[k].bytes);
  const int rs = sync_stream(ctx);
  (void)hipFree(base);
  return rc != WGT_OK ? rc : rs;
}

int check_render_args(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H, uint32_t tw, uint32_t th) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (!cam) return fail(ctx, WGT_E_INVALID, "null camera");
  if (!ctx->has_scene) return fail(ctx, WGT_E_NOSCENE, "no scene uploaded");
  const std::string bad = check_frame_args(*cam, W, H, tw, th);
  return bad.empty() ? WGT_OK : fail(ctx, WGT_E_INVALID, bad);
}

// The common preambles, in the calls' order of checks; kNothingToDo: the call returns WGT_OK at once
// (WGT_BEGIN).  `bad`: the refusal of the call's own argument check, or null when fine.
constexpr int kNothingToDo = 1;
#define WGT_BEGIN(preamble)                                                     \
  do {                                                                          \
    if (int rc_ = (preamble)) return rc_ == kNothingToDo ? (int)WGT_OK : rc_;   \
  } while (0)
// The ray queries': context, scene, n == 0, the call's own check, device.
int query_begin(wgt_ctx* ctx, uint32_t n, const char* bad) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (!ctx->has_scene) return fail(ctx, WGT_E_NOSCENE, "no scene uploaded");
  if (n == 0) return kNothingToDo;
  if (bad) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  return WGT_OK;
}
// The tile-list calls': check_render_args, the stats to clear (when the call has_stats), an empty
// list, a null one, the call's own check, device.
int tiles_begin(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H, uint32_t tw, uint32_t th,
                const wgt_tile* d_tiles, uint32_t n_tiles, bool has_stats, wgt_stats* stats, const char* bad) {
  if (int rc = check_render_args(ctx, cam, W, H, tw, th)) return rc;
  if (has_stats && !stats) return fail(ctx, WGT_E_INVALID, "null stats");
  if (has_stats) std::memset(stats, 0, sizeof *stats);
  if (n_tiles == 0) return kNothingToDo;
  if (!d_tiles) return fail(ctx, WGT_E_INVALID, "null tile list");
  if (bad) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  return WGT_OK;
}
const char* null_buffer(bool any) { return any ? "null buffer" : nullptr; }
const char* bad_hits(const wgt_hit_buffers* b) {
  if (!b) return "null buffer";
  return !b->prim && !b->dist && !b->pos && !b->norm && !b->col && !b->flags ? "no hit field asked for" : nullptr;
}

// wgt_scene_info::node_form: the persistent kernel's node form for the reference camera.
uint32_t reference_node_form(const DevScene& sc) {
  const wgt_camera_param cam{{278.0f, 278.0f, -800.0f}, 0.0f, {278.0f, 278.0f, 0.0f}, 0.0f, 1.0f, 40.0f, 1u, 0u};
  return sc.n_tris ? (uint32_t)node_form(sc, make_frame(cam, 1, 1)) : 0u;
}

// The wgt_stats field of each device counter, in the order of CNT_* (wgt_internal.h)
constexpr uint64_t wgt_stats::*kStatOf[] = {
    &wgt_stats::queries, &wgt_stats::traced_rays, &wgt_stats::samples, &wgt_stats::nan_rays,
    &wgt_stats::node_visits, &wgt_stats::tri_tests, &wgt_stats::pixels, &wgt_stats::loop_wave_iters,
    &wgt_stats::loop_lane_iters, &wgt_stats::trav_wave_steps, &wgt_stats::trav_lane_steps, &wgt_stats::cyc_service,
    &wgt_stats::cyc_trav, &wgt_stats::cyc_refill, &wgt_stats::cyc_finalise, &wgt_stats::cyc_shade,
    &wgt_stats::cyc_camera, &wgt_stats::cyc_quads, &wgt_stats::cyc_root, &wgt_stats::stack_spills,
    &wgt_stats::stack_refills, &wgt_stats::stack_overflows, &wgt_stats::top_node_visits, &wgt_stats::cyc_node_steps,
    &wgt_stats::cyc_top_steps, &wgt_stats::cyc_tri_steps, &wgt_stats::quad_ref_scans};
static_assert(sizeof kStatOf / sizeof *kStatOf == CNT_QUAD_REF + 1, "one field per counter");
void fill_stats(const unsigned long long* c, wgt_stats* s) {
  for (int i = 0; i <= CNT_QUAD_REF; ++i) s->*kStatOf[i] = c[i];
}
// The time of one frame's launch (profile runs only).
void fill_timing(float ms, wgt_stats* s) {
  s->kernel_ms = s->trace_ms = ms;
  s->iterations = 1;
}
// The stats of a synchronous render (wgt_render_frames, wgt_render_tile): the counters of a
// second, instrumented pass over the context's tile list, and the time of the render itself
int stats_of_render(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H, uint32_t tw, uint32_t th,
                    uint32_t n_tiles, float ms, wgt_stats* stats) {
  const int rc = wgt_render_tiles_stats(ctx, cam, W, H, tw, th, (const wgt_tile*)ctx->buf[wgt_ctx::kTiles].p,
                                        n_tiles, stats);
  if (rc == WGT_OK) fill_timing(ms, stats);
  return rc;
}

hipEvent_t pool_event(wgt_ctx* ctx, size_t i) {
  while (ctx->evpool.size() <= i) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    ctx->evpool.push_back(e);
  }
  return ctx->evpool[i];
}

// The identity of a launch's tile list for the order's view key: the hash of a host list's origins
// (the synchronous entry points, which stage it), or a device list's address.
struct TilesId {
  uint64_t id;
  bool by_ptr;
};
TilesId tiles_at(const wgt_tile* d_tiles) { return TilesId{(uint64_t)(uintptr_t)d_tiles, true}; }
TilesId tiles_of(const wgt_tile* host_tiles, uint32_t n) { return TilesId{order_tiles_hash(host_tiles, n), false}; }

// The shared order buffers hold `nb` words each: regrown (both, after every launch of the context
// has ended) when a launch that is to write one has more blocks than any such launch before it.
int ensure_order(wgt_ctx* ctx, uint32_t nb) {
  if (ctx->order_cap >= nb) return WGT_OK;
  if (int rc = use_drain(ctx)) return rc;
  free_buf(ctx->order_mem);
  ctx->order_cap = 0;
  ctx->order.buffers_reset();
  const uint32_t cap = (nb + 63u) & ~63u;  // each buffer 256-B aligned
  WGT_HIP(ctx, hipMalloc(&ctx->order_mem.p, (size_t)kOrderBufs * cap * 4));
  ctx->order_mem.bytes = (size_t)kOrderBufs * cap * 4;
  ctx->order_cap = cap;
  for (hipEvent_t& e : ctx->order_ev)
    if (!e) WGT_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return WGT_OK;
}
uint32_t* order_buf(const wgt_ctx* ctx, int b) { return (uint32_t*)ctx->order_mem.p + (size_t)b * ctx->order_cap; }

// Render the tile list: one launch of the persistent kernel (or, WGT_KERNEL=1, of the
// simple one), asynchronous on stream s unless timed (ms: the launch's time, waited for).
// sm: a sampled frame's map and table (sample_args), SampleArgs{} for a plain one.
// tid: the tile list's identity (the queue order is planned per view, OrderPlanner).
int render_frame(wgt_ctx* ctx, const DevFrame& fr, const SampleArgs& sm, const wgt_tile* d_tiles, TilesId tid, uchar4* out8,
                 float4* out32, uint32_t* outhit, unsigned long long* counters, hipStream_t s, float* ms) {
  const uint64_t n64 = (uint64_t)fr.tw * fr.th * fr.n_tiles;
  if (n64 == 0) return WGT_OK;
  // 32-bit pixel offsets in the kernels (slot_setup)
  if (n64 > 0x7fffffffull) return fail(ctx, WGT_E_INVALID, "too many pixels in one launch");
  hipEvent_t e0 = ms ? pool_event(ctx, 0) : nullptr, e1 = ms ? pool_event(ctx, 1) : nullptr;
  if (ms && (!e0 || !e1)) return fail(ctx, WGT_E_HIP, "hipEventCreate failed");
  if (ms) WGT_HIP(ctx, hipEventRecord(e0, s));
  int rc;
  // the next workspace slot: a launch on any stream first waits for the previous
  // launch that used it (WGT_WS_SLOTS = 1 serialises every launch of the context; 4 by
  // default, one per pipeline stream, so that up to 4 frames are in flight: a strongly scaled
  // rank's share of a frame holds fewer pixels than the device has lanes)
  const uint32_t n_slots = std::min<uint32_t>(std::max<uint32_t>(env_u32("WGT_WS_SLOTS", wgt_ctx::kMaxWsSlots), 1u),
                                              (uint32_t)wgt_ctx::kMaxWsSlots);
  const int slot = (int)(ctx->next_slot % n_slots);
  wgt_ctx::WsSlot& sl = ctx->slots[slot];
  ctx->next_slot = (ctx->next_slot + 1) % n_slots;
  const size_t ws_need = render_ws_bytes(ctx->sc, fr, ctx->ps_resident);
  if (sl.ws.bytes < ws_need && (rc = use_drain(ctx))) return rc;  // before regrowing
  const void* old_ws = sl.ws.p;
  const size_t old_bytes = sl.ws.bytes;
  if ((rc = ensure(ctx, sl.ws, ws_need))) return rc;
  // a new workspace (ensure reallocated: its size changed, whatever address hipMalloc returned):
  // nothing is known zero
  if (sl.ws.p != old_ws || sl.ws.bytes != old_bytes) sl.clean_nb = 0;
  if (!sl.ev) WGT_HIP(ctx, hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
  else WGT_HIP(ctx, hipStreamWaitEvent(s, sl.ev, 0));
  // the queue order: this launch's own (TODAY), or its view's shared one, which it writes (REFINE) or
  // only reads (REUSE).  A shared buffer is rewritten only when the launches that read it have ended:
  // they are the last launches of their slots or earlier ones, so the slots' events tell (never a wait)
  const OrderKnobs knobs = order_knobs();
  const uint32_t nb = order_blocks(fr);
  const bool eligible = order_eligible(fr, knobs, sm.map != nullptr, nb);
  const OrderKey key = order_key(fr, nb, knobs, ctx->order.epoch(), tid.id, tid.by_ptr);
  // room in the shared buffers only for the launch that would write one: a first sighting and a launch
  // on its own allocate nothing, and a reusing launch's buffer holds its nb already
  if (ctx->order.refine_due(key, eligible) && (rc = ensure_order(ctx, nb))) return rc;
  const OrderPlan op = ctx->order.plan(key, eligible, slot, [&](int i) {
    if (!ctx->slots[i].ev) return true;
    const hipError_t q = hipEventQuery(ctx->slots[i].ev);
    // "not ready" is the answer, not a failure of this launch: it is not left behind as the last error
    if (q != hipSuccess) (void)hipGetLastError();
    return q == hipSuccess;
  });
  OrderArgs oa;
  oa.side = op.side;
  if (op.mode != kOrderToday) oa.shared = order_buf(ctx, op.buf);
  if (op.mode == kOrderRefine) oa.sorted = ctx->order_ev[op.buf];
  if (op.mode == kOrderReuse) {
    oa.prepass = false;
    // the sort that wrote the order ended a few ms into its own launch: no wait for a main kernel
    WGT_HIP(ctx, hipStreamWaitEvent(s, ctx->order_ev[op.buf], 0));
  }
  {
    const hipError_t e = launch_render(ctx->sc, fr, sm, d_tiles, out8, out32, outhit, counters, ctx->ps_resident,
                                       sl.ws.p, sl.ws.bytes, s, sl.clean_nb, oa);
    if (e != hipSuccess) {
      ctx->order.launch_failed(op);
      sl.clean_nb = 0;
      // part of the launch may be queued (a pre-pass and a sort into a shared buffer): the slot's event
      // covers it, so that the planner's reader of this slot is not taken for ended too early
      (void)hipEventRecord(sl.ev, s);
      return fail(ctx, WGT_E_HIP, std::string("launch_render: ") + hipGetErrorString(e));
    }
  }
  WGT_HIP(ctx, hipEventRecord(sl.ev, s));
  if (ms) {
    WGT_HIP(ctx, hipEventRecord(e1, s));
    WGT_HIP(ctx, hipEventSynchronize(e1));
    WGT_HIP(ctx, hipEventElapsedTime(ms, e0, e1));
  }
  return WGT_OK;
}

// The counting pass of a launch (the instrumented kernels) over the tile list d_tiles, read back.
int count_frame(wgt_ctx* ctx, const DevFrame& fr, const SampleArgs& sm, const wgt_tile* d_tiles, TilesId tid, wgt_stats* stats) {
  int rc;
  unsigned long long c[CNT_N], *d_c;
  if ((rc = scratch(ctx, wgt_ctx::kCounters, sizeof c, d_c))) return rc;
  WGT_HIP(ctx, hipMemsetAsync(d_c, 0, sizeof c, ctx->stream));
  if ((rc = render_frame(ctx, fr, sm, d_tiles, tid, nullptr, nullptr, nullptr, d_c, ctx->stream, nullptr))) return rc;
  if ((rc = fetch(ctx, c, d_c, sizeof c)) || (rc = sync_stream(ctx))) return rc;
  fill_stats(c, stats);
  return WGT_OK;
}

// The queries' launches on stream s; the asynchronous entry points are these behind their checks,
// the synchronous ones stage their inputs, call the same, fetch and synchronise.
int occluded_launch(wgt_ctx* ctx, const float* d_rays, const float* d_max_dist, uint32_t n, uint8_t* d_out,
                    hipStream_t s) {
  return launch_on(ctx, s, "launch_occluded", [&] { return launch_occluded(ctx->sc, d_rays, d_max_dist, n, d_out, s); });
}
int hits_launch(wgt_ctx* ctx, const float* d_rays, uint32_t n, const wgt_hit_buffers& dev, hipStream_t s) {
  return launch_on(ctx, s, "launch_trace_hits", [&] { return launch_trace_hits(ctx->sc, d_rays, n, dev, s); });
}
int nearest_launch(wgt_ctx* ctx, const float* d_points, const float* d_max_dist, uint32_t n,
                   const wgt_nearest_buffers& dev, unsigned long long* d_counts, hipStream_t s) {
  return launch_on(ctx, s, "launch_nearest",
                   [&] { return launch_nearest(ctx->sc, d_points, d_max_dist, n, dev, d_counts, s); });
}
// The radiance query (behind its checks): the plan (plan_radiance), then one launch of the planned form.
int radiance_launch(wgt_ctx* ctx, const float* d_rays, const uint32_t* d_seeds, uint32_t seed0, uint32_t samples,
                    uint32_t n, const wgt_radiance_buffers& dev, unsigned long long* d_counts, hipStream_t s) {
  if (ctx->sc.n_tris > 0 && ctx->rad_resident == 0)
    WGT_HIP(ctx, radiance_resident_waves(ctx->sc, ctx->device, ctx->rad_resident));
  RadianceArgs a;
  const std::string bad = plan_radiance(ctx->sc, seed0, samples, n, ctx->rad_resident, a);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  uint32_t* d_ws = nullptr;
  int rc;
  if (a.persistent && (rc = scratch(ctx, wgt_ctx::kRadWs, 8, d_ws))) return rc;
  return launch_on(ctx, s, "launch_radiance", [&] {
    return launch_radiance(ctx->sc, a, d_rays, d_seeds, dev, d_counts, ctx->rad_resident, d_ws, s);
  });
}
// The multi-hit query (behind its checks): the plan (plan_multi_hit), then one launch of the planned form.
int multi_hit_launch(wgt_ctx* ctx, const float* d_rays, const float* d_max_dist, uint32_t n, uint32_t k,
                     uint32_t flags, const wgt_multi_hit_buffers& dev, unsigned long long* d_counts, hipStream_t s) {
  MultiHitPlan p;
  const std::string bad = plan_multi_hit(ctx->sc, dev, n, k, flags, p);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  return launch_on(ctx, s, "launch_multi_hit",
                   [&] { return launch_multi_hit(ctx->sc, p, d_rays, d_max_dist, dev, d_counts, s); });
}
// The k-nearest query (behind its checks): the plan (plan_nearest_k), then one launch of the planned form.
int nearest_k_launch(wgt_ctx* ctx, const float* d_points, const float* d_max_dist, uint32_t n, uint32_t k,
                     const wgt_nearest_k_buffers& dev, unsigned long long* d_counts, hipStream_t s) {
  NearestKPlan p;
  const std::string bad = plan_nearest_k(ctx->sc, dev, n, k, p);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  return launch_on(ctx, s, "launch_nearest_k",
                   [&] { return launch_nearest_k(ctx->sc, p, d_points, d_max_dist, dev, d_counts, s); });
}
// The overlap query (behind its checks): the plan (plan_overlap), then one launch of the planned form.
int overlap_launch(wgt_ctx* ctx, const float* d_tris, uint32_t n, uint32_t k, const wgt_overlap_buffers& dev,
                   unsigned long long* d_counts, hipStream_t s) {
  OverlapPlan p;
  const std::string bad = plan_overlap(ctx->sc, d_tris, &dev, n, k, p);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  return launch_on(ctx, s, "launch_overlap", [&] { return launch_overlap(ctx->sc, p, d_tris, dev, d_counts, s); });
}
// The self-intersection query (behind its checks): the plan (plan_overlap_self), then one launch of the planned form.
int overlap_self_launch(wgt_ctx* ctx, const uint32_t* d_indices, uint32_t k, const wgt_overlap_buffers& dev,
                        unsigned long long* d_counts, hipStream_t s) {
  OverlapSelfPlan p;
  const std::string bad = plan_overlap_self(ctx->sc, &dev, k, p);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  return launch_on(ctx, s, "launch_overlap_self",
                   [&] { return launch_overlap_self(ctx->sc, p, d_indices, dev, d_counts, s); });
}
// The self-intersection calls' preamble: query_begin with the scene's triangle count as n, so a scene without
// triangles is answered as the overlap query answers n == 0.
int overlap_self_begin(wgt_ctx* ctx, const char* bad) {
  return query_begin(ctx, ctx && ctx->has_scene ? ctx->sc.n_tris : 1u, bad);
}
// The G-buffer launch of a tile list (behind check_render_args, the render calls' preamble).
int gbuffer_launch(wgt_ctx* ctx, const DevFrame& fr, const SampleArgs& sm, const wgt_tile* d_tiles,
                   const wgt_hit_buffers& dev, float* d_rays, hipStream_t s) {
  // 32-bit pixel offsets in the kernels (slot_setup), as render_frame
  if ((uint64_t)fr.tw * fr.th * fr.n_tiles > 0x7fffffffull)
    return fail(ctx, WGT_E_INVALID, "too many pixels in one launch");
  return launch_on(ctx, s, "launch_gbuffer", [&] { return launch_gbuffer(ctx->sc, fr, sm, d_tiles, dev, d_rays, s); });
}

// Device staging of n hit records for the fields `out` asks for (the synchronous forms).
int stage_hits(wgt_ctx* ctx, const wgt_hit_buffers& out, size_t n, wgt_hit_buffers& dev) {
  dev = wgt_hit_buffers{};
  int rc;
  if (out.prim && (rc = scratch(ctx, wgt_ctx::kPrim, n * 4, dev.prim))) return rc;
  if (out.dist && (rc = scratch(ctx, wgt_ctx::kDist, n * 4, dev.dist))) return rc;
  if (out.pos || out.norm || out.col) {
    float* v;
    if ((rc = scratch(ctx, wgt_ctx::kHitVec, n * 36, v))) return rc;
    if (out.pos) dev.pos = v;
    if (out.norm) dev.norm = v + 3 * n;
    if (out.col) dev.col = v + 6 * n;
  }
  if (out.flags && (rc = scratch(ctx, wgt_ctx::kHitFlags, n, dev.flags))) return rc;
  return WGT_OK;
}
// Defined contents for records no kernel writes (a tile reaching past the frame): prim = miss, zeros
int clear_hits(wgt_ctx* ctx, const wgt_hit_buffers& dev, size_t n) {
  if (dev.prim) WGT_HIP(ctx, hipMemsetAsync(dev.prim, 0xff, n * 4, ctx->stream));
  if (dev.dist) WGT_HIP(ctx, hipMemsetAsync(dev.dist, 0, n * 4, ctx->stream));
  if (dev.pos) WGT_HIP(ctx, hipMemsetAsync(dev.pos, 0, n * 12, ctx->stream));
  if (dev.norm) WGT_HIP(ctx, hipMemsetAsync(dev.norm, 0, n * 12, ctx->stream));
  if (dev.col) WGT_HIP(ctx, hipMemsetAsync(dev.col, 0, n * 12, ctx->stream));
  if (dev.flags) WGT_HIP(ctx, hipMemsetAsync(dev.flags, 0, n, ctx->stream));
  return WGT_OK;
}
// Copy back only the fields asked for.
int fetch_hits(wgt_ctx* ctx, const wgt_hit_buffers& out, const wgt_hit_buffers& dev, size_t n) {
  int rc;
  if (out.prim && (rc = fetch(ctx, out.prim, dev.prim, n * 4))) return rc;
  if (out.dist && (rc = fetch(ctx, out.dist, dev.dist, n * 4))) return rc;
  if (out.pos && (rc = fetch(ctx, out.pos, dev.pos, n * 12))) return rc;
  if (out.norm && (rc = fetch(ctx, out.norm, dev.norm, n * 12))) return rc;
  if (out.col && (rc = fetch(ctx, out.col, dev.col, n * 12))) return rc;
  if (out.flags && (rc = fetch(ctx, out.flags, dev.flags, n))) return rc;
  return WGT_OK;
}
// wgt_trace_hits, and with two fields wgt_trace_rays, behind their preambles.
int trace_hits_sync(wgt_ctx* ctx, const float* rays, uint32_t n, const wgt_hit_buffers& out) {
  wgt_hit_buffers dev;
  const float* d_rays;
  int rc;
  if ((rc = stage_hits(ctx, out, n, dev))) return rc;
  if ((rc = stage(ctx, wgt_ctx::kRays, rays, (size_t)n * 24, d_rays))) return rc;
  if ((rc = hits_launch(ctx, d_rays, n, dev, ctx->stream))) return rc;
  if ((rc = fetch_hits(ctx, out, dev, n))) return rc;
  return sync_stream(ctx);
}

// What an upload and a rebuild alike do once the new scene sc (bound to its allocations) is resident
// and no launch reads the old one: the tree's counts are bvh's (its arrays may be empty), `resident`
// is ps_resident_waves(sc), level_begin the refit's level lists when they are known (a rebuilt tree's;
// empty: the next refit prepares them).  Nothing here can fail.
void install_scene(wgt_ctx* ctx, const DevScene& sc, const BvhOut& bvh, uint32_t resident, size_t device_bytes,
                   std::vector<uint32_t> level_begin) {
  // a new scene: the workspaces' scheduling words are re-zeroed by the next launch's memset
  for (auto& sl : ctx->slots) sl.clean_nb = 0;
  ctx->order.invalidate();  // and its views' orders are the old scene's
  ctx->level_begin = std::move(level_begin);
  free_buf(ctx->motion);  // the old scene's snapshot: no launch reads it any more
  ctx->has_snapshot = false;
  ctx->sc = sc;
  ctx->ps_resident = resident;
  ctx->rad_resident = 0;
  if (env_u32("WGT_DEBUG", 0))
    std::fprintf(stderr, "[wgt] resident: k_render_ps %u waves; LDS stack %u of %u entries, parked %u\n",
                 ctx->ps_resident, sc.ps_cap, sc.stack, sc.ps_park);
  wgt_scene_info& in = ctx->info;
  in = wgt_scene_info{};
  fill_bvh_info(bvh, sc.n_tris, ps_form(sc), in);
  in.n_lights = sc.n_lights; in.n_quads = sc.n_quads; in.n_spheres = sc.n_spheres;
  in.device_bytes = device_bytes;
  in.node_form = reference_node_form(sc);
  in.ps_resident = ctx->ps_resident;
  ctx->has_scene = true;
}

}  // namespace

extern "C" {

int wgt_version(void) { return WGT_API_VERSION; }

const char* wgt_last_error(const wgt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int wgt_device_count(int* count) {
  if (!count) return fail(nullptr, WGT_E_INVALID, "null count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    *count = 0;
    return fail(nullptr, WGT_E_HIP, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = n;
  return WGT_OK;
}

int wgt_create(int hip_device, wgt_ctx** out) {
  if (!out) return fail(nullptr, WGT_E_INVALID, "null out");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0)
    return fail(nullptr, WGT_E_HIP, "no HIP device available (the product has no CPU fallback)");
  if (hip_device < 0 || hip_device >= n) return fail(nullptr, WGT_E_INVALID, "bad device index");
  wgt_ctx* ctx = new wgt_ctx();
  ctx->device = hip_device;
  auto cleanup = [&](const char* what, hipError_t err) {
    std::string m = std::string(what) + ": " + hipGetErrorString(err);
    wgt_destroy(ctx);
    return fail(nullptr, WGT_E_HIP, m);
  };
  if ((e = hipSetDevice(hip_device)) != hipSuccess) return cleanup("hipSetDevice", e);
  if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess)
    return cleanup("hipStreamCreate", e);
  // the sampled kernels' constants, here so that no sampled call, asynchronous ones included, ever copies
  float tab[kSampleBins][4];
  sample_constants(tab);
  if ((e = hipMalloc(&ctx->sample_tab.p, sizeof tab)) != hipSuccess) return cleanup("hipMalloc", e);
  ctx->sample_tab.bytes = sizeof tab;
  if ((e = hipMemcpy(ctx->sample_tab.p, tab, sizeof tab, hipMemcpyHostToDevice)) != hipSuccess)
    return cleanup("hipMemcpy", e);
  *out = ctx;
  return WGT_OK;
}

void wgt_destroy(wgt_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  // every launch that may read the scene or a buffer of the context (trace queries,
  // the workspace slots' renders on any stream, the context stream) ends first
  (void)use_drain(ctx);
  for (hipStream_t& p : ctx->pipe)
    if (p) {
      (void)hipStreamSynchronize(p);
      (void)hipStreamDestroy(p);
    }
  if (ctx->scene_mem) (void)hipFree(ctx->scene_mem);
  for (DevBuf& b : ctx->buf) free_buf(b);
  for (DevBuf& b : ctx->tree) free_buf(b);
  free_buf(ctx->level_order);
  free_buf(ctx->motion);
  free_buf(ctx->sample_tab);
  free_buf(ctx->order_mem);
  for (hipEvent_t e : ctx->order_ev)
    if (e) (void)hipEventDestroy(e);
  for (auto& sl : ctx->slots) {
    if (sl.ev) (void)hipEventSynchronize(sl.ev);
    free_buf(sl.ws);
    if (sl.ev) (void)hipEventDestroy(sl.ev);
  }
  if (ctx->use_ev) (void)hipEventDestroy(ctx->use_ev);
  for (hipEvent_t e : ctx->evpool) (void)hipEventDestroy(e);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

void* wgt_stream(wgt_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

void* wgt_pipeline_stream(wgt_ctx* ctx, uint32_t i) {
  if (!ctx || i >= (uint32_t)wgt_ctx::kMaxWsSlots) {
    (void)fail(ctx, WGT_E_INVALID, "pipeline stream index out of range");
    return nullptr;
  }
  if (!ctx->pipe[i]) {
    if (hipSetDevice(ctx->device) != hipSuccess) return nullptr;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) != hipSuccess || cus <= 0)
      return nullptr;
    std::vector<uint32_t> mask(((size_t)cus + 31) / 32, 0xffffffffu);
    const hipError_t e = hipExtStreamCreateWithCUMask(&ctx->pipe[i], (uint32_t)mask.size(), mask.data());
    if (e != hipSuccess) {
      ctx->pipe[i] = nullptr;
      (void)fail(ctx, WGT_E_HIP, std::string("hipExtStreamCreateWithCUMask: ") + hipGetErrorString(e));
      return nullptr;
    }
  }
  return (void*)ctx->pipe[i];
}

int wgt_sync(wgt_ctx* ctx) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  return sync_stream(ctx);
}

// Host-only exports of the tree (build_for_export).
int wgt_bvh_build(const wgt_triangle* tris, uint32_t n_tris, float* nodes_out, uint32_t nodes_cap,
                  float* tris_out, wgt_scene_info* info) {
  if (!tris || n_tris == 0 || !info) return fail(nullptr, WGT_E_INVALID, "null triangles or info");
  BvhOut bvh;
  const std::string err = build_for_export(tris, n_tris, bvh);
  if (!err.empty()) return fail(nullptr, WGT_E_INVALID, err);
  *info = wgt_scene_info{};
  fill_bvh_info(bvh, n_tris, ps_form_for(bvh, n_tris), *info);
  info->device_bytes = (bvh.nodes.size() + bvh.tris.size() + bvh.tshade.size()) * 4;
  if (nodes_out) {
    if (nodes_cap < bvh.n_nodes) return fail(nullptr, WGT_E_INVALID, "node capacity too small");
    std::memcpy(nodes_out, bvh.nodes.data(), bvh.nodes.size() * 4);
  }
  if (tris_out) std::memcpy(tris_out, bvh.tris.data(), bvh.tris.size() * 4);
  return WGT_OK;
}

int wgt_bvh_build_compact(const wgt_triangle* tris, uint32_t n_tris, uint32_t* cnodes_out, int32_t* crefs_out,
                          uint32_t nodes_cap, float* step_out) {
  if (!tris || n_tris == 0 || !cnodes_out || !crefs_out || !step_out)
    return fail(nullptr, WGT_E_INVALID, "null triangles or outputs");
  BvhOut bvh;
  const std::string err = build_for_export(tris, n_tris, bvh);
  if (!err.empty()) return fail(nullptr, WGT_E_INVALID, err);
  if (nodes_cap < bvh.n_nodes) return fail(nullptr, WGT_E_INVALID, "node capacity too small");
  std::memcpy(cnodes_out, bvh.cnodes.data(), bvh.cnodes.size() * 4);
  std::memcpy(crefs_out, bvh.crefs.data(), bvh.crefs.size() * 4);
  *step_out = bvh.cstep;
  return WGT_OK;
}

int wgt_upload_scene(wgt_ctx* ctx, const wgt_quad* lights, uint32_t n_lights, const wgt_quad* quads,
                     uint32_t n_quads, const wgt_sphere* spheres, uint32_t n_spheres,
                     const wgt_triangle* tris, uint32_t n_tris) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (n_lights < 1 || !lights)
    return fail(ctx, WGT_E_INVALID, "need >= 1 light (sample_from_light reads lights[0])");
  if (n_spheres < 1 || !spheres)
    return fail(ctx, WGT_E_INVALID, "need >= 1 sphere (the reference binds a dummy sphere)");
  if (n_quads > 0 && !quads) return fail(ctx, WGT_E_INVALID, "null quads");
  if (n_tris > 0 && !tris) return fail(ctx, WGT_E_INVALID, "null triangles");
  // the persistent kernel keeps a pending quad hit's index + 1 in 26 bits (wgt_kernels.hip dq)
  if ((uint64_t)n_lights + n_quads >= (1u << 26) - 1u) return fail(ctx, WGT_E_INVALID, "too many lights and quads");
  std::string bad = check_scene_limits(lights, n_lights, spheres, n_spheres, tris, n_tris);
  if (bad.empty() && n_quads) bad = check_scene_limits(quads, n_quads, nullptr, 0, nullptr, 0);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));

  BvhOut bvh;
  const double fixed_ext = std::max(scene_extent(lights, n_lights, spheres, n_spheres, nullptr, 0),
                                    scene_extent(quads, n_quads, nullptr, 0, nullptr, 0));
  if (n_tris > 0) {
    const double ext = std::max(fixed_ext, scene_extent(nullptr, 0, nullptr, 0, tris, n_tris));
    bad = build_bvh(tris, n_tris, ext, bvh);
    if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  }
  const ScenePlan plan = pack_scene(lights, n_lights, quads, n_quads, spheres, n_spheres, n_tris, bvh, DeviceImage(bvh));

  if (int rc = use_drain(ctx)) return rc;  // no launch on any stream may still read the old scene
  if (ctx->scene_mem) {
    (void)hipFree(ctx->scene_mem);
    ctx->scene_mem = nullptr;
  }
  ctx->has_scene = false;
  for (DevBuf& b : ctx->tree) free_buf(b);  // a rebuilt tree and its spare: the upload's tree is in scene_mem
  ctx->tree_cur = -1;
  ctx->fixed_extent = fixed_ext;
  ctx->fixed_bytes = plan.off[kPartNodes];
  ctx->level_begin.clear();
  free_buf(ctx->level_order);
  WGT_HIP(ctx, hipMalloc(&ctx->scene_mem, plan.host.size()));
  WGT_HIP(ctx, hipMemcpy(ctx->scene_mem, plan.host.data(), plan.host.size(), hipMemcpyHostToDevice));
  DevScene sc = plan.sc;
  bind_scene(sc, plan.off, ctx->scene_mem);
  uint32_t resident = 0;
  WGT_HIP(ctx, ps_resident_waves(sc, ctx->device, resident));
  // the next refit prepares the new tree's level lists
  install_scene(ctx, sc, bvh, resident, plan.host.size(), std::vector<uint32_t>());
  return WGT_OK;
}

namespace {

using refit_clock = std::chrono::steady_clock;

// The moved triangles of an update whose checks have passed: host records (staged here), device
// records, or device vertices (verts.verts non-null).
struct MovedInput {
  const wgt_triangle* host_tris;
  const wgt_triangle* d_tris;
  MovedVerts verts;
};

// The refit kernels on the tree of sc, on the context's stream: the records (from d_moved, or from
// verts when verts.verts is set), the boxes level by level, deepest first (level l's nodes are
// d_order[level_begin[l], level_begin[l + 1])), then the compact form for ray origins within the
// scene's `extent`: its step and bound M come back.  An update runs them on the resident tree, a
// rebuild on the tree it is making.
int refit_tree(wgt_ctx* ctx, const DevScene& sc, const uint32_t* d_order, const std::vector<uint32_t>& level_begin,
               uint32_t* d_max_exp, double extent, const wgt_triangle* d_moved, const MovedVerts& verts, float& step,
               double& M) {
  int rc;
  hipStream_t s = ctx->stream;
  WGT_HIP(ctx, hipMemsetAsync(d_max_exp, 0, 4, s));
  if (verts.verts) WGT_HIP(ctx, launch_refit_verts(sc, verts, s));
  else WGT_HIP(ctx, launch_refit_tris(sc, d_moved, s));
  for (size_t l = level_begin.size() - 1; l-- > 0;)
    WGT_HIP(ctx, launch_refit_nodes(sc, d_order + level_begin[l], level_begin[l + 1] - level_begin[l], s));
  float root[kNode4Floats];
  if ((rc = fetch(ctx, root, sc.nodes, sizeof root)) || (rc = sync_stream(ctx))) return rc;
  M = compact_bound(extent, root);
  const double G = std::ldexp(M, -21);
  WGT_HIP(ctx, launch_refit_step(sc, G, d_max_exp, s));
  uint32_t max_exp = 0;
  if ((rc = fetch(ctx, &max_exp, d_max_exp, 4)) || (rc = sync_stream(ctx))) return rc;
  step = pow2f(kCompactMinExp + (int)max_exp);
  WGT_HIP(ctx, launch_refit_compact(sc, step, G, s));
  return WGT_OK;
}

// The refit that the three updates share, after their checks: `extent` is the scene's with the new
// triangles, t0 the call's start (the host part of wgt_update_timing ends at the first refit
// kernel).  The entry points differ only in how the records get written.
int refit_resident(wgt_ctx* ctx, refit_clock::time_point t0, double extent, const MovedInput& in) {
  int rc;
  if ((rc = use_drain(ctx))) return rc;  // no launch on any stream may still read the old tree
  DevScene& sc = ctx->sc;
  hipStream_t s = ctx->stream;
  if (ctx->level_begin.empty()) {  // the first refit of this scene: its level lists
    std::vector<uint8_t> level(sc.n_nodes);
    WGT_HIP(ctx, hipMemcpy(level.data(), sc.node_level, level.size(), hipMemcpyDeviceToHost));
    std::vector<uint32_t> order, begin;
    const std::string deep = refit_levels(level.data(), sc.n_nodes, order, begin);
    if (!deep.empty()) return fail(ctx, WGT_E_INVALID, deep);
    if ((rc = ensure(ctx, ctx->level_order, ((size_t)sc.n_nodes + 1) * 4))) return rc;
    WGT_HIP(ctx, hipMemcpy(ctx->level_order.p, order.data(), order.size() * 4, hipMemcpyHostToDevice));
    ctx->level_begin = std::move(begin);
  }
  const uint32_t* d_order = (const uint32_t*)ctx->level_order.p;
  uint32_t* d_max_exp = (uint32_t*)ctx->level_order.p + sc.n_nodes;
  const wgt_triangle* d_moved = in.d_tris;
  if (in.host_tris) {
    if ((rc = stage(ctx, wgt_ctx::kMoved, in.host_tris, (size_t)sc.n_tris * sizeof(wgt_triangle), d_moved))) return rc;
    if ((rc = sync_stream(ctx))) return rc;  // the staging copy belongs to the host part's time
  }
  hipEvent_t e0 = pool_event(ctx, 0), e1 = pool_event(ctx, 1);
  if (!e0 || !e1) return fail(ctx, WGT_E_HIP, "hipEventCreate failed");
  const refit_clock::time_point t1 = refit_clock::now();
  // from here on the resident tree changes: a HIP failure leaves it undefined until the next upload
  for (auto& sl : ctx->slots) sl.clean_nb = 0;  // as an upload
  ctx->order.invalidate();
  WGT_HIP(ctx, hipEventRecord(e0, s));
  float step;
  double M;
  if ((rc = refit_tree(ctx, sc, d_order, ctx->level_begin, d_max_exp, extent, d_moved, in.verts, step, M))) return rc;
  WGT_HIP(ctx, hipEventRecord(e1, s));
  WGT_HIP(ctx, hipEventSynchronize(e1));
  WGT_HIP(ctx, hipEventElapsedTime(&ctx->refit_device_ms, e0, e1));
  ctx->refit_host_ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
  sc.cstep = step;
  sc.rcstep = 1.0f / step;  // a power of two: exact
  sc.cbound = (float)M;
  ctx->info.bvh_compact_step = step;
  ctx->info.node_form = reference_node_form(sc);
  return WGT_OK;
}

// The device check of moved triangles in device memory, on the caller's stream `s` (so after
// everything queued there), and its result read back; the stream has drained when it returns, so
// the refit on the context's stream may read the input.  It writes a scratch word of the
// context's alone: a refusal leaves the scene as it was.
int check_on_device(wgt_ctx* ctx, hipStream_t s, const wgt_triangle* d_tris, uint32_t n_tris, const MovedVerts& verts,
                    RefitCheck& out) {
  RefitCheck* d_check;
  if (int rc = scratch(ctx, wgt_ctx::kCheck, sizeof(RefitCheck), d_check)) return rc;
  WGT_HIP(ctx, hipMemsetAsync(&d_check->extent_bits, 0, sizeof d_check->extent_bits, s));
  WGT_HIP(ctx, hipMemsetAsync(&d_check->first_bad, 0xff, 2 * sizeof(uint32_t), s));  // kNoBadTriangle
  if (verts.verts) WGT_HIP(ctx, launch_check_verts(verts, d_check, s));
  else WGT_HIP(ctx, launch_check_tris(d_tris, n_tris, d_check, s));
  WGT_HIP(ctx, hipMemcpyAsync(&out, d_check, sizeof out, hipMemcpyDeviceToHost, s));
  WGT_HIP(ctx, hipStreamSynchronize(s));
  return WGT_OK;
}

// The refusal of the device check's triangle `i` of the records d_tris, in check_triangle_limits' words.
int refuse_checked(wgt_ctx* ctx, const wgt_triangle* d_tris, uint32_t n_tris, uint32_t i) {
  if (i >= n_tris) return fail(ctx, WGT_E_HIP, "the device check named a triangle past the end");
  wgt_triangle t;
  WGT_HIP(ctx, hipMemcpy(&t, d_tris + i, sizeof t, hipMemcpyDeviceToHost));
  const std::string bad = check_triangle_limits(t, i);
  return fail(ctx, WGT_E_INVALID, bad.empty() ? "triangle " + std::to_string(i) + ": beyond the scene limits" : bad);
}

// The rebuild that both forms share, after their argument checks: d_tris are n device records that
// everything queued on `cs` has written, `leaf` the leaf target.  The new tree is made in the spare
// allocation and swapped in at the end, so a refusal or a HIP failure leaves the scene as it was.
int rebuild_resident(wgt_ctx* ctx, refit_clock::time_point t0, const wgt_triangle* d_tris, uint32_t n, uint32_t leaf,
                     hipStream_t cs) {
  int rc;
  RefitCheck chk;
  if ((rc = check_on_device(ctx, cs, d_tris, n, MovedVerts{}, chk))) return rc;
  if (chk.first_bad != kNoBadTriangle) return refuse_checked(ctx, d_tris, n, chk.first_bad);
  const double extent = std::max(ctx->fixed_extent, checked_extent(chk));
  if ((rc = use_drain(ctx))) return rc;  // every launch of the context has ended when the trees are swapped
  hipStream_t s = ctx->stream;
  const uint32_t cap = rebuild_node_cap(n);
  size_t temp_bytes = 0;
  WGT_HIP(ctx, rebuild_temp_bytes(n, cap, temp_bytes));
  const RebuildScratch ws = plan_rebuild_scratch(n, temp_bytes);
  char* w;
  if ((rc = scratch(ctx, wgt_ctx::kRebuild, ws.bytes, w))) return rc;
  const int spare = ctx->tree_cur == 0 ? 1 : 0;
  size_t off[kSceneParts] = {};
  if ((rc = ensure(ctx, ctx->tree[spare], tree_layout(n, cap, off)))) return rc;
  DevScene sc = ctx->sc;  // the lights, quads and spheres stay
  bind_tree(sc, off, ctx->tree[spare].p);
  // the level lists' buffer is written below: the resident tree's lists are dropped first, so that its
  // next refit prepares them again should this call fail
  ctx->level_begin.clear();
  if ((rc = ensure(ctx, ctx->level_order, ((size_t)cap + 1) * 4))) return rc;
  uint32_t* d_order = (uint32_t*)ctx->level_order.p;
  hipEvent_t e0 = pool_event(ctx, 0), e1 = pool_event(ctx, 1);
  if (!e0 || !e1) return fail(ctx, WGT_E_HIP, "hipEventCreate failed");
  unsigned long long* d_key[2] = {(unsigned long long*)(w + ws.key[0]), (unsigned long long*)(w + ws.key[1])};
  uint32_t* d_val[2] = {(uint32_t*)(w + ws.val[0]), (uint32_t*)(w + ws.val[1])};
  RebuildRange* d_list[2] = {(RebuildRange*)(w + ws.list[0]), (RebuildRange*)(w + ws.list[1])};
  uint4* d_cuts = (uint4*)(w + ws.cuts);
  uint32_t *d_count = (uint32_t*)(w + ws.count), *d_offset = (uint32_t*)(w + ws.offset);
  RebuildBounds* d_bounds = (RebuildBounds*)(w + ws.bounds);
  RebuildStats* d_stats = (RebuildStats*)(w + ws.stats);
  const RebuildTree tree{(float4*)sc.nodes, (float4*)sc.tris, (uint4*)sc.cnodes, (uint8_t*)sc.node_level, n, cap, leaf};

  const refit_clock::time_point t1 = refit_clock::now();
  WGT_HIP(ctx, hipEventRecord(e0, s));
  WGT_HIP(ctx, hipMemsetAsync(d_bounds->lo, 0xff, sizeof d_bounds->lo, s));
  WGT_HIP(ctx, hipMemsetAsync(d_bounds->hi, 0, sizeof d_bounds->hi, s));
  WGT_HIP(ctx, hipMemsetAsync(d_stats, 0, sizeof *d_stats, s));
  WGT_HIP(ctx, launch_rebuild_bounds(d_tris, n, d_bounds, s));
  WGT_HIP(ctx, launch_rebuild_keys(d_tris, n, d_bounds, d_key[0], d_val[0], s));
  WGT_HIP(ctx, launch_rebuild_sort(w + ws.temp, temp_bytes, d_key[0], d_key[1], d_val[0], d_val[1], n, s));
  BvhOut counts;  // the tree's counts, as a build reports them; no BVH2 exists
  std::vector<uint32_t> level_count;
  if (n <= leaf) {
    WGT_HIP(ctx, launch_rebuild_single(tree, d_val[1], s));
    counts.n_nodes = counts.n_leaves = counts.max_depth = counts.stack_need = 1;
    counts.max_leaf = n;
    level_count.push_back(1u);
  } else {
    const RebuildRange root{0u, n, 2 * kRebuildLevels, 0u};
    WGT_HIP(ctx, hipMemcpyAsync(d_list[0], &root, sizeof root, hipMemcpyHostToDevice, s));
    uint32_t first = 0, count = 1;
    for (uint32_t level = 0; count != 0; ++level) {
      if (level >= kRebuildLevels) return fail(ctx, WGT_E_HIP, "rebuild: the tree is deeper than its budget");  // never
      const RebuildRange* cur = d_list[level & 1u];
      WGT_HIP(ctx, launch_rebuild_count(d_key[1], cur, count, leaf, d_cuts, d_count, s));
      WGT_HIP(ctx, launch_rebuild_scan(w + ws.temp, temp_bytes, d_count, d_offset, count, s));
      uint32_t next = 0;
      if ((rc = fetch(ctx, &next, d_offset + count, 4)) || (rc = sync_stream(ctx))) return rc;
      if ((uint64_t)first + count + next > cap) return fail(ctx, WGT_E_HIP, "rebuild: more nodes than triangles");  // never
      WGT_HIP(ctx, launch_rebuild_write(tree, cur, d_cuts, d_offset, d_val[1], first, count, level, d_list[~level & 1u],
                                        d_stats, s));
      level_count.push_back(count);
      first += count;
      count = next;
    }
    RebuildStats st;
    if ((rc = fetch(ctx, &st, d_stats, sizeof st)) || (rc = sync_stream(ctx))) return rc;
    counts.n_nodes = first;
    counts.n_leaves = st.n_leaves;
    counts.max_leaf = st.max_leaf;
    counts.stack_need = st.stack_need;
    counts.max_depth = (uint32_t)level_count.size();
    if (st.stack_need > (uint32_t)kStackMax) return fail(ctx, WGT_E_HIP, "rebuild: the stack need exceeds the kernels' limit");  // never
  }
  plan_tree_form(counts, n, sc);
  std::vector<uint32_t> level_begin = level_begin_of(level_count);
  WGT_HIP(ctx, launch_rebuild_iota(d_order, sc.n_nodes, s));
  float step;
  double M;
  if ((rc = refit_tree(ctx, sc, d_order, level_begin, d_order + sc.n_nodes, extent, d_tris, MovedVerts{}, step, M))) return rc;
  WGT_HIP(ctx, hipEventRecord(e1, s));
  WGT_HIP(ctx, hipEventSynchronize(e1));
  WGT_HIP(ctx, hipEventElapsedTime(&ctx->refit_device_ms, e0, e1));
  ctx->refit_host_ms = std::chrono::duration<float, std::milli>(t1 - t0).count();
  sc.cstep = counts.cstep = step;
  sc.rcstep = 1.0f / step;  // a power of two: exact
  sc.cbound = (float)M;
  uint32_t resident = 0;
  WGT_HIP(ctx, ps_resident_waves(sc, ctx->device, resident));
  // the swap: the old tree's allocation (if it is one of the two) becomes the spare
  ctx->tree_cur = spare;
  size_t used[kSceneParts] = {};
  install_scene(ctx, sc, counts, resident, ctx->fixed_bytes + tree_layout(n, sc.n_nodes, used), std::move(level_begin));
  return WGT_OK;
}

}  // namespace

int wgt_update_triangles(wgt_ctx* ctx, const wgt_triangle* tris, uint32_t n_tris) {
  const refit_clock::time_point t0 = refit_clock::now();
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (!ctx->has_scene) return fail(ctx, WGT_E_NOSCENE, "no scene uploaded");
  if (!tris) return fail(ctx, WGT_E_INVALID, "null triangles");
  std::string bad = check_update_count(ctx->sc.n_tris, n_tris);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  // a refusal leaves the device untouched: under the limits every triangle box is finite
  bad = check_scene_limits(nullptr, 0, nullptr, 0, tris, n_tris);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  const double extent = std::max(ctx->fixed_extent, scene_extent(nullptr, 0, nullptr, 0, tris, n_tris));
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  return refit_resident(ctx, t0, extent, MovedInput{tris, nullptr, MovedVerts{}});
}

int wgt_update_triangles_device(wgt_ctx* ctx, const wgt_triangle* d_tris, uint32_t n_tris, void* stream) {
  const refit_clock::time_point t0 = refit_clock::now();
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (!ctx->has_scene) return fail(ctx, WGT_E_NOSCENE, "no scene uploaded");
  std::string bad = check_update_records(d_tris, ctx->sc.n_tris, n_tris);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream_or_own(ctx, stream);
  RefitCheck chk;
  if (int rc = check_on_device(ctx, s, d_tris, n_tris, MovedVerts{}, chk)) return rc;
  if (chk.first_bad != kNoBadTriangle) return refuse_checked(ctx, d_tris, n_tris, chk.first_bad);
  const double extent = std::max(ctx->fixed_extent, checked_extent(chk));
  return refit_resident(ctx, t0, extent, MovedInput{nullptr, d_tris, MovedVerts{}});
}

int wgt_update_vertices_device(wgt_ctx* ctx, const float* d_verts, uint32_t n_verts, const uint32_t* d_index,
                               uint32_t n_tris, void* stream) {
  const refit_clock::time_point t0 = refit_clock::now();
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (!ctx->has_scene) return fail(ctx, WGT_E_NOSCENE, "no scene uploaded");
  std::string bad = check_update_vertices(d_verts, n_verts, d_index, ctx->sc.n_tris, n_tris);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  hipStream_t s = stream_or_own(ctx, stream);
  const MovedVerts verts{d_verts, n_verts, d_index, n_tris};
  RefitCheck chk;
  if (int rc = check_on_device(ctx, s, nullptr, n_tris, verts, chk)) return rc;
  if (chk.first_bad != kNoBadTriangle) {  // read that triangle back and word the refusal as the host form does
    const uint32_t i = chk.first_bad;
    if (i >= n_tris) return fail(ctx, WGT_E_HIP, "the device check named a triangle past the end");
    uint32_t k[3] = {3u * i, 3u * i + 1u, 3u * i + 2u};  // unindexed: within n_verts = 3 n_tris
    if (d_index) WGT_HIP(ctx, hipMemcpy(k, d_index + (size_t)3 * i, sizeof k, hipMemcpyDeviceToHost));
    bad = check_vertex_index(k, n_verts, i);
    if (bad.empty()) {
      float v[9];
      for (int c = 0; c < 3; ++c)
        WGT_HIP(ctx, hipMemcpy(v + 3 * c, d_verts + (size_t)3 * k[c], 3 * sizeof(float), hipMemcpyDeviceToHost));
      wgt_triangle t;
      triangle_of_vertices(v, t);
      bad = check_triangle_limits(t, i);
    }
    return fail(ctx, WGT_E_INVALID, bad.empty() ? "triangle " + std::to_string(i) + ": beyond the scene limits" : bad);
  }
  const double extent = std::max(ctx->fixed_extent, checked_extent(chk));
  return refit_resident(ctx, t0, extent, MovedInput{nullptr, nullptr, verts});
}

int wgt_rebuild_triangles_device(wgt_ctx* ctx, const wgt_triangle* d_tris, uint32_t n_tris, void* stream) {
  const refit_clock::time_point t0 = refit_clock::now();
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (!ctx->has_scene) return fail(ctx, WGT_E_NOSCENE, "no scene uploaded");
  const uint32_t leaf = RebuildLeafFromEnv();
  const std::string bad = check_rebuild_records(d_tris, n_tris, leaf, true);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  return rebuild_resident(ctx, t0, d_tris, n_tris, leaf, stream_or_own(ctx, stream));
}

int wgt_rebuild_triangles(wgt_ctx* ctx, const wgt_triangle* tris, uint32_t n_tris) {
  const refit_clock::time_point t0 = refit_clock::now();
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (!ctx->has_scene) return fail(ctx, WGT_E_NOSCENE, "no scene uploaded");
  const uint32_t leaf = RebuildLeafFromEnv();
  const std::string bad = check_rebuild_records(tris, n_tris, leaf, false);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  const wgt_triangle* d_tris;  // staged on the context's stream, which the body's check then reads on
  if (int rc = stage(ctx, wgt_ctx::kMoved, tris, (size_t)n_tris * sizeof(wgt_triangle), d_tris)) return rc;
  return rebuild_resident(ctx, t0, d_tris, n_tris, leaf, ctx->stream);
}

int wgt_bvh_build_morton(const wgt_triangle* tris, uint32_t n_tris, float* nodes_out, uint32_t nodes_cap,
                         float* tris_out, uint32_t* cnodes_out, int32_t* crefs_out, float* step_out,
                         wgt_scene_info* info) {
  if (!tris || n_tris == 0 || !info) return fail(nullptr, WGT_E_INVALID, "null triangles or info");
  // what a rebuild refuses before it builds
  std::string bad = check_rebuild_records(tris, n_tris, RebuildLeafFromEnv(), false);
  if (bad.empty()) bad = check_scene_limits(nullptr, 0, nullptr, 0, tris, n_tris);
  if (!bad.empty()) return fail(nullptr, WGT_E_INVALID, bad);
  BvhOut bvh;
  const std::string err = morton_for_export(tris, n_tris, bvh);
  if (!err.empty()) return fail(nullptr, WGT_E_INVALID, err);
  *info = wgt_scene_info{};
  fill_bvh_info(bvh, n_tris, ps_form_for(bvh, n_tris), *info);
  info->device_bytes = (bvh.nodes.size() + bvh.tris.size() + bvh.tshade.size()) * 4;
  if ((nodes_out || cnodes_out || crefs_out) && nodes_cap < bvh.n_nodes)
    return fail(nullptr, WGT_E_INVALID, "node capacity too small");
  if (nodes_out) std::memcpy(nodes_out, bvh.nodes.data(), bvh.nodes.size() * 4);
  if (tris_out) std::memcpy(tris_out, bvh.tris.data(), bvh.tris.size() * 4);
  if (cnodes_out) std::memcpy(cnodes_out, bvh.cnodes.data(), bvh.cnodes.size() * 4);
  if (crefs_out) std::memcpy(crefs_out, bvh.crefs.data(), bvh.crefs.size() * 4);
  if (step_out) *step_out = bvh.cstep;
  return WGT_OK;
}

int wgt_update_timing(const wgt_ctx* ctx, float* host_ms, float* device_ms) {
  if (!ctx || !host_ms || !device_ms) return fail(nullptr, WGT_E_INVALID, "null argument");
  *host_ms = ctx->refit_host_ms;
  *device_ms = ctx->refit_device_ms;
  return WGT_OK;
}

int wgt_bvh_read(wgt_ctx* ctx, float* nodes_out, uint32_t nodes_cap, float* tris_out, uint32_t* cnodes_out,
                 int32_t* crefs_out, float* step_out) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (!ctx->has_scene) return fail(ctx, WGT_E_NOSCENE, "no scene uploaded");
  const DevScene& sc = ctx->sc;
  if (sc.n_tris == 0) return fail(ctx, WGT_E_INVALID, "the scene has no triangles, so no tree");
  if ((nodes_out || cnodes_out || crefs_out) && nodes_cap < sc.n_nodes)
    return fail(ctx, WGT_E_INVALID, "node capacity too small");
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = use_drain(ctx)) return rc;
  std::vector<float> nodes((size_t)sc.n_nodes * kNode4Floats);
  std::vector<uint32_t> crecs((size_t)sc.n_nodes * kCRecordFloat4s * 4);
  WGT_HIP(ctx, hipMemcpy(nodes.data(), sc.nodes, nodes.size() * 4, hipMemcpyDeviceToHost));
  WGT_HIP(ctx, hipMemcpy(crecs.data(), sc.cnodes, crecs.size() * 4, hipMemcpyDeviceToHost));
  ExportImage(nodes.data(), crecs.data(), sc.n_nodes, nodes_out, cnodes_out, crefs_out);
  if (tris_out)
    WGT_HIP(ctx, hipMemcpy(tris_out, sc.tris, (size_t)sc.n_tris * kTriRecordBytes, hipMemcpyDeviceToHost));
  if (step_out) *step_out = sc.cstep;
  return WGT_OK;
}

int wgt_bvh_refit(const wgt_triangle* built_from, const wgt_triangle* now, uint32_t n_tris, float* nodes_out,
                  uint32_t nodes_cap, float* tris_out, uint32_t* cnodes_out, int32_t* crefs_out, float* step_out,
                  wgt_scene_info* info) {
  if (!built_from || !now || n_tris == 0 || !info) return fail(nullptr, WGT_E_INVALID, "null triangles or info");
  // what wgt_update_triangles refuses before it refits
  const std::string bad = check_scene_limits(nullptr, 0, nullptr, 0, now, n_tris);
  if (!bad.empty()) return fail(nullptr, WGT_E_INVALID, bad);
  BvhOut bvh;
  const std::string err = refit_for_export(built_from, now, n_tris, bvh);
  if (!err.empty()) return fail(nullptr, WGT_E_INVALID, err);
  *info = wgt_scene_info{};
  fill_bvh_info(bvh, n_tris, ps_form_for(bvh, n_tris), *info);
  info->device_bytes = (bvh.nodes.size() + bvh.tris.size() + bvh.tshade.size()) * 4;
  if ((nodes_out || cnodes_out || crefs_out) && nodes_cap < bvh.n_nodes)
    return fail(nullptr, WGT_E_INVALID, "node capacity too small");
  if (nodes_out) std::memcpy(nodes_out, bvh.nodes.data(), bvh.nodes.size() * 4);
  if (tris_out) std::memcpy(tris_out, bvh.tris.data(), bvh.tris.size() * 4);
  if (cnodes_out) std::memcpy(cnodes_out, bvh.cnodes.data(), bvh.cnodes.size() * 4);
  if (crefs_out) std::memcpy(crefs_out, bvh.crefs.data(), bvh.crefs.size() * 4);
  if (step_out) *step_out = bvh.cstep;
  return WGT_OK;
}

int wgt_scene_info_get(const wgt_ctx* ctx, wgt_scene_info* info) {
  if (!ctx || !info) return fail(nullptr, WGT_E_INVALID, "null argument");
  if (!ctx->has_scene) return fail(const_cast<wgt_ctx*>(ctx), WGT_E_NOSCENE, "no scene uploaded");
  *info = ctx->info;
  return WGT_OK;
}

int wgt_order_info(const wgt_ctx* ctx, wgt_order_stats* out) {
  if (!ctx || !out) return fail(nullptr, WGT_E_INVALID, "null argument");
  *out = wgt_order_stats{};
  ctx->order.counts(out->today, out->refine, out->reuse, out->invalidations);
  if (ctx->order.current() >= 0) {
    out->nb = ctx->order.current_key().nb;
    out->refine_side = ctx->order.current_side();
  }
  return WGT_OK;
}

int wgt_order_read(wgt_ctx* ctx, uint32_t* perm_out, uint32_t cap, uint32_t* n_out) {
  if (!ctx || !n_out) return fail(ctx, WGT_E_INVALID, "null argument");
  *n_out = 0;
  const int b = ctx->order.current();
  if (b < 0) return WGT_OK;
  const uint32_t nb = ctx->order.current_key().nb;
  if (!perm_out || cap < nb) return fail(ctx, WGT_E_INVALID, "order capacity too small");
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  WGT_HIP(ctx, hipEventSynchronize(ctx->order_ev[b]));  // the sort that wrote it
  WGT_HIP(ctx, hipMemcpy(perm_out, order_buf(ctx, b), (size_t)nb * 4, hipMemcpyDeviceToHost));
  *n_out = nb;
  return WGT_OK;
}

int wgt_order_reset(wgt_ctx* ctx) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  ctx->order.invalidate();
  return WGT_OK;
}

int wgt_render_tiles_async(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H,
                           uint32_t tw, uint32_t th, const wgt_tile* d_tiles, uint32_t n_tiles,
                           void* d_rgba8, float* d_rgba32f, uint32_t* d_hit_id, void* stream) {
  WGT_BEGIN(tiles_begin(ctx, cam, W, H, tw, th, d_tiles, n_tiles, false, nullptr, nullptr));
  const DevFrame fr = tile_frame(*cam, W, H, tw, th, n_tiles);
  return render_frame(ctx, fr, SampleArgs{}, d_tiles, tiles_at(d_tiles), (uchar4*)d_rgba8, (float4*)d_rgba32f, d_hit_id, nullptr,
                      stream_or_own(ctx, stream), nullptr);
}

int wgt_render_tiles_stats(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H,
                           uint32_t tw, uint32_t th, const wgt_tile* d_tiles, uint32_t n_tiles,
                           wgt_stats* stats) {
  WGT_BEGIN(tiles_begin(ctx, cam, W, H, tw, th, d_tiles, n_tiles, true, stats, nullptr));
  return count_frame(ctx, tile_frame(*cam, W, H, tw, th, n_tiles), SampleArgs{}, d_tiles, tiles_at(d_tiles), stats);
}

int wgt_render_tiles_profile(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H,
                             uint32_t tw, uint32_t th, const wgt_tile* d_tiles, uint32_t n_tiles,
                             wgt_stats* stats) {
  WGT_BEGIN(tiles_begin(ctx, cam, W, H, tw, th, d_tiles, n_tiles, true, stats, nullptr));
  int rc;
  const DevFrame fr = tile_frame(*cam, W, H, tw, th, n_tiles);
  float ms = 0.0f;
  if ((rc = render_frame(ctx, fr, SampleArgs{}, d_tiles, tiles_at(d_tiles), nullptr, nullptr, nullptr, nullptr, ctx->stream, &ms)))
    return rc;
  if ((rc = sync_stream(ctx))) return rc;
  fill_timing(ms, stats);
  return WGT_OK;
}

int wgt_render_frames(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H,
                      const uint32_t* seeds, uint32_t n_frames, uint8_t* rgba8_out, wgt_stats* stats) {
  int rc = check_render_args(ctx, cam, W, H, W, H);
  if (rc) return rc;
  if (n_frames == 0) return WGT_OK;
  if (!seeds || !rgba8_out) return fail(ctx, WGT_E_INVALID, "null seeds or output");
  const size_t npx = (size_t)W * H;
  if (npx * n_frames > 0xffffffffull / 4) return fail(ctx, WGT_E_INVALID, "batch too large");
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  // one full-frame tile per frame: the compact tile output is frame after frame
  std::vector<wgt_tile> tl(n_frames);
  for (uint32_t j = 0; j < n_frames; ++j) tl[j] = wgt_tile{0u, 0u, seeds[j], j};
  uchar4* d_out8;
  const wgt_tile* d_tiles;
  if ((rc = scratch(ctx, wgt_ctx::kOut8, npx * n_frames * 4, d_out8))) return rc;
  if ((rc = stage(ctx, wgt_ctx::kTiles, tl.data(), n_frames * sizeof(wgt_tile), d_tiles))) return rc;
  const DevFrame fr = tile_frame(*cam, W, H, W, H, n_frames);
  float ms = 0.0f;
  if ((rc = render_frame(ctx, fr, SampleArgs{}, d_tiles, tiles_of(tl.data(), n_frames), d_out8, nullptr, nullptr, nullptr,
                         ctx->stream, stats ? &ms : nullptr)))
    return rc;
  if ((rc = fetch(ctx, rgba8_out, d_out8, npx * n_frames * 4)) || (rc = sync_stream(ctx))) return rc;
  return stats ? stats_of_render(ctx, cam, W, H, W, H, n_frames, ms, stats) : WGT_OK;
}

}  // extern "C"

namespace {

// The sampled calls' map and the context's table for the kernels.
SampleArgs sample_args(const wgt_ctx* ctx, const uint8_t* d_map) {
  return SampleArgs{d_map, (const float4*)ctx->sample_tab.p};
}
// ... and their camera: cam's with its spp taken as 1, kept in `store`; a null one stays null for the
// checks to refuse in their order.
const wgt_camera_param* sampled_cam(const wgt_camera_param* cam, wgt_camera_param& store) {
  if (!cam) return nullptr;
  store = sampled_camera(*cam);
  return &store;
}

// wgt_render_tile, and with a host sample map (sampled) wgt_render_tile_sampled: the map is checked
// last and staged on the context's stream; the camera's spp is then taken as 1.
int render_tile(wgt_ctx* ctx, const wgt_camera_param* cam_in, uint32_t W, uint32_t H, uint32_t x0, uint32_t y0,
                uint32_t tw, uint32_t th, bool sampled, const uint8_t* sample_map, uint8_t* rgba8_out,
                float* rgba32f_out, uint32_t* hit_id_out, wgt_stats* stats) {
  wgt_camera_param c1;
  const wgt_camera_param* cam = sampled ? sampled_cam(cam_in, c1) : cam_in;
  int rc = check_render_args(ctx, cam, W, H, tw, th);
  if (rc) return rc;
  if (x0 >= W || y0 >= H) return fail(ctx, WGT_E_INVALID, "tile origin outside the frame");
  if (sampled)
    if (const char* bad = check_sample_map(sample_map)) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  const size_t npx = (size_t)tw * th;
  const wgt_tile tile{x0, y0, cam->seed, 0u};
  uchar4* d_out8 = nullptr;
  float4* d_out32 = nullptr;
  uint32_t* d_hit = nullptr;
  const wgt_tile* d_tile;
  SampleArgs sm{};
  if (sampled) {
    const uint8_t* d_map;
    if ((rc = stage(ctx, wgt_ctx::kSampleMap, sample_map, (size_t)W * H, d_map))) return rc;
    sm = sample_args(ctx, d_map);
  }
  if (rgba8_out && (rc = scratch(ctx, wgt_ctx::kOut8, npx * 4, d_out8))) return rc;
  if (rgba32f_out && (rc = scratch(ctx, wgt_ctx::kOut32, npx * 16, d_out32))) return rc;
  if (hit_id_out && (rc = scratch(ctx, wgt_ctx::kHit, npx * 4, d_hit))) return rc;
  if ((rc = stage(ctx, wgt_ctx::kTiles, &tile, sizeof tile, d_tile))) return rc;
  // Pixels of a partially covered tile that fall outside the frame are not written
  // by the kernel (path_tracer.wgsl:377); give them defined contents.
  if (x0 + (uint64_t)tw > W || y0 + (uint64_t)th > H) {
    if (d_out8) WGT_HIP(ctx, hipMemsetAsync(d_out8, 0, npx * 4, ctx->stream));
    if (d_out32) WGT_HIP(ctx, hipMemsetAsync(d_out32, 0, npx * 16, ctx->stream));
    if (d_hit) WGT_HIP(ctx, hipMemsetAsync(d_hit, 0xff, npx * 4, ctx->stream));
  }
  const DevFrame fr = tile_frame(*cam, W, H, tw, th, 1);
  float ms = 0.0f;
  if ((rc = render_frame(ctx, fr, sm, d_tile, tiles_of(&tile, 1), d_out8, d_out32, d_hit, nullptr, ctx->stream,
                         stats ? &ms : nullptr)))
    return rc;
  if (d_out8 && (rc = fetch(ctx, rgba8_out, d_out8, npx * 4))) return rc;
  if (d_out32 && (rc = fetch(ctx, rgba32f_out, d_out32, npx * 16))) return rc;
  if (d_hit && (rc = fetch(ctx, hit_id_out, d_hit, npx * 4))) return rc;
  if ((rc = sync_stream(ctx))) return rc;
  if (!stats) return WGT_OK;
  if (!sampled) return stats_of_render(ctx, cam, W, H, tw, th, 1, ms, stats);
  std::memset(stats, 0, sizeof *stats);
  if ((rc = count_frame(ctx, fr, sm, d_tile, tiles_of(&tile, 1), stats))) return rc;
  fill_timing(ms, stats);
  return WGT_OK;
}

}  // namespace

extern "C" {

int wgt_render_tile(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H, uint32_t x0,
                    uint32_t y0, uint32_t tw, uint32_t th, uint8_t* rgba8_out, float* rgba32f_out,
                    uint32_t* hit_id_out, wgt_stats* stats) {
  return render_tile(ctx, cam, W, H, x0, y0, tw, th, false, nullptr, rgba8_out, rgba32f_out, hit_id_out, stats);
}

int wgt_render_tile_sampled(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H, uint32_t x0,
                            uint32_t y0, uint32_t tw, uint32_t th, const uint8_t* sample_map, uint8_t* rgba8_out,
                            float* rgba32f_out, uint32_t* hit_id_out, wgt_stats* stats) {
  return render_tile(ctx, cam, W, H, x0, y0, tw, th, true, sample_map, rgba8_out, rgba32f_out, hit_id_out, stats);
}

int wgt_render_tiles_sampled_async(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H, uint32_t tw,
                                   uint32_t th, const wgt_tile* d_tiles, uint32_t n_tiles, const uint8_t* d_sample_map,
                                   void* d_rgba8, float* d_rgba32f, uint32_t* d_hit_id, void* stream) {
  wgt_camera_param c1;
  cam = sampled_cam(cam, c1);
  WGT_BEGIN(tiles_begin(ctx, cam, W, H, tw, th, d_tiles, n_tiles, false, nullptr, check_sample_map(d_sample_map)));
  const DevFrame fr = tile_frame(*cam, W, H, tw, th, n_tiles);
  return render_frame(ctx, fr, sample_args(ctx, d_sample_map), d_tiles, tiles_at(d_tiles), (uchar4*)d_rgba8, (float4*)d_rgba32f,
                      d_hit_id, nullptr,
                      stream_or_own(ctx, stream), nullptr);
}

int wgt_trace_rays_async(wgt_ctx* ctx, const float* d_rays, uint32_t n, uint32_t* d_prim_id,
                         float* d_dist, void* stream) {
  WGT_BEGIN(query_begin(ctx, n, null_buffer(!d_rays || !d_prim_id || !d_dist)));
  // the closest-hit query is the hit-record one with two fields
  const wgt_hit_buffers dev{d_prim_id, d_dist, nullptr, nullptr, nullptr, nullptr};
  return hits_launch(ctx, d_rays, n, dev, stream_or_own(ctx, stream));
}

int wgt_trace_rays(wgt_ctx* ctx, const float* rays, uint32_t n, uint32_t* prim_id, float* dist) {
  WGT_BEGIN(query_begin(ctx, n, null_buffer(!rays || !prim_id || !dist)));
  return trace_hits_sync(ctx, rays, n, wgt_hit_buffers{prim_id, dist, nullptr, nullptr, nullptr, nullptr});
}

int wgt_occluded_rays_async(wgt_ctx* ctx, const float* d_rays, const float* d_max_dist, uint32_t n,
                            uint8_t* d_occluded, void* stream) {
  WGT_BEGIN(query_begin(ctx, n, null_buffer(!d_rays || !d_max_dist || !d_occluded)));
  return occluded_launch(ctx, d_rays, d_max_dist, n, d_occluded, stream_or_own(ctx, stream));
}

int wgt_occluded_rays(wgt_ctx* ctx, const float* rays, const float* max_dist, uint32_t n, uint8_t* occluded) {
  WGT_BEGIN(query_begin(ctx, n, null_buffer(!rays || !max_dist || !occluded)));
  const float *d_rays, *d_limit;
  uint8_t* d_out;
  int rc;
  if ((rc = scratch(ctx, wgt_ctx::kOccOut, n, d_out))) return rc;
  if ((rc = stage(ctx, wgt_ctx::kRays, rays, (size_t)n * 24, d_rays))) return rc;
  if ((rc = stage(ctx, wgt_ctx::kOccLimit, max_dist, (size_t)n * 4, d_limit))) return rc;
  if ((rc = occluded_launch(ctx, d_rays, d_limit, n, d_out, ctx->stream))) return rc;
  if ((rc = fetch(ctx, occluded, d_out, n))) return rc;
  return sync_stream(ctx);
}

int wgt_trace_hits_async(wgt_ctx* ctx, const float* d_rays, uint32_t n, const wgt_hit_buffers* d_out, void* stream) {
  WGT_BEGIN(query_begin(ctx, n, !d_rays ? "null buffer" : bad_hits(d_out)));
  return hits_launch(ctx, d_rays, n, *d_out, stream_or_own(ctx, stream));
}

int wgt_trace_hits(wgt_ctx* ctx, const float* rays, uint32_t n, const wgt_hit_buffers* out) {
  WGT_BEGIN(query_begin(ctx, n, !rays ? "null buffer" : bad_hits(out)));
  return trace_hits_sync(ctx, rays, n, *out);
}

int wgt_nearest_points_async(wgt_ctx* ctx, const float* d_points, const float* d_max_dist, uint32_t n,
                             const wgt_nearest_buffers* d_out, void* stream) {
  WGT_BEGIN(query_begin(ctx, n, check_nearest_args(d_points, d_out, n)));
  return nearest_launch(ctx, d_points, d_max_dist, n, *d_out, nullptr, stream_or_own(ctx, stream));
}

int wgt_nearest_points(wgt_ctx* ctx, const float* points, const float* max_dist, uint32_t n,
                       const wgt_nearest_buffers* out) {
  WGT_BEGIN(query_begin(ctx, n, check_nearest_args(points, out, n)));
  const NearestStage st = plan_nearest_stage(*out, max_dist != nullptr, n);
  wgt_nearest_buffers dev{};
  const float *d_points, *d_limit = nullptr;
  float* d_vec = nullptr;
  int rc;
  if (st.prim && (rc = scratch(ctx, wgt_ctx::kPrim, st.prim, dev.prim))) return rc;
  if (st.dist && (rc = scratch(ctx, wgt_ctx::kDist, st.dist, dev.dist))) return rc;
  if (st.vec && (rc = scratch(ctx, wgt_ctx::kHitVec, st.vec, d_vec))) return rc;
  if (out->pos) dev.pos = d_vec;
  if (out->uv) dev.uv = d_vec + st.uv_at;
  if ((rc = stage(ctx, wgt_ctx::kRays, points, st.points, d_points))) return rc;
  if (max_dist && (rc = stage(ctx, wgt_ctx::kOccLimit, max_dist, st.limits, d_limit))) return rc;
  if ((rc = nearest_launch(ctx, d_points, d_limit, n, dev, nullptr, ctx->stream))) return rc;
  if (out->prim && (rc = fetch(ctx, out->prim, dev.prim, st.prim))) return rc;
  if (out->dist && (rc = fetch(ctx, out->dist, dev.dist, st.dist))) return rc;
  if (out->pos && (rc = fetch(ctx, out->pos, dev.pos, (size_t)n * 12))) return rc;
  if (out->uv && (rc = fetch(ctx, out->uv, dev.uv, (size_t)n * 8))) return rc;
  return sync_stream(ctx);
}

int wgt_nearest_points_stats(wgt_ctx* ctx, const float* d_points, const float* d_max_dist, uint32_t n,
                             const wgt_nearest_buffers* d_out, uint64_t counts[2]) {
  if (counts) counts[0] = counts[1] = 0;  // what n == 0 leaves
  const char* bad = check_nearest_args(d_points, d_out, n);
  WGT_BEGIN(query_begin(ctx, n, bad ? bad : (counts ? nullptr : "null counts")));
  unsigned long long c[2], *d_c;
  int rc;
  if ((rc = scratch(ctx, wgt_ctx::kCounters, sizeof c, d_c))) return rc;
  WGT_HIP(ctx, hipMemsetAsync(d_c, 0, sizeof c, ctx->stream));
  if ((rc = nearest_launch(ctx, d_points, d_max_dist, n, *d_out, d_c, ctx->stream))) return rc;
  if ((rc = fetch(ctx, c, d_c, sizeof c)) || (rc = sync_stream(ctx))) return rc;
  counts[0] = c[0];
  counts[1] = c[1];
  return WGT_OK;
}

int wgt_nearest_points_spec(const wgt_triangle* tris, uint32_t n_tris, uint32_t first_prim, const float* points,
                            const float* max_dist, uint32_t n, const wgt_nearest_buffers* out) {
  if (n == 0) return WGT_OK;
  if (n_tris > 0 && !tris) return fail(nullptr, WGT_E_INVALID, "null triangles");
  if (const char* bad = check_nearest_args(points, out, n)) return fail(nullptr, WGT_E_INVALID, bad);
  nearest_points_spec(tris, n_tris, first_prim, points, max_dist, n, *out);
  return WGT_OK;
}

int wgt_nearest_k_points_async(wgt_ctx* ctx, const float* d_points, const float* d_max_dist, uint32_t n, uint32_t k,
                               const wgt_nearest_k_buffers* d_out, void* stream) {
  WGT_BEGIN(query_begin(ctx, n, check_nearest_k_args(d_points, d_out, n, k)));
  return nearest_k_launch(ctx, d_points, d_max_dist, n, k, *d_out, nullptr, stream_or_own(ctx, stream));
}

int wgt_nearest_k_points(wgt_ctx* ctx, const float* points, const float* max_dist, uint32_t n, uint32_t k,
                         const wgt_nearest_k_buffers* out) {
  WGT_BEGIN(query_begin(ctx, n, check_nearest_k_args(points, out, n, k)));
  const NearestKStage st = plan_nearest_k_stage(*out, max_dist != nullptr, n, k);
  wgt_nearest_k_buffers dev{};
  const float *d_points, *d_limit = nullptr;
  float* d_vec = nullptr;
  int rc;
  if (st.count && (rc = scratch(ctx, wgt_ctx::kOut32, st.count, dev.count))) return rc;
  if (st.prim && (rc = scratch(ctx, wgt_ctx::kPrim, st.prim, dev.prim))) return rc;
  if (st.dist && (rc = scratch(ctx, wgt_ctx::kDist, st.dist, dev.dist))) return rc;
  if (st.vec && (rc = scratch(ctx, wgt_ctx::kHitVec, st.vec, d_vec))) return rc;
  if (out->pos) dev.pos = d_vec;
  if (out->uv) dev.uv = d_vec + st.uv_at;
  if ((rc = stage(ctx, wgt_ctx::kRays, points, st.points, d_points))) return rc;
  if (max_dist && (rc = stage(ctx, wgt_ctx::kOccLimit, max_dist, st.limits, d_limit))) return rc;
  if ((rc = nearest_k_launch(ctx, d_points, d_limit, n, k, dev, nullptr, ctx->stream))) return rc;
  if (out->count && (rc = fetch(ctx, out->count, dev.count, st.count))) return rc;
  if (out->prim && (rc = fetch(ctx, out->prim, dev.prim, st.prim))) return rc;
  if (out->dist && (rc = fetch(ctx, out->dist, dev.dist, st.dist))) return rc;
  if (out->pos && (rc = fetch(ctx, out->pos, dev.pos, (size_t)n * k * 12))) return rc;
  if (out->uv && (rc = fetch(ctx, out->uv, dev.uv, (size_t)n * k * 8))) return rc;
  return sync_stream(ctx);
}

int wgt_nearest_k_points_stats(wgt_ctx* ctx, const float* d_points, const float* d_max_dist, uint32_t n, uint32_t k,
                               const wgt_nearest_k_buffers* d_out, uint64_t counts[2]) {
  if (counts) counts[0] = counts[1] = 0;  // what n == 0 leaves
  const char* bad = check_nearest_k_args(d_points, d_out, n, k);
  WGT_BEGIN(query_begin(ctx, n, bad ? bad : (counts ? nullptr : "null counts")));
  unsigned long long c[2], *d_c;
  int rc;
  if ((rc = scratch(ctx, wgt_ctx::kCounters, sizeof c, d_c))) return rc;
  WGT_HIP(ctx, hipMemsetAsync(d_c, 0, sizeof c, ctx->stream));
  if ((rc = nearest_k_launch(ctx, d_points, d_max_dist, n, k, *d_out, d_c, ctx->stream))) return rc;
  if ((rc = fetch(ctx, c, d_c, sizeof c)) || (rc = sync_stream(ctx))) return rc;
  counts[0] = c[0];
  counts[1] = c[1];
  return WGT_OK;
}

int wgt_nearest_k_points_spec(const wgt_triangle* tris, uint32_t n_tris, uint32_t first_prim, const float* points,
                              const float* max_dist, uint32_t n, uint32_t k, const wgt_nearest_k_buffers* out) {
  if (n == 0) return WGT_OK;
  if (n_tris > 0 && !tris) return fail(nullptr, WGT_E_INVALID, "null triangles");
  if (const char* bad = check_nearest_k_args(points, out, n, k)) return fail(nullptr, WGT_E_INVALID, bad);
  nearest_k_points_spec(tris, n_tris, first_prim, points, max_dist, n, k, *out);
  return WGT_OK;
}

int wgt_overlap_triangles_async(wgt_ctx* ctx, const float* d_tris, uint32_t n, uint32_t k,
                                const wgt_overlap_buffers* d_out, void* stream) {
  WGT_BEGIN(query_begin(ctx, n, check_overlap_args(d_tris, d_out, k)));
  return overlap_launch(ctx, d_tris, n, k, *d_out, nullptr, stream_or_own(ctx, stream));
}

int wgt_overlap_triangles(wgt_ctx* ctx, const float* tris, uint32_t n, uint32_t k, const wgt_overlap_buffers* out) {
  WGT_BEGIN(query_begin(ctx, n, check_overlap_args(tris, out, k)));
  const StageLayout lay = stage_overlap(tris, *out, n, k);
  return run_staged(ctx, lay, [&](auto at) {
    const wgt_overlap_buffers dev{(uint8_t*)at(kOvsHit), (uint32_t*)at(kOvsCount), (uint32_t*)at(kOvsPrim)};
    return overlap_launch(ctx, (const float*)at(kOvsQuery), n, k, dev, nullptr, ctx->stream);
  });
}

int wgt_overlap_triangles_stats(wgt_ctx* ctx, const float* d_tris, uint32_t n, uint32_t k,
                                const wgt_overlap_buffers* d_out, uint64_t counts[2]) {
  if (counts) counts[0] = counts[1] = 0;  // what n == 0 leaves
  const char* bad = check_overlap_args(d_tris, d_out, k);
  WGT_BEGIN(query_begin(ctx, n, bad ? bad : (counts ? nullptr : "null counts")));
  unsigned long long c[2], *d_c;
  int rc;
  if ((rc = scratch(ctx, wgt_ctx::kCounters, sizeof c, d_c))) return rc;
  WGT_HIP(ctx, hipMemsetAsync(d_c, 0, sizeof c, ctx->stream));
  if ((rc = overlap_launch(ctx, d_tris, n, k, *d_out, d_c, ctx->stream))) return rc;
  if ((rc = fetch(ctx, c, d_c, sizeof c)) || (rc = sync_stream(ctx))) return rc;
  counts[0] = c[0];
  counts[1] = c[1];
  return WGT_OK;
}

int wgt_overlap_triangles_spec(const wgt_triangle* tris, uint32_t n_tris, uint32_t first_prim, const float* query,
                               uint32_t n, uint32_t k, const wgt_overlap_buffers* out) {
  if (n == 0) return WGT_OK;
  if (n_tris > 0 && !tris) return fail(nullptr, WGT_E_INVALID, "null triangles");
  if (const char* bad = check_overlap_args(query, out, k)) return fail(nullptr, WGT_E_INVALID, bad);
  overlap_triangles_spec(tris, n_tris, first_prim, query, n, k, *out);
  return WGT_OK;
}

int wgt_overlap_self_async(wgt_ctx* ctx, const uint32_t* d_indices, uint32_t k, const wgt_overlap_buffers* d_out,
                           void* stream) {
  WGT_BEGIN(overlap_self_begin(ctx, check_overlap_self_args(d_out, k)));
  return overlap_self_launch(ctx, d_indices, k, *d_out, nullptr, stream_or_own(ctx, stream));
}

int wgt_overlap_self(wgt_ctx* ctx, const uint32_t* indices, uint32_t k, const wgt_overlap_buffers* out) {
  WGT_BEGIN(overlap_self_begin(ctx, check_overlap_self_args(out, k)));
  const StageLayout lay = stage_overlap_self(indices, *out, ctx->sc.n_tris, k);
  return run_staged(ctx, lay, [&](auto at) {
    const wgt_overlap_buffers dev{(uint8_t*)at(kOssHit), (uint32_t*)at(kOssCount), (uint32_t*)at(kOssPrim)};
    return overlap_self_launch(ctx, (const uint32_t*)at(kOssIndex), k, dev, nullptr, ctx->stream);
  });
}

int wgt_overlap_self_stats(wgt_ctx* ctx, const uint32_t* d_indices, uint32_t k, const wgt_overlap_buffers* d_out,
                           uint64_t counts[2]) {
  if (counts) counts[0] = counts[1] = 0;  // what a scene without triangles leaves
  const char* bad = check_overlap_self_args(d_out, k);
  WGT_BEGIN(overlap_self_begin(ctx, bad ? bad : (counts ? nullptr : "null counts")));
  unsigned long long c[2], *d_c;
  int rc;
  if ((rc = scratch(ctx, wgt_ctx::kCounters, sizeof c, d_c))) return rc;
  WGT_HIP(ctx, hipMemsetAsync(d_c, 0, sizeof c, ctx->stream));
  if ((rc = overlap_self_launch(ctx, d_indices, k, *d_out, d_c, ctx->stream))) return rc;
  if ((rc = fetch(ctx, c, d_c, sizeof c)) || (rc = sync_stream(ctx))) return rc;
  counts[0] = c[0];
  counts[1] = c[1];
  return WGT_OK;
}

int wgt_overlap_self_spec(const wgt_triangle* tris, uint32_t n_tris, uint32_t first_prim, const uint32_t* indices,
                          uint32_t k, const wgt_overlap_buffers* out) {
  if (n_tris == 0) return WGT_OK;
  if (!tris) return fail(nullptr, WGT_E_INVALID, "null triangles");
  if (const char* bad = check_overlap_self_args(out, k)) return fail(nullptr, WGT_E_INVALID, bad);
  overlap_self_spec(tris, n_tris, first_prim, indices, k, *out);
  return WGT_OK;
}

int wgt_trace_radiance_async(wgt_ctx* ctx, const float* d_rays, const uint32_t* d_seeds, uint32_t seed0,
                             uint32_t samples, uint32_t n, const wgt_radiance_buffers* d_out, void* stream) {
  WGT_BEGIN(query_begin(ctx, n, check_radiance_args(d_rays, d_out, samples)));
  return radiance_launch(ctx, d_rays, d_seeds, seed0, samples, n, *d_out, nullptr, stream_or_own(ctx, stream));
}

int wgt_trace_radiance(wgt_ctx* ctx, const float* rays, const uint32_t* seeds, uint32_t seed0, uint32_t samples,
                       uint32_t n, const wgt_radiance_buffers* out) {
  WGT_BEGIN(query_begin(ctx, n, check_radiance_args(rays, out, samples)));
  const RadianceStage st = plan_radiance_stage(*out, seeds != nullptr, n);
  wgt_radiance_buffers dev{};
  const float* d_rays;
  const uint32_t* d_seeds = nullptr;
  int rc;
  if (st.rgb && (rc = scratch(ctx, wgt_ctx::kHitVec, st.rgb, dev.rgb))) return rc;
  if (st.prim && (rc = scratch(ctx, wgt_ctx::kPrim, st.prim, dev.prim))) return rc;
  if (st.seed_out && (rc = scratch(ctx, wgt_ctx::kRadSeedOut, st.seed_out, dev.seed_out))) return rc;
  if ((rc = stage(ctx, wgt_ctx::kRays, rays, st.rays, d_rays))) return rc;
  if (seeds && (rc = stage(ctx, wgt_ctx::kRadSeeds, seeds, st.seeds, d_seeds))) return rc;
  if ((rc = radiance_launch(ctx, d_rays, d_seeds, seed0, samples, n, dev, nullptr, ctx->stream))) return rc;
  if (out->rgb && (rc = fetch(ctx, out->rgb, dev.rgb, st.rgb))) return rc;
  if (out->prim && (rc = fetch(ctx, out->prim, dev.prim, st.prim))) return rc;
  if (out->seed_out && (rc = fetch(ctx, out->seed_out, dev.seed_out, st.seed_out))) return rc;
  return sync_stream(ctx);
}

int wgt_trace_radiance_stats(wgt_ctx* ctx, const float* d_rays, const uint32_t* d_seeds, uint32_t seed0,
                             uint32_t samples, uint32_t n, const wgt_radiance_buffers* d_out, uint64_t counts[4]) {
  if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;  // what n == 0 leaves
  const char* bad = check_radiance_args(d_rays, d_out, samples);
  WGT_BEGIN(query_begin(ctx, n, bad ? bad : (counts ? nullptr : "null counts")));
  unsigned long long c[4], *d_c;
  int rc;
  if ((rc = scratch(ctx, wgt_ctx::kCounters, sizeof c, d_c))) return rc;
  WGT_HIP(ctx, hipMemsetAsync(d_c, 0, sizeof c, ctx->stream));
  if ((rc = radiance_launch(ctx, d_rays, d_seeds, seed0, samples, n, *d_out, d_c, ctx->stream))) return rc;
  if ((rc = fetch(ctx, c, d_c, sizeof c)) || (rc = sync_stream(ctx))) return rc;
  for (int k = 0; k < 4; ++k) counts[k] = c[k];
  return WGT_OK;
}

int wgt_trace_multi_hits_async(wgt_ctx* ctx, const float* d_rays, const float* d_max_dist, uint32_t n, uint32_t k,
                               uint32_t flags, const wgt_multi_hit_buffers* d_out, void* stream) {
  WGT_BEGIN(query_begin(ctx, n, check_multi_hit_args(d_rays, d_out, k, flags)));
  return multi_hit_launch(ctx, d_rays, d_max_dist, n, k, flags, *d_out, nullptr, stream_or_own(ctx, stream));
}

int wgt_trace_multi_hits(wgt_ctx* ctx, const float* rays, const float* max_dist, uint32_t n, uint32_t k,
                         uint32_t flags, const wgt_multi_hit_buffers* out) {
  WGT_BEGIN(query_begin(ctx, n, check_multi_hit_args(rays, out, k, flags)));
  const MultiHitStage st = plan_multi_hit_stage(*out, max_dist != nullptr, n, k);
  wgt_multi_hit_buffers dev{};
  const float *d_rays, *d_limit = nullptr;
  int rc;
  if (st.count && (rc = scratch(ctx, wgt_ctx::kOut32, st.count, dev.count))) return rc;
  if (st.prim && (rc = scratch(ctx, wgt_ctx::kPrim, st.prim, dev.prim))) return rc;
  if (st.dist && (rc = scratch(ctx, wgt_ctx::kDist, st.dist, dev.dist))) return rc;
  if ((rc = stage(ctx, wgt_ctx::kRays, rays, st.rays, d_rays))) return rc;
  if (max_dist && (rc = stage(ctx, wgt_ctx::kOccLimit, max_dist, st.limits, d_limit))) return rc;
  if ((rc = multi_hit_launch(ctx, d_rays, d_limit, n, k, flags, dev, nullptr, ctx->stream))) return rc;
  if (out->count && (rc = fetch(ctx, out->count, dev.count, st.count))) return rc;
  if (out->prim && (rc = fetch(ctx, out->prim, dev.prim, st.prim))) return rc;
  if (out->dist && (rc = fetch(ctx, out->dist, dev.dist, st.dist))) return rc;
  return sync_stream(ctx);
}

int wgt_trace_multi_hits_stats(wgt_ctx* ctx, const float* d_rays, const float* d_max_dist, uint32_t n, uint32_t k,
                               uint32_t flags, const wgt_multi_hit_buffers* d_out, uint64_t counts[2]) {
  if (counts) counts[0] = counts[1] = 0;  // what n == 0 leaves
  const char* bad = check_multi_hit_args(d_rays, d_out, k, flags);
  WGT_BEGIN(query_begin(ctx, n, bad ? bad : (counts ? nullptr : "null counts")));
  unsigned long long c[2], *d_c;
  int rc;
  if ((rc = scratch(ctx, wgt_ctx::kCounters, sizeof c, d_c))) return rc;
  WGT_HIP(ctx, hipMemsetAsync(d_c, 0, sizeof c, ctx->stream));
  if ((rc = multi_hit_launch(ctx, d_rays, d_max_dist, n, k, flags, *d_out, d_c, ctx->stream))) return rc;
  if ((rc = fetch(ctx, c, d_c, sizeof c)) || (rc = sync_stream(ctx))) return rc;
  counts[0] = c[0];
  counts[1] = c[1];
  return WGT_OK;
}

int wgt_render_gbuffer_async(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H, uint32_t tw,
                             uint32_t th, const wgt_tile* d_tiles, uint32_t n_tiles, const wgt_hit_buffers* d_out,
                             float* d_rays, void* stream) {
  WGT_BEGIN(tiles_begin(ctx, cam, W, H, tw, th, d_tiles, n_tiles, false, nullptr, bad_hits(d_out)));
  const DevFrame fr = tile_frame(*cam, W, H, tw, th, n_tiles);
  return gbuffer_launch(ctx, fr, SampleArgs{}, d_tiles, *d_out, d_rays, stream_or_own(ctx, stream));
}

int wgt_render_gbuffer_sampled_async(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H, uint32_t tw,
                                     uint32_t th, const wgt_tile* d_tiles, uint32_t n_tiles, const uint8_t* d_sample_map,
                                     const wgt_hit_buffers* d_out, float* d_rays, void* stream) {
  wgt_camera_param c1;
  cam = sampled_cam(cam, c1);
  const char* bad = bad_hits(d_out);
  if (!bad) bad = check_sample_map(d_sample_map);
  WGT_BEGIN(tiles_begin(ctx, cam, W, H, tw, th, d_tiles, n_tiles, false, nullptr, bad));
  const DevFrame fr = tile_frame(*cam, W, H, tw, th, n_tiles);
  return gbuffer_launch(ctx, fr, sample_args(ctx, d_sample_map), d_tiles, *d_out, d_rays, stream_or_own(ctx, stream));
}

}  // extern "C"

namespace {

// wgt_render_gbuffer, and with a host sample map (sampled) wgt_render_gbuffer_sampled, as render_tile.
int render_gbuffer(wgt_ctx* ctx, const wgt_camera_param* cam_in, uint32_t W, uint32_t H, uint32_t x0, uint32_t y0,
                   uint32_t tw, uint32_t th, bool sampled, const uint8_t* sample_map, const wgt_hit_buffers* out,
                   float* rays_out) {
  wgt_camera_param c1;
  const wgt_camera_param* cam = sampled ? sampled_cam(cam_in, c1) : cam_in;
  int rc = check_render_args(ctx, cam, W, H, tw, th);
  if (rc) return rc;
  if (const char* bad = bad_hits(out)) return fail(ctx, WGT_E_INVALID, bad);
  if (x0 >= W || y0 >= H) return fail(ctx, WGT_E_INVALID, "tile origin outside the frame");
  if (sampled)
    if (const char* bad = check_sample_map(sample_map)) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  const size_t npx = (size_t)tw * th;
  const wgt_tile tile{x0, y0, cam->seed, 0u};
  wgt_hit_buffers dev;
  const wgt_tile* d_tile;
  float* d_rays = nullptr;
  SampleArgs sm{};
  if (sampled) {
    const uint8_t* d_map;
    if ((rc = stage(ctx, wgt_ctx::kSampleMap, sample_map, (size_t)W * H, d_map))) return rc;
    sm = sample_args(ctx, d_map);
  }
  if ((rc = stage_hits(ctx, *out, npx, dev))) return rc;
  if (rays_out && (rc = scratch(ctx, wgt_ctx::kGbRays, npx * 24, d_rays))) return rc;
  if ((rc = stage(ctx, wgt_ctx::kTiles, &tile, sizeof tile, d_tile))) return rc;
  // pixels of a partially covered tile outside the frame are not written by the kernel
  if (x0 + (uint64_t)tw > W || y0 + (uint64_t)th > H) {
    if ((rc = clear_hits(ctx, dev, npx))) return rc;
    if (d_rays) WGT_HIP(ctx, hipMemsetAsync(d_rays, 0, npx * 24, ctx->stream));
  }
  const DevFrame fr = tile_frame(*cam, W, H, tw, th, 1);
  if ((rc = gbuffer_launch(ctx, fr, sm, d_tile, dev, d_rays, ctx->stream))) return rc;
  if ((rc = fetch_hits(ctx, *out, dev, npx))) return rc;
  if (d_rays && (rc = fetch(ctx, rays_out, d_rays, npx * 24))) return rc;
  return sync_stream(ctx);
}

}  // namespace

extern "C" {

int wgt_render_gbuffer(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H, uint32_t x0, uint32_t y0,
                       uint32_t tw, uint32_t th, const wgt_hit_buffers* out, float* rays_out) {
  return render_gbuffer(ctx, cam, W, H, x0, y0, tw, th, false, nullptr, out, rays_out);
}

int wgt_render_gbuffer_sampled(wgt_ctx* ctx, const wgt_camera_param* cam, uint32_t W, uint32_t H, uint32_t x0,
                               uint32_t y0, uint32_t tw, uint32_t th, const uint8_t* sample_map,
                               const wgt_hit_buffers* out, float* rays_out) {
  return render_gbuffer(ctx, cam, W, H, x0, y0, tw, th, true, sample_map, out, rays_out);
}

int wgt_sample_plan_defaults(wgt_sample_plan_params* out) {
  if (!out) return fail(nullptr, WGT_E_INVALID, "null params");
  *out = sample_plan_defaults();
  return WGT_OK;
}

size_t wgt_sample_plan_workspace_bytes(uint32_t W, uint32_t H) { return sample_plan_workspace_bytes(W, H); }

int wgt_sample_plan_async(wgt_ctx* ctx, const wgt_sample_plan_params* params, uint32_t W, uint32_t H,
                          const wgt_temporal_state* d_state, void* d_workspace, size_t workspace_bytes,
                          uint8_t* d_map_out, uint64_t* d_total_out, void* stream) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  std::string bad = check_sample_plan_args(params, W, H, d_state, d_map_out);
  if (bad.empty()) bad = check_sample_plan_workspace(d_workspace, workspace_bytes, W, H);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  const SamplePlan plan = plan_sample_plan(params ? *params : sample_plan_defaults(), W, H);
  // no scene is read: the launches are ordered by the stream alone
  WGT_HIP(ctx, launch_sample_plan(plan, d_state->len, d_state->moments, d_workspace, d_map_out,
                                  (unsigned long long*)d_total_out, stream_or_own(ctx, stream)));
  return WGT_OK;
}

int wgt_sample_plan(wgt_ctx* ctx, const wgt_sample_plan_params* params, uint32_t W, uint32_t H,
                    const wgt_temporal_state* state, uint8_t* map_out, uint64_t* total_out) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  const std::string bad = check_sample_plan_args(params, W, H, state, map_out);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  const StageLayout lay = stage_sample_plan(W, H, *state, map_out, total_out);
  return run_staged(ctx, lay, [&](auto at) {
    const wgt_temporal_state dst{nullptr, (float*)at(kSpsLen), (float*)at(kSpsMom)};
    return wgt_sample_plan_async(ctx, params, W, H, &dst, at(kSpsWs), lay.part[kSpsWs].bytes, (uint8_t*)at(kSpsMap),
                                 (uint64_t*)at(kSpsTotal), ctx->stream);
  });
}

int wgt_denoise_defaults(wgt_denoise_params* out) {
  if (!out) return fail(nullptr, WGT_E_INVALID, "null params");
  *out = denoise_defaults();
  return WGT_OK;
}

size_t wgt_denoise_workspace_bytes(uint32_t W, uint32_t H) { return denoise_workspace_bytes(W, H); }

int wgt_denoise_async(wgt_ctx* ctx, const wgt_denoise_params* params, uint32_t W, uint32_t H, const float* d_rgba32f_in,
                      const wgt_hit_buffers* d_guides, void* d_workspace, size_t workspace_bytes, float* d_rgba32f_out,
                      void* d_rgba8_out, void* stream) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  std::string bad = check_denoise_args(params, W, H, d_rgba32f_in, d_guides, d_rgba32f_out, d_rgba8_out);
  if (bad.empty()) bad = check_denoise_workspace(d_workspace, workspace_bytes, W, H);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  const DenoisePlan plan = plan_denoise(params ? *params : denoise_defaults(), W, H);
  // no scene is read: the launches are ordered by the stream alone
  WGT_HIP(ctx, launch_denoise(plan, (const float4*)d_rgba32f_in, *d_guides, d_workspace, (float4*)d_rgba32f_out,
                              (uchar4*)d_rgba8_out, stream_or_own(ctx, stream)));
  return WGT_OK;
}

int wgt_denoise(wgt_ctx* ctx, const wgt_denoise_params* params, uint32_t W, uint32_t H, const float* rgba32f_in,
                const wgt_hit_buffers* guides, float* rgba32f_out, uint8_t* rgba8_out) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  const std::string bad = check_denoise_args(params, W, H, rgba32f_in, guides, rgba32f_out, rgba8_out);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  const StageLayout lay = stage_denoise(W, H, rgba32f_in, *guides, rgba32f_out, rgba8_out);
  return run_staged(ctx, lay, [&](auto at) {
    const wgt_hit_buffers dev{(uint32_t*)at(kDnsPrim), nullptr, (float*)at(kDnsPos), (float*)at(kDnsNorm),
                              (float*)at(kDnsCol), (uint8_t*)at(kDnsFlags)};
    float* const d_img = (float*)at(kDnsIn);  // filtered in place
    return wgt_denoise_async(ctx, params, W, H, d_img, &dev, at(kDnsWs), lay.part[kDnsWs].bytes,
                             rgba32f_out ? d_img : nullptr, at(kDnsOut8), ctx->stream);
  });
}

int wgt_temporal_defaults(wgt_temporal_params* out) {
  if (!out) return fail(nullptr, WGT_E_INVALID, "null params");
  *out = temporal_defaults();
  return WGT_OK;
}

}  // extern "C"

namespace {

// The two forms of the accumulation share everything but one check and the motion buffers:
// motion_form = wgt_temporal_accumulate_motion (motion is then looked at when there is a previous frame).
int temporal_async(wgt_ctx* ctx, const wgt_temporal_params* params, uint32_t W, uint32_t H, const wgt_camera_param* cam,
                   const wgt_camera_param* cam_prev, const float* d_rgba32f_in, const wgt_hit_buffers* d_guides,
                   bool motion_form, const wgt_motion_buffers* d_motion, const wgt_temporal_state* d_prev,
                   const wgt_hit_buffers* d_guides_prev, const wgt_temporal_state* d_out, void* d_rgba8_out,
                   void* stream) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  const std::string bad =
      motion_form ? check_temporal_motion_args(params, W, H, cam, cam_prev, d_rgba32f_in, d_guides, d_motion, d_prev,
                                               d_guides_prev, d_out)
                  : check_temporal_args(params, W, H, cam, cam_prev, d_rgba32f_in, d_guides, d_prev, d_guides_prev, d_out);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  const TemporalPlan plan = plan_temporal(params ? *params : temporal_defaults(), W, H, *cam, cam_prev);
  // no scene is read: the launch is ordered by the stream alone
  WGT_HIP(ctx, launch_temporal(plan, (const float4*)d_rgba32f_in, *d_guides, motion_form && !plan.first ? d_motion : nullptr,
                               d_prev, d_guides_prev, *d_out, (uchar4*)d_rgba8_out, stream_or_own(ctx, stream)));
  return WGT_OK;
}

int temporal_sync(wgt_ctx* ctx, const wgt_temporal_params* params, uint32_t W, uint32_t H, const wgt_camera_param* cam,
                  const wgt_camera_param* cam_prev, const float* rgba32f_in, const wgt_hit_buffers* guides,
                  bool motion_form, const wgt_motion_buffers* motion, const wgt_temporal_state* prev,
                  const wgt_hit_buffers* guides_prev, const wgt_temporal_state* out, uint8_t* rgba8_out) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  const std::string bad =
      motion_form ? check_temporal_motion_args(params, W, H, cam, cam_prev, rgba32f_in, guides, motion, prev, guides_prev, out)
                  : check_temporal_args(params, W, H, cam, cam_prev, rgba32f_in, guides, prev, guides_prev, out);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  const bool first = !prev, mot = motion_form && !first;
  const StageLayout lay = stage_temporal(W, H, rgba32f_in, *guides, mot ? motion : nullptr, prev, guides_prev, *out, rgba8_out);
  return run_staged(ctx, lay, [&](auto at) {
    const wgt_hit_buffers dg{(uint32_t*)at(kTpsPrim), nullptr, (float*)at(kTpsPos), (float*)at(kTpsNorm), nullptr,
                             (uint8_t*)at(kTpsFlags)};
    const wgt_hit_buffers dgp{(uint32_t*)at(kTpsPPrim), nullptr, (float*)at(kTpsPPos), (float*)at(kTpsPNorm), nullptr,
                              (uint8_t*)at(kTpsPFlags)};
    const wgt_motion_buffers dmot{(float*)at(kTpsMPos), (float*)at(kTpsMNorm)};
    const wgt_temporal_state dprev{(float*)at(kTpsPrevRgba), (float*)at(kTpsPrevLen), (float*)at(kTpsPrevMom)};
    const wgt_temporal_state dout{(float*)at(kTpsIn), (float*)at(kTpsLen), (float*)at(kTpsMom)};  // accumulated in place
    return temporal_async(ctx, params, W, H, cam, cam_prev, dout.rgba32f, &dg, motion_form, mot ? &dmot : nullptr,
                          first ? nullptr : &dprev, first ? nullptr : &dgp, &dout, at(kTpsOut8), ctx->stream);
  });
}

// The reproject's launch on stream s (behind the calls' checks): a reader of the scene and of the snapshot.
int reproject_launch(wgt_ctx* ctx, uint32_t n, const wgt_hit_buffers& dev, const wgt_motion_buffers& out, hipStream_t s) {
  const float4* snap = (const float4*)ctx->motion.p;
  const uint32_t* slot_of = (const uint32_t*)(snap + (size_t)ctx->sc.n_tris * kMotionSnapFloat4s);
  return launch_on(ctx, s, "launch_motion_reproject",
                   [&] { return launch_motion_reproject(ctx->sc, snap, slot_of, n, dev, out, s); });
}
// wgt_motion_reproject's preamble, in the calls' order of checks.
int reproject_begin(wgt_ctx* ctx, uint32_t n, const wgt_hit_buffers* guides, const wgt_motion_buffers* out) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (!ctx->has_scene) return fail(ctx, WGT_E_NOSCENE, "no scene uploaded");
  const std::string bad = check_motion_reproject_args(ctx->has_snapshot, n, guides, out);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  return WGT_OK;
}

}  // namespace

extern "C" {

int wgt_temporal_accumulate_async(wgt_ctx* ctx, const wgt_temporal_params* params, uint32_t W, uint32_t H,
                                  const wgt_camera_param* cam, const wgt_camera_param* cam_prev,
                                  const float* d_rgba32f_in, const wgt_hit_buffers* d_guides,
                                  const wgt_temporal_state* d_prev, const wgt_hit_buffers* d_guides_prev,
                                  const wgt_temporal_state* d_out, void* d_rgba8_out, void* stream) {
  return temporal_async(ctx, params, W, H, cam, cam_prev, d_rgba32f_in, d_guides, false, nullptr, d_prev, d_guides_prev,
                        d_out, d_rgba8_out, stream);
}

int wgt_temporal_accumulate(wgt_ctx* ctx, const wgt_temporal_params* params, uint32_t W, uint32_t H,
                            const wgt_camera_param* cam, const wgt_camera_param* cam_prev, const float* rgba32f_in,
                            const wgt_hit_buffers* guides, const wgt_temporal_state* prev,
                            const wgt_hit_buffers* guides_prev, const wgt_temporal_state* out, uint8_t* rgba8_out) {
  return temporal_sync(ctx, params, W, H, cam, cam_prev, rgba32f_in, guides, false, nullptr, prev, guides_prev, out,
                       rgba8_out);
}

int wgt_temporal_accumulate_motion_async(wgt_ctx* ctx, const wgt_temporal_params* params, uint32_t W, uint32_t H,
                                         const wgt_camera_param* cam, const wgt_camera_param* cam_prev,
                                         const float* d_rgba32f_in, const wgt_hit_buffers* d_guides,
                                         const wgt_motion_buffers* d_motion, const wgt_temporal_state* d_prev,
                                         const wgt_hit_buffers* d_guides_prev, const wgt_temporal_state* d_out,
                                         void* d_rgba8_out, void* stream) {
  return temporal_async(ctx, params, W, H, cam, cam_prev, d_rgba32f_in, d_guides, true, d_motion, d_prev, d_guides_prev,
                        d_out, d_rgba8_out, stream);
}

int wgt_temporal_accumulate_motion(wgt_ctx* ctx, const wgt_temporal_params* params, uint32_t W, uint32_t H,
                                   const wgt_camera_param* cam, const wgt_camera_param* cam_prev,
                                   const float* rgba32f_in, const wgt_hit_buffers* guides,
                                   const wgt_motion_buffers* motion, const wgt_temporal_state* prev,
                                   const wgt_hit_buffers* guides_prev, const wgt_temporal_state* out,
                                   uint8_t* rgba8_out) {
  return temporal_sync(ctx, params, W, H, cam, cam_prev, rgba32f_in, guides, true, motion, prev, guides_prev, out,
                       rgba8_out);
}

int wgt_motion_snapshot(wgt_ctx* ctx, void* stream) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (!ctx->has_scene) return fail(ctx, WGT_E_NOSCENE, "no scene uploaded");
  const DevScene& sc = ctx->sc;
  if (sc.n_tris == 0) return fail(ctx, WGT_E_INVALID, "the scene has no triangles, so nothing to snapshot");
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  if (!ctx->motion.p) {  // the first snapshot of this scene; slot_of starts as "no slot" in every word
    if (int rc = ensure(ctx, ctx->motion, (size_t)sc.n_tris * kMotionSnapBytes)) return rc;
    WGT_HIP(ctx, hipMemsetAsync(ctx->motion.p, 0xff, ctx->motion.bytes, ctx->stream));
    if (int rc = sync_stream(ctx)) return rc;
  }
  float4* snap = (float4*)ctx->motion.p;
  uint32_t* slot_of = (uint32_t*)(snap + (size_t)sc.n_tris * kMotionSnapFloat4s);
  hipStream_t s = stream_or_own(ctx, stream);
  if (int rc = launch_on(ctx, s, "launch_motion_snapshot", [&] { return launch_motion_snapshot(sc, snap, slot_of, s); }))
    return rc;
  ctx->has_snapshot = true;
  return WGT_OK;
}

int wgt_motion_snapshot_read(wgt_ctx* ctx, float* out, uint32_t cap_tris) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (!ctx->has_scene) return fail(ctx, WGT_E_NOSCENE, "no scene uploaded");
  if (!ctx->has_snapshot) return fail(ctx, WGT_E_INVALID, "no motion snapshot since the last upload (wgt_motion_snapshot)");
  if (!out) return fail(ctx, WGT_E_INVALID, "null out");
  if (cap_tris < ctx->sc.n_tris) return fail(ctx, WGT_E_INVALID, "triangle capacity too small");
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  if (int rc = use_drain(ctx)) return rc;
  WGT_HIP(ctx, hipMemcpy(out, ctx->motion.p, (size_t)ctx->sc.n_tris * kMotionSnapFloat4s * 16, hipMemcpyDeviceToHost));
  return WGT_OK;
}

int wgt_motion_reproject_async(wgt_ctx* ctx, uint32_t n, const wgt_hit_buffers* d_guides, const wgt_motion_buffers* d_out,
                               void* stream) {
  if (int rc = reproject_begin(ctx, n, d_guides, d_out)) return rc;
  return reproject_launch(ctx, n, *d_guides, *d_out, stream_or_own(ctx, stream));
}

int wgt_motion_reproject(wgt_ctx* ctx, uint32_t n, const wgt_hit_buffers* guides, const wgt_motion_buffers* out) {
  int rc;
  if ((rc = reproject_begin(ctx, n, guides, out))) return rc;
  // staged through the context's scratch, as wgt_trace_hits' records: prim, pos | norm, flags in;
  // pos_prev | norm_prev out
  const size_t N = n;
  wgt_hit_buffers dev{};
  const uint32_t* d_prim;
  const uint8_t* d_flags;
  float *d_vec, *d_out;
  if ((rc = stage(ctx, wgt_ctx::kPrim, guides->prim, N * 4, d_prim))) return rc;
  if ((rc = stage(ctx, wgt_ctx::kHitFlags, guides->flags, N, d_flags))) return rc;
  if ((rc = scratch(ctx, wgt_ctx::kHitVec, N * 24, d_vec))) return rc;
  if ((rc = scratch(ctx, wgt_ctx::kMotionOut, N * 24, d_out))) return rc;
  WGT_HIP(ctx, hipMemcpyAsync(d_vec, guides->pos, N * 12, hipMemcpyHostToDevice, ctx->stream));
  WGT_HIP(ctx, hipMemcpyAsync(d_vec + 3 * N, guides->norm, N * 12, hipMemcpyHostToDevice, ctx->stream));
  dev.prim = const_cast<uint32_t*>(d_prim);
  dev.flags = const_cast<uint8_t*>(d_flags);
  dev.pos = d_vec;
  dev.norm = d_vec + 3 * N;
  const wgt_motion_buffers dout{d_out, d_out + 3 * N};
  if ((rc = reproject_launch(ctx, n, dev, dout, ctx->stream))) return rc;
  if ((rc = fetch(ctx, out->pos_prev, dout.pos_prev, N * 12))) return rc;
  if ((rc = fetch(ctx, out->norm_prev, dout.norm_prev, N * 12))) return rc;
  return sync_stream(ctx);
}

int wgt_denoise_variance_defaults(wgt_denoise_variance_params* out) {
  if (!out) return fail(nullptr, WGT_E_INVALID, "null params");
  *out = denoise_variance_defaults();
  return WGT_OK;
}

size_t wgt_denoise_variance_workspace_bytes(uint32_t W, uint32_t H) { return denoise_variance_workspace_bytes(W, H); }

int wgt_denoise_variance_async(wgt_ctx* ctx, const wgt_denoise_variance_params* params, uint32_t W, uint32_t H,
                               const wgt_temporal_state* d_state, const wgt_hit_buffers* d_guides, void* d_workspace,
                               size_t workspace_bytes, float* d_rgba32f_out, void* d_rgba8_out, float* d_variance_out,
                               void* stream) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  std::string bad = check_denoise_variance_args(params, W, H, d_state, d_guides, d_rgba32f_out, d_rgba8_out);
  if (bad.empty()) bad = check_denoise_variance_workspace(d_workspace, workspace_bytes, W, H);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  const DenoiseVariancePlan plan = plan_denoise_variance(params ? *params : denoise_variance_defaults(), W, H);
  // no scene is read: the launches are ordered by the stream alone
  WGT_HIP(ctx, launch_denoise_variance(plan, *d_state, *d_guides, d_workspace, (float4*)d_rgba32f_out,
                                       (uchar4*)d_rgba8_out, d_variance_out, stream_or_own(ctx, stream)));
  return WGT_OK;
}

int wgt_denoise_variance(wgt_ctx* ctx, const wgt_denoise_variance_params* params, uint32_t W, uint32_t H,
                         const wgt_temporal_state* state, const wgt_hit_buffers* guides, float* rgba32f_out,
                         uint8_t* rgba8_out, float* variance_out) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  const std::string bad = check_denoise_variance_args(params, W, H, state, guides, rgba32f_out, rgba8_out);
  if (!bad.empty()) return fail(ctx, WGT_E_INVALID, bad);
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  const StageLayout lay = stage_denoise_variance(W, H, *state, *guides, rgba32f_out, rgba8_out, variance_out);
  return run_staged(ctx, lay, [&](auto at) {
    const wgt_hit_buffers dg{(uint32_t*)at(kDvsPrim), nullptr, (float*)at(kDvsPos), (float*)at(kDvsNorm),
                             (float*)at(kDvsCol), (uint8_t*)at(kDvsFlags)};
    const wgt_temporal_state dst{(float*)at(kDvsIn), (float*)at(kDvsLen), (float*)at(kDvsMom)};  // filtered in place
    return wgt_denoise_variance_async(ctx, params, W, H, &dst, &dg, at(kDvsWs), lay.part[kDvsWs].bytes,
                                      rgba32f_out ? dst.rgba32f : nullptr, at(kDvsOut8), (float*)at(kDvsVar), ctx->stream);
  });
}

int wgt_selftest_math(wgt_ctx* ctx, uint32_t n, uint32_t seed, uint64_t counts[8]) {
  if (!ctx) return fail(nullptr, WGT_E_INVALID, "null context");
  if (!counts) return fail(ctx, WGT_E_INVALID, "null counts");
  WGT_HIP(ctx, hipSetDevice(ctx->device));
  int rc;
  unsigned long long* d_counts;
  if ((rc = scratch(ctx, wgt_ctx::kPrim, 64, d_counts))) return rc;
  WGT_HIP(ctx, hipMemsetAsync(d_counts, 0, 64, ctx->stream));
  WGT_HIP(ctx, launch_selftest_math(n, seed, d_counts, ctx->stream));
  if ((rc = fetch(ctx, counts, d_counts, 64)) || (rc = sync_stream(ctx))) return rc;
  counts[0] = 1ull << 32;  // sqrt: every bit pattern
  // n quad-distance quotients, n Moller-Trumbore reciprocals, and every pattern 2^-87 <= |x| <= 2^34
  // of the traversal's reciprocal
  uint32_t lo, hi;
  const float flo = kSlabDirMin, fhi = 0x1p34f;
  std::memcpy(&lo, &flo, 4);
  std::memcpy(&hi, &fhi, 4);
  counts[2] = 2ull * n + 2ull * (hi - lo + 1u);
  return WGT_OK;
}

}  // extern "C"
