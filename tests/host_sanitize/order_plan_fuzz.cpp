// order_plan_fuzz.cpp — the planner of the pixel queue's order across launches (launch_plan.h
// OrderPlanner, order_key, order_eligible) under AddressSanitizer + UBSan (CPU only; built and run by
// tests/test_order_sanitize.py).  It drives the planner alone with seeded random sequences of
// launches over a handful of views, scene changes, resets and completions; whether a workspace slot's
// last launch has ended is this program's own answer.  A model of the device keeps, per shared
// buffer, the view whose order it holds and the launches still reading it.  Exits non-zero on a
// failed invariant; the sanitizers abort on the first finding.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/wgt_api.h"
#include "../../webgputracer_amd/csrc/host/launch_plan.h"

using namespace wgt;

static int g_fail = 0;
static unsigned long long g_today = 0, g_refine = 0, g_reuse = 0, g_refused = 0;  // over all runs
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                          \
    }                                                                    \
  } while (0)

// A view of the test: camera, frame, tiles and spp.
struct View {
  float ox;
  uint32_t W, H, tw, th, n_tiles, spp;
  uint64_t tiles;
  bool by_ptr;
};
static const View kViews[] = {
    {278.0f, 52, 28, 52, 28, 1, 16, 11, false},   {278.0f, 52, 28, 52, 28, 1, 4, 11, false},
    {278.0f, 52, 28, 52, 28, 1, 1, 11, false},    {279.0f, 52, 28, 52, 28, 1, 16, 11, false},
    {278.0f, 64, 48, 16, 16, 12, 16, 0x7000, true}, {278.0f, 64, 48, 16, 16, 12, 16, 0x7100, true},
    {278.0f, 64, 48, 16, 16, 6, 16, 0x7000, true},  {278.0f, 53, 28, 53, 28, 1, 16, 11, false},
    {278.0f, 52, 28, 26, 28, 2, 256, 11, false},  {278.0f, 52, 28, 52, 28, 1, 16, 11, true},
};
constexpr int kNViews = sizeof kViews / sizeof *kViews;

static DevFrame frame_of(const View& v) {
  const wgt_camera_param cam{{v.ox, 278.0f, -800.0f}, 0.0f, {278.0f, 278.0f, 0.0f}, 0.0f, (float)v.W / (float)v.H, 40.0f, v.spp, 0u};
  return tile_frame(cam, v.W, v.H, v.tw, v.th, v.n_tiles);
}

struct Launch {
  int slot, buf;  // buf: the shared buffer it reads, -1 for none
  bool done;
};

static void set_knob(const char* name, uint32_t v) { setenv(name, std::to_string(v).c_str(), 1); }

static void run(uint32_t seed) {
  std::mt19937 g(seed);
  OrderPlanner pl;
  std::vector<Launch> launches;
  bool busy[OrderPlanner::kSlots] = {};  // the slot's last launch has not ended
  // the model's buffers: the key whose order each holds
  bool held[kOrderBufs] = {};
  OrderKey held_key[kOrderBufs] = {};
  // the model's expectation of the planner's memory
  bool seen = false, cur = false;
  OrderKey last{}, cur_key{};
  uint64_t n_today = 0, n_refine = 0, n_reuse = 0, n_invalid = 0;
  const uint32_t refines[] = {0, 1, 2, 4, 100}, lpts[] = {1, 1, 1, 0, 2};
  const int n_views = 2 + (int)(g() % (kNViews - 1));  // a handful: runs of one view are likely
  const int n_slots = 1 + (int)(g() % OrderPlanner::kSlots);
  int next_slot = 0, vi = 0;
  set_knob("WGT_PQ_REUSE", 1);
  set_knob("WGT_PQ_REFINE", 2);
  set_knob("WGT_PQ_LPT", 1);
  set_knob("WGT_KERNEL", 2);
  for (int step = 0; step < 400; ++step) {
    const uint32_t what = g() % 100;
    if (what < 4) {  // a scene change (upload, refit, rebuild) or a reset: after every launch has ended or not
      pl.invalidate();
      n_invalid += cur ? 1 : 0;
      cur = seen = false;
      continue;
    }
    if (what < 24) {  // a slot's launches end (they are serialised: all of them)
      const int s = (int)(g() % OrderPlanner::kSlots);
      busy[s] = false;
      for (Launch& l : launches)
        if (l.slot == s) l.done = true;
      continue;
    }
    if (what < 28) {  // knobs change between launches
      set_knob("WGT_PQ_REUSE", g() % 4 ? 1 : 0);
      set_knob("WGT_PQ_REFINE", refines[g() % 5]);
      set_knob("WGT_PQ_LPT", lpts[g() % 5]);
      set_knob("WGT_KERNEL", g() % 8 ? 2 : 1);
      continue;
    }
    // a launch: mostly the view of the launch before
    if (g() % 3 == 0) vi = (int)(g() % n_views);
    const View& v = kViews[vi];
    const bool sampled = g() % 16 == 0;
    const DevFrame fr = frame_of(v);
    const OrderKnobs knobs = order_knobs();
    const uint32_t nb = order_blocks(fr);
    CHECK(nb == ((v.tw + 7) / 8) * ((v.th + 7) / 8) * v.n_tiles);
    const bool eligible = order_eligible(fr, knobs, sampled, nb);
    CHECK(eligible == (knobs.reuse != 0 && !sampled && fr.kernel == 2 && fr.pq_lpt != 0 && fr.sqrt_spp > fr.pq_lpt));
    const OrderKey key = order_key(fr, nb, knobs, pl.epoch(), v.tiles, v.by_ptr);
    CHECK(same_view(key, key));
    const int slot = next_slot;
    next_slot = (next_slot + 1) % n_slots;
    // the runtime's question before it plans: would this launch write a shared buffer if one is free?
    const bool due = pl.refine_due(key, eligible);
    CHECK(due == (eligible && !(cur && same_view(key, cur_key)) && seen && same_view(key, last)));
    if (due && g() % 8 == 0) {
      // the buffers grow for it: every launch has ended, no order is kept, the sighting still counts
      for (Launch& l : launches) l.done = true;
      for (bool& b : busy) b = false;
      pl.buffers_reset();
      n_invalid += cur ? 1 : 0;
      cur = false;
      held[0] = held[1] = false;
      CHECK(pl.current() == -1 && pl.readers(0) == 0u && pl.readers(1) == 0u && pl.refine_due(key, eligible));
    }
    const OrderPlan p = pl.plan(key, eligible, slot, [&](int s) { return !busy[s]; });
    if (p.mode == kOrderRefine) CHECK(due);

    // what may read or write a shared buffer at all
    if (!eligible) CHECK(p.mode == kOrderToday);
    if (p.mode == kOrderToday) CHECK(p.buf == -1 && p.side == fr.pq_lpt);
    else CHECK(p.buf >= 0 && p.buf < kOrderBufs);
    // the model's expectation
    const bool is_cur = eligible && cur && same_view(key, cur_key);
    const bool second = eligible && !is_cur && seen && same_view(key, last);
    if (is_cur) CHECK(p.mode == kOrderReuse);
    if (eligible && !is_cur && !second) CHECK(p.mode == kOrderToday);  // a first sighting
    if (p.mode == kOrderRefine) CHECK(second);
    if (p.mode == kOrderReuse) {
      CHECK(is_cur && p.side == 0u && held[p.buf] && same_view(held_key[p.buf], key));
      // never a buffer of another geometry
      const OrderKey& h = held_key[p.buf];
      CHECK(h.nb == nb && h.fr.tw == fr.tw && h.fr.th == fr.th && h.fr.n_tiles == fr.n_tiles && h.fr.W == fr.W &&
            h.fr.H == fr.H && h.epoch == pl.epoch());
      ++n_reuse;
    }
    if (second) {
      // a buffer is free when every launch that read it has ended; with every slot idle one is
      bool any_busy = false;
      for (bool b : busy) any_busy |= b;
      if (!any_busy) CHECK(p.mode == kOrderRefine);
      if (p.mode == kOrderToday) {  // refused: every buffer has a reader slot that has not ended
        ++g_refused;
        for (int b = 0; b < kOrderBufs; ++b) {
          bool blocked = false;
          for (int s = 0; s < OrderPlanner::kSlots; ++s) blocked |= (pl.readers(b) >> s & 1u) && busy[s];
          CHECK(blocked);
        }
      }
    }
    if (p.mode == kOrderRefine) {
      for (const Launch& l : launches) CHECK(l.buf != p.buf || l.done);  // no reader left in flight
      CHECK(p.side >= fr.pq_lpt && p.side <= fr.sqrt_spp - 1u);
      CHECK(p.side == std::min(std::max(knobs.refine, fr.pq_lpt), fr.sqrt_spp - 1u));
      held[p.buf] = true;
      held_key[p.buf] = key;
      cur = true;
      cur_key = key;
      CHECK(pl.current() == p.buf && pl.current_side() == p.side && pl.current_key().nb == nb);
      ++n_refine;
    }
    if (p.mode == kOrderToday) ++n_today;
    if (eligible) {
      seen = true;
      last = key;
    } else {
      seen = false;
    }
    launches.push_back(Launch{slot, p.mode == kOrderToday ? -1 : p.buf, false});
    busy[slot] = true;
    // the planner knows every reader still in flight
    for (const Launch& l : launches)
      if (!l.done && l.buf >= 0) CHECK(pl.readers(l.buf) >> l.slot & 1u);
    if (g() % 64 == 0) {  // a launch that could not be queued
      pl.launch_failed(p);
      if (p.mode == kOrderRefine) {
        ++n_invalid;
        cur = seen = false;
        held[p.buf] = false;
        CHECK(pl.current() == -1);
      }
    }
  }
  uint64_t a, b, c, d;
  pl.counts(a, b, c, d);
  CHECK(a == n_today && b == n_refine && c == n_reuse && d == n_invalid);
  g_today += a;
  g_refine += b;
  g_reuse += c;
}

// One view alone: TODAY, REFINE, REUSE..., and again after a scene change; WGT_PQ_REUSE=0: TODAY only.
static void check_sequence() {
  set_knob("WGT_PQ_REUSE", 1);
  set_knob("WGT_PQ_REFINE", 2);
  set_knob("WGT_PQ_LPT", 1);
  set_knob("WGT_KERNEL", 2);
  OrderPlanner pl;
  auto idle = [](int) { return true; };
  auto never = [](int) { return false; };
  auto go = [&](const View& v, int slot, bool done) {
    const DevFrame fr = frame_of(v);
    const OrderKnobs k = order_knobs();
    const uint32_t nb = order_blocks(fr);
    const OrderKey key = order_key(fr, nb, k, pl.epoch(), v.tiles, v.by_ptr);
    return done ? pl.plan(key, order_eligible(fr, k, false, nb), slot, idle)
                : pl.plan(key, order_eligible(fr, k, false, nb), slot, never);
  };
  CHECK(go(kViews[0], 0, true).mode == kOrderToday);
  OrderPlan p = go(kViews[0], 1, true);
  CHECK(p.mode == kOrderRefine && p.side == 2u && p.buf == 0);
  CHECK(go(kViews[0], 2, true).mode == kOrderReuse);
  CHECK(go(kViews[0], 3, true).mode == kOrderReuse);
  // another view, twice, while the readers of buffer 0 are in flight: the other buffer
  CHECK(go(kViews[3], 0, false).mode == kOrderToday);
  p = go(kViews[3], 1, false);
  CHECK(p.mode == kOrderRefine && p.buf == 1);
  // a third view while both buffers are read: no buffer, TODAY, and REFINE once they have ended
  CHECK(go(kViews[7], 2, false).mode == kOrderToday);
  CHECK(go(kViews[7], 3, false).mode == kOrderToday);
  CHECK(go(kViews[7], 0, true).mode == kOrderRefine);
  // alternating views never share
  OrderPlanner alt;
  for (int i = 0; i < 8; ++i) {
    const View& v = kViews[i & 1 ? 3 : 0];
    const DevFrame fr = frame_of(v);
    const OrderKnobs k = order_knobs();
    CHECK(alt.plan(order_key(fr, order_blocks(fr), k, alt.epoch(), v.tiles, v.by_ptr), true, i % 4, idle).mode == kOrderToday);
  }
  // the side clamps: 4 spp -> 1; 1 spp: LPT off
  pl.invalidate();
  CHECK(go(kViews[1], 0, true).mode == kOrderToday);
  p = go(kViews[1], 1, true);
  CHECK(p.mode == kOrderRefine && p.side == 1u);
  for (int i = 0; i < 3; ++i) CHECK(go(kViews[2], i, true).mode == kOrderToday);
  // seeds are no part of a view; the tile list's identity, the epoch and the knobs are
  const DevFrame fr = frame_of(kViews[0]);
  const OrderKnobs k = order_knobs();
  const OrderKey a = order_key(fr, 28, k, 1, 5, false);
  CHECK(!same_view(a, order_key(fr, 28, k, 2, 5, false)) && !same_view(a, order_key(fr, 28, k, 1, 6, false)));
  CHECK(!same_view(a, order_key(fr, 28, k, 1, 5, true)) && !same_view(a, order_key(fr, 29, k, 1, 5, false)));
  CHECK(!same_view(a, order_key(fr, 28, OrderKnobs{1, 4}, 1, 5, false)));
  DevFrame f2 = fr;
  f2.perm = (const uint32_t*)&f2;  // what launch_render fills in is none of the view
  f2.n_slots = 77;
  CHECK(same_view(a, order_key(f2, 28, k, 1, 5, false)));
  const wgt_tile t0[2] = {{0, 8, 1, 2}, {16, 0, 3, 4}}, t1[2] = {{0, 8, 9, 9}, {16, 0, 9, 9}}, t2[2] = {{8, 0, 1, 2}, {16, 0, 3, 4}};
  CHECK(order_tiles_hash(t0, 2) == order_tiles_hash(t1, 2) && order_tiles_hash(t0, 2) != order_tiles_hash(t2, 2));
  CHECK(order_tiles_hash(t0, 1) != order_tiles_hash(t0, 2));
  // WGT_PQ_REUSE=0: every launch on its own
  set_knob("WGT_PQ_REUSE", 0);
  OrderPlanner off;
  for (int i = 0; i < 4; ++i) {
    const OrderKnobs k0 = order_knobs();
    CHECK(!order_eligible(fr, k0, false, 28));
    CHECK(off.plan(order_key(fr, 28, k0, off.epoch(), 5, false), order_eligible(fr, k0, false, 28), i, idle).mode == kOrderToday);
  }
  // block counts the kernels refuse are no view
  DevFrame big = fr;
  big.tw = big.th = 0xffffffffu;
  big.n_tiles = 0xffffffffu;
  CHECK(order_blocks(big) == 0u);
  big.tw = big.th = 8;
  big.n_tiles = 1u << 26;
  CHECK(order_blocks(big) == 0u);
  big.n_tiles = (1u << 26) - 1u;
  CHECK(order_blocks(big) == (1u << 26) - 1u);
}

int main() {
  check_sequence();
  for (uint32_t seed = 1; seed <= 3000; ++seed) run(seed);
  if (g_fail) {
    std::fprintf(stderr, "order_plan_fuzz: %d failed checks\n", g_fail);
    return 1;
  }
  // the sequences reached every plan, and a REFINE refused for want of a free buffer
  CHECK(g_today > 1000 && g_refine > 1000 && g_reuse > 1000 && g_refused > 100);
  if (g_fail) return 1;
  std::printf("order_plan_fuzz: ok (today %llu, refine %llu, reuse %llu, refused %llu)\n", g_today, g_refine, g_reuse, g_refused);
  return 0;
}
