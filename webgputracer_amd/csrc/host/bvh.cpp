// bvh.cpp — binned-SAH BVH2 builder, collapsed into the 4-wide BVH the kernels
// traverse.  Leaf boxes are unions of the padded triangle boxes of the geometry
// spec (wgt_geom.h tri_box, evaluated on the host with the same fp32 operations),
// so every node box contains, bit for bit, the boxes of all triangles below it:
// the traversal is exact.  The collapse only regroups BVH2 child
// boxes, so the BVH4 child boxes are exactly BVH2 node boxes.
#include "bvh.h"

#include "../wgt_compact.h"
#include "../wgt_morton.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>
#include <memory>

namespace wgt {
namespace {

constexpr float kInf = std::numeric_limits<float>::infinity();

struct Box {
  float lo[3], hi[3];
  void reset() {
    for (int c = 0; c < 3; ++c) {
      lo[c] = kInf;
      hi[c] = -kInf;
    }
  }
  void grow(const Box& b) {
    for (int c = 0; c < 3; ++c) {
      lo[c] = std::min(lo[c], b.lo[c]);
      hi[c] = std::max(hi[c], b.hi[c]);
    }
  }
  double area() const {
    double dx = (double)hi[0] - lo[0], dy = (double)hi[1] - lo[1], dz = (double)hi[2] - lo[2];
    if (dx < 0 || dy < 0 || dz < 0) return 0.0;
    return 2.0 * (dx * dy + dy * dz + dz * dx);
  }
};

struct Prim {
  Box b;
  float c[3];
  uint32_t idx;
};

// A child of a BVH2 node, or a slot of a BVH4 node: its box and its ref (wgt_geom.h)
struct Child {
  Box b;
  int ref;
};
// The SAH BVH2 (host only), in preorder: children follow their parent.
struct Node2 {
  Child c[2];
};
using Bvh2 = std::vector<Node2>;

constexpr int kMaxBins = 256;
constexpr double kCostTri = 1.0;  // SAH cost of a triangle test (BvhOptions::sah_trav: of a node visit)

// Depth of a median-split subtree over `count` primitives (leaves <= kLeafMax).
uint32_t MedianDepth(uint32_t count) {
  uint32_t d = 0;
  for (; count > (uint32_t)kLeafMax; count = (count + 1) / 2) ++d;
  return d;
}

class Builder {
 public:
  Builder(std::vector<Prim>& p, BvhOut& o, Bvh2& n2, const BvhOptions& opt)
      : prims_(p), out_(o), nodes_(n2), limit_(opt.max_depth), sah_leaf_(std::min(opt.sah_leaf, (uint32_t)kLeafMax)),
        cost_trav_(opt.sah_trav), bins_(std::max(2, std::min(opt.sah_bins, kMaxBins))) {}

  // Returns the child reference of the subtree over prims_[begin, end).
  int Build(uint32_t begin, uint32_t end, uint32_t depth, Box& box) {
    box.reset();
    Box cb;
    cb.reset();
    for (uint32_t i = begin; i < end; ++i) {
      box.grow(prims_[i].b);
      for (int c = 0; c < 3; ++c) {
        cb.lo[c] = std::min(cb.lo[c], prims_[i].c[c]);
        cb.hi[c] = std::max(cb.hi[c], prims_[i].c[c]);
      }
    }
    const uint32_t count = end - begin;
    out_.depth2 = std::max(out_.depth2, depth);
    if (count == 1) return MakeLeaf(begin, count, box);

    uint32_t mid = begin;
    // Depth guarantee: every leaf at depth <= limit_ (the traversal stack holds at
    // most `depth` entries).  Invariant: depth + MedianDepth(count) <= limit_; an SAH
    // split is taken only if both children keep it, otherwise the median split does.
    bool median = true;  // unless an SAH split is taken; of few enough triangles, a leaf instead
    double best = std::numeric_limits<double>::infinity();
    int best_axis = -1, best_bin = -1;
    const double parea = box.area();
    for (int axis = 0; axis < 3; ++axis) {
      const float ext = cb.hi[axis] - cb.lo[axis];
      if (!(ext > 0.0f)) continue;
      Box bb[kMaxBins];
      uint32_t bn[kMaxBins] = {};
      for (int k = 0; k < bins_; ++k) bb[k].reset();
      const double scale = bins_ / (double)ext;
      for (uint32_t i = begin; i < end; ++i) {
        int k = std::min(bins_ - 1, (int)((prims_[i].c[axis] - cb.lo[axis]) * scale));
        bb[k].grow(prims_[i].b);
        bn[k]++;
      }
      double rarea[kMaxBins];
      uint32_t rcount[kMaxBins];
      Box acc;
      acc.reset();
      uint32_t n = 0;
      for (int k = bins_ - 1; k > 0; --k) {
        acc.grow(bb[k]);
        n += bn[k];
        rarea[k] = acc.area();
        rcount[k] = n;
      }
      acc.reset();
      n = 0;
      for (int k = 0; k < bins_ - 1; ++k) {
        acc.grow(bb[k]);
        n += bn[k];
        if (n == 0 || rcount[k + 1] == 0) continue;
        double cost = acc.area() * n + rarea[k + 1] * rcount[k + 1];
        if (cost < best) {
          best = cost;
          best_axis = axis;
          best_bin = k;
        }
      }
    }
    const double split_cost = cost_trav_ + kCostTri * (parea > 0 ? best / parea : 0.0);
    const double leaf_cost = kCostTri * count;
    if (best_axis >= 0 && !(count <= sah_leaf_ && leaf_cost <= split_cost)) {
      const float ext = cb.hi[best_axis] - cb.lo[best_axis];
      const double scale = bins_ / (double)ext;
      auto it = std::partition(prims_.begin() + begin, prims_.begin() + end, [&](const Prim& p) {
        int k = std::min(bins_ - 1, (int)((p.c[best_axis] - cb.lo[best_axis]) * scale));
        return k <= best_bin;
      });
      mid = (uint32_t)(it - prims_.begin());
      median = mid == begin || mid == end || depth + 1 + MedianDepth(std::max(mid - begin, end - mid)) > limit_;
    }
    if (median) {
      if (count <= (uint32_t)kLeafMax) return MakeLeaf(begin, count, box);
      int axis = 0;
      for (int c = 1; c < 3; ++c)
        if (cb.hi[c] - cb.lo[c] > cb.hi[axis] - cb.lo[axis]) axis = c;
      mid = begin + count / 2;
      std::nth_element(prims_.begin() + begin, prims_.begin() + mid, prims_.begin() + end,
                       [axis](const Prim& a, const Prim& b) {
                         return a.c[axis] < b.c[axis] || (a.c[axis] == b.c[axis] && a.idx < b.idx);
                       });
    }
    const size_t id = nodes_.size();
    nodes_.emplace_back();
    Child l, r;
    l.ref = Build(begin, mid, depth + 1, l.b);
    r.ref = Build(mid, end, depth + 1, r.b);
    nodes_[id] = Node2{{l, r}};
    out_.sah_cost += cost_trav_ * box.area();
    return (int)id;
  }

 private:
  int MakeLeaf(uint32_t begin, uint32_t count, const Box& box) {
    out_.n_leaves++;
    out_.max_leaf = std::max(out_.max_leaf, count);
    out_.sah_cost += kCostTri * count * box.area();
    return leaf_ref(begin, count);
  }

  std::vector<Prim>& prims_;
  BvhOut& out_;
  Bvh2& nodes_;
  uint32_t limit_, sah_leaf_;
  double cost_trav_;
  int bins_;
};

// A collapse's result: the BVH4 nodes in preorder, their exact worst-case stack need and depth.
struct Tree4 {
  std::vector<float> nodes;
  uint32_t stack_need = 0, max_depth = 0;
  uint32_t size() const { return (uint32_t)(nodes.size() / kNode4Floats); }
};

// Appends the BVH4 node of the slots ch[0, n) (2 <= n <= kBvhWidth) at `depth` and, through
// sub(ref2, need) -> node index, the subtrees of its internal slots, in preorder; returns its
// index.  `need` receives the worst-case stack entries of the subtree: the traversal pushes at
// most (children - 1) per node on a root-to-node path, so need = (n - 1) + max over internal
// slots.  Empty slots are padded as wgt_geom.h says.
template <class Sub>
int EmitNode(Tree4& t, const Child* ch, int n, uint32_t depth, uint32_t& need, Sub&& sub) {
  const size_t id = t.size();
  t.nodes.resize(t.nodes.size() + kNode4Floats);
  t.max_depth = std::max(t.max_depth, depth + 1);
  int refs[kBvhWidth];
  uint32_t deepest = 0;
  for (int i = 0; i < n; ++i) {
    refs[i] = ch[i].ref;
    if (ch[i].ref < 0) continue;
    uint32_t sn = 0;
    refs[i] = sub(ch[i].ref, sn);
    deepest = std::max(deepest, sn);
  }
  need = (uint32_t)(n - 1) + deepest;
  const auto o = Node4(t.nodes, id);  // only now: the subtrees grew t.nodes
  for (int i = 0; i < kBvhWidth; ++i) {
    const bool live = i < n;
    for (int c = 0; c < 3; ++c) {
      o.lo(c, i) = live ? ch[i].b.lo[c] : kEmptySlotCoord;
      o.hi(c, i) = live ? ch[i].b.hi[c] : kEmptySlotCoord;
    }
    o.set_ref(i, live ? refs[i] : refs[0]);
    o.pad(i) = 0.0f;
  }
  return (int)id;
}

// Budgeted greedy collapse: a BVH4 node starts from the two children of a BVH2
// node and repeatedly opens its largest-area internal child until it has 4
// slots.  The stack is bounded by `budget`: a child is opened only while (children - 1)
// + the least need any child can still reach (its BVH2 height: a 2-wide node
// pushes one entry per level) fits, so only the deep, stack-heavy paths get
// narrower nodes.  Any budget >= the BVH2 height is met.
class Collapser {
 public:
  explicit Collapser(const Bvh2& n2) : n2_(n2), h_(n2.size(), 0u) {
    for (size_t i = h_.size(); i-- > 0;) h_[i] = 1u + std::max(Below(n2_[i].c[0]), Below(n2_[i].c[1]));
  }
  uint32_t Height(int id2) const { return h_[id2]; }

  Tree4 Run(uint32_t budget) const {
    Tree4 t;
    Collapse(t, 0, 0, budget, t.stack_need);
    return t;
  }

 private:
  uint32_t Below(const Child& c) const { return c.ref >= 0 ? h_[c.ref] : 0u; }

  int Collapse(Tree4& t, int id2, uint32_t depth, uint32_t budget, uint32_t& need) const {
    Child ch[kBvhWidth] = {n2_[id2].c[0], n2_[id2].c[1]};
    int n = 2;
    bool blocked[kBvhWidth] = {false, false, false, false};
    while (n < kBvhWidth) {
      int best = -1;
      double ba = -1.0;
      for (int i = 0; i < n; ++i)
        if (ch[i].ref >= 0 && !blocked[i] && ch[i].b.area() > ba) {
          ba = ch[i].b.area();
          best = i;
        }
      if (best < 0) break;
      // the node after opening `best`: n children, the least subtree need of each
      const Child a = n2_[ch[best].ref].c[0], b = n2_[ch[best].ref].c[1];
      uint32_t m = std::max(Below(a), Below(b));
      for (int i = 0; i < n; ++i)
        if (i != best) m = std::max(m, Below(ch[i]));
      if ((uint32_t)n + m > budget) {  // (n + 1 children) - 1 + m
        blocked[best] = true;
        continue;
      }
      ch[best] = a;
      ch[n++] = b;
    }
    return EmitNode(t, ch, n, depth, need, [&](int ref2, uint32_t& sn) {
      return Collapse(t, ref2, depth + 1, budget - (uint32_t)(n - 1), sn);
    });
  }

  const Bvh2& n2_;
  std::vector<uint32_t> h_;  // BVH2 height (internal levels) of every BVH2 node
};

// SAH-optimal collapse under the stack budget (the default; BvhOptions::kGreedy
// selects Collapser).  Every BVH4 node is a frontier of 2..4 descendants of a BVH2
// node; a dynamic program over the BVH2 (children before parents) picks, per node
// and per stack budget B, the frontier minimising the BVH4 SAH cost
//   N(r, B) = c_node * A(r) + min_{k=2..4} Q(r's children -> k slots, B - (k - 1))
//   Q(c -> 1 slot, B) = leaf ? c_tri * count * A(c) : N(c, B)
//   Q(c -> k slots, B) = min_{i + j = k} Q(left(c) -> i, B) + Q(right(c) -> j, B)
// (A = surface area; a node of k slots pushes at most k - 1 entries, so its
// subtree's stack need is (k - 1) + the largest need of its internal slots).
// Like the greedy collapse it only regroups BVH2 boxes: the BVH4 child boxes are
// BVH2 node boxes and the exactness argument is unchanged.
// The table is built once, for every budget up to `budget`; Run queries it.
class DpCollapser {
 public:
  DpCollapser(const Bvh2& n2, const BvhOptions& opt, uint32_t budget)
      : n2_(n2), nb_(budget + 1), n_(n2.size()), c_node_(opt.dp_node), c_tri_(opt.dp_tri),
        leaf_max_(std::min(opt.dp_leaf, (uint32_t)kLeafMax)) {
    cost_.assign(n_ * 4 * nb_, kInf);  // [node][k-1][B]: k = 1 is N(node, B)
    range_.assign(n_, Range{0u, 0u});
    area_.assign(n_, 0.0);
    for (size_t i = n_; i-- > 0;) {   // preorder: children have larger ids
      const Child a = n2_[i].c[0], b = n2_[i].c[1];
      Box u = a.b;
      u.grow(b.b);
      const double area = u.area();
      area_[i] = area;
      // the node's triangles: one contiguous range (the children's ranges are adjacent)
      const Range ra = Tris(a), rb = Tris(b);
      range_[i] = Range{std::min(ra.first, rb.first), ra.count + rb.count};
      for (uint32_t B = 0; B < nb_; ++B) {
        // k slots of node i's frontier, each with need <= B
        for (int k = 2; k <= 4; ++k) {
          float best = kInf;
          for (int ia = 1; ia < k; ++ia) best = std::min(best, Slots(a, ia, B) + Slots(b, k - ia, B));
          Q(i, k, B) = best;
        }
        float best = kInf;
        for (int k = 2; k <= 4; ++k)
          if ((uint32_t)(k - 1) <= B) best = std::min(best, Q(i, k, B - (uint32_t)(k - 1)));
        Q(i, 1, B) = (float)(c_node_ * area) + best;
      }
    }
  }
  // The least SAH cost of a tree with stack need <= budget (infinite: the table has none).
  float Cost(uint32_t budget) const { return budget < nb_ ? Q(0, 1, budget) : kInf; }

  Tree4 Run(uint32_t budget) const {
    Tree4 t;
    Emit(t, 0, 0, budget, t.stack_need);
    return t;
  }

 private:
  // Emit node id2 as a BVH4 node with stack need <= budget.
  int Emit(Tree4& t, int id2, uint32_t depth, uint32_t budget, uint32_t& need) const {
    int best_k = 2;
    float best = kInf;
    for (int k = 2; k <= 4; ++k)
      if ((uint32_t)(k - 1) <= budget && Q(id2, k, budget - (uint32_t)(k - 1)) < best) {
        best = Q(id2, k, budget - (uint32_t)(k - 1));
        best_k = k;
      }
    const uint32_t sb = budget - (uint32_t)(best_k - 1);
    Child slots[kBvhWidth];
    int n = 0;
    Split(n2_[id2].c[0], n2_[id2].c[1], best_k, sb, slots, n);
    return EmitNode(t, slots, n, depth, need, [&](int ref2, uint32_t& sn) { return Emit(t, ref2, depth + 1, sb, sn); });
  }

  float& Q(size_t node, int k, uint32_t B) { return cost_[(node * 4 + (size_t)(k - 1)) * nb_ + B]; }
  float Q(size_t node, int k, uint32_t B) const { return cost_[(node * 4 + (size_t)(k - 1)) * nb_ + B]; }
  // cost of covering child c with k slots, each of stack need <= B
  float Slots(const Child& c, int k, uint32_t B) const {
    if (c.ref < 0) return k == 1 ? (float)(c_tri_ * leaf_count(c.ref) * c.b.area()) : kInf;
    if (k == 1 && Mergeable(c)) return std::min(Q((size_t)c.ref, 1, B), MergedCost(c));
    return Q((size_t)c.ref, k, B);
  }
  struct Range {
    uint32_t first, count;
  };
  Range Tris(const Child& c) const {
    if (c.ref < 0) return Range{leaf_first(c.ref), leaf_count(c.ref)};
    return range_[(size_t)c.ref];
  }
  // an internal BVH2 child with few enough triangles may become one leaf slot
  bool Mergeable(const Child& c) const {
    if (c.ref < 0 || leaf_max_ == 0) return false;
    const uint32_t n = range_[(size_t)c.ref].count;
    return n != 0 && n <= leaf_max_;
  }
  float MergedCost(const Child& c) const { return (float)(c_tri_ * range_[(size_t)c.ref].count * area_[(size_t)c.ref]); }
  // the slot of child c in a cover by one slot: merged into a leaf when that is cheaper
  Child AsSlot(const Child& c, uint32_t B) const {
    if (Mergeable(c) && MergedCost(c) < Q((size_t)c.ref, 1, B)) {
      const Range r = range_[(size_t)c.ref];
      Child m = c;
      m.ref = leaf_ref(r.first, r.count);
      return m;
    }
    return c;
  }
  // the slots of the cheapest cover of a and b by k slots (budget B each), appended to out[n...]
  void Split(const Child& a, const Child& b, int k, uint32_t B, Child* out, int& n) const {
    int best_i = 1;
    float best = kInf;
    for (int i = 1; i < k; ++i) {
      const float c = Slots(a, i, B) + Slots(b, k - i, B);
      if (c < best) {
        best = c;
        best_i = i;
      }
    }
    Cover(a, best_i, B, out, n);
    Cover(b, k - best_i, B, out, n);
  }
  void Cover(const Child& c, int k, uint32_t B, Child* out, int& n) const {
    if (k == 1) out[n++] = AsSlot(c, B);
    else Split(n2_[c.ref].c[0], n2_[c.ref].c[1], k, B, out, n);
  }

  const Bvh2& n2_;
  uint32_t nb_;
  size_t n_;
  double c_node_, c_tri_;
  uint32_t leaf_max_;
  std::vector<float> cost_;
  std::vector<Range> range_;
  std::vector<double> area_;
};

// The compact form's arithmetic is wgt_compact.h's (shared with the device refit).  The smallest
// power-of-two step every node accepts (compact_step_ok); the predicate is monotone in the step,
// so this is the largest of the nodes' own smallest steps (compact_node_exp).
float CompactStep(const BvhOut& out, double G) {
  int e = kCompactMinExp;
  for (;;) {
    const float s = std::ldexp(1.0f, e);
    bool ok = true;
    for (uint32_t k = 0; k < out.n_nodes && ok; ++k) ok = compact_step_ok(&out.nodes[(size_t)k * kNode4Floats], s, G);
    if (ok) return s;
    ++e;
  }
}

// ---- the stages of BuildBvh, in order; a failing stage says why in err ----

// The primitives: each triangle's padded box (tri_box) and its centre.
bool MakePrims(const wgt_triangle* tris, uint32_t n, const BvhOptions& opt, std::vector<Prim>& prims, std::string& err) {
  if (n == 0) { err = "BuildBvh: no triangles"; return false; }
  // leaf walks use 32-bit byte offsets into the 64-B records (wgt_geom.h kTriRecordBytes)
  if (n >= (1u << 26)) { err = "BuildBvh: too many triangles (max 2^26-1)"; return false; }
  prims.resize(n);
  for (uint32_t i = 0; i < n; ++i) {
    const wgt_triangle& t = tris[i];
    f3 lo, hi;
    tri_box(f3{t.v0[0], t.v0[1], t.v0[2]}, f3{t.e1[0], t.e1[1], t.e1[2]},
            f3{t.e2[0], t.e2[1], t.e2[2]}, lo, hi);
    Prim& p = prims[i];
    p.b.lo[0] = lo.x; p.b.lo[1] = lo.y; p.b.lo[2] = lo.z;
    p.b.hi[0] = hi.x; p.b.hi[1] = hi.y; p.b.hi[2] = hi.z;
    for (int c = 0; c < 3; ++c) p.c[c] = 0.5f * p.b.lo[c] + 0.5f * p.b.hi[c];
    p.idx = i;
    for (int c = 0; c < 3; ++c)
      if (!std::isfinite(p.b.lo[c]) || !std::isfinite(p.b.hi[c])) {
        err = "BuildBvh: non-finite triangle " + std::to_string(i);
        return false;
      }
  }
  if (MedianDepth(n) > opt.max_depth) {
    err = "BuildBvh: too many triangles for depth limit " + std::to_string(opt.max_depth);
    return false;
  }
  return true;
}

// The SAH BVH2 over prims (reordered into leaf order), with its counts and SAH cost in out.
bool BuildBvh2(std::vector<Prim>& prims, const BvhOptions& opt, Bvh2& n2, BvhOut& out, std::string& err) {
  const uint32_t n = (uint32_t)prims.size();
  n2.reserve(2 * ((size_t)n / 2 + 1));
  Box root_box;
  const int root = Builder(prims, out, n2, opt).Build(0, n, 0, root_box);
  if (root < 0) {
    // single leaf: a root node whose second child is an empty slot (wgt_geom.h)
    Box empty;
    for (int c = 0; c < 3; ++c) empty.lo[c] = empty.hi[c] = kEmptySlotCoord;
    n2.assign(1, Node2{{{root_box, root}, {empty, root}}});
    out.depth2 = 1;
  }
  if (out.depth2 > opt.max_depth) {
    err = "BuildBvh: depth " + std::to_string(out.depth2) + " exceeds " + std::to_string(opt.max_depth);
    return false;
  }
  out.n_nodes2 = (uint32_t)n2.size();
  if (root_box.area() > 0) out.sah_cost /= root_box.area();
  return true;
}

// The BVH4: the BVH2 collapsed under the stack limit and, when asked for and feasible, under
// the narrow limit too; the narrow tree is taken if it is cheap enough.  The greedy heights
// judge feasibility; the optimal collapse's table, built once at the wide budget, serves both.
bool CollapseBvh2(const Bvh2& n2, const BvhOptions& opt, BvhOut& out, std::string& err) {
  const Collapser greedy(n2);
  if (greedy.Height(0) > opt.stack_limit) {
    err = "BuildBvh: BVH2 height " + std::to_string(greedy.Height(0)) + " exceeds the stack limit " +
          std::to_string(opt.stack_limit);
    return false;
  }
  std::unique_ptr<DpCollapser> dp;
  if (opt.collapse == BvhOptions::kOptimal) {
    dp.reset(new DpCollapser(n2, opt, opt.stack_limit));
    if (!(dp->Cost(opt.stack_limit) < kInf)) dp.reset();
  }
  const auto collapse = [&](uint32_t budget) {
    return dp && dp->Cost(budget) < kInf ? dp->Run(budget) : greedy.Run(budget);
  };
  Tree4 tree = collapse(opt.stack_limit);
  if (tree.stack_need > opt.stack_limit) {
    err = "BuildBvh: traversal stack " + std::to_string(tree.stack_need) + " exceeds " + std::to_string(opt.stack_limit);
    return false;
  }
  if (tree.size() >= (1u << 24)) {  // the device copies address nodes by 32-bit byte offsets below kNoRef
    err = "BuildBvh: too many BVH nodes (max 2^24-1)";
    return false;
  }
  if (opt.narrow_limit > 0 && opt.narrow_limit < opt.stack_limit && greedy.Height(0) <= opt.narrow_limit) {
    Tree4 nar = collapse(opt.narrow_limit);
    // greedy trees: at most narrow_ratio x the nodes; optimal trees: at most narrow_ratio
    // x the SAH cost of the wide tree
    const bool cheap = dp ? dp->Cost(opt.narrow_limit) <= opt.narrow_ratio * dp->Cost(opt.stack_limit)
                          : nar.size() <= opt.narrow_ratio * tree.size();
    if (nar.stack_need <= opt.narrow_limit && cheap) {
      tree = std::move(nar);
      out.narrow = true;
    }
  }
  out.n_nodes = tree.size();
  out.stack_need = tree.stack_need;
  out.max_depth = tree.max_depth;
  out.nodes = std::move(tree.nodes);
  return true;
}

// The device traversal has no iteration cap: it terminates because every
// internal ref points forward (preorder), so no node is visited twice.
bool CheckRefs(const BvhOut& out, uint32_t n_tris, std::string& err) {
  for (uint32_t i = 0; i < out.n_nodes; ++i)
    for (int s = 0; s < kBvhWidth; ++s) {
      const int32_t r = Node4(out.nodes, i).ref(s);
      const uint32_t u = ~(uint32_t)r;
      const bool ok = r >= 0 ? ((uint32_t)r > i && (uint32_t)r < out.n_nodes)
                             : ((uint64_t)(u >> 3) + (u & 7u) + 1u <= n_tris);
      if (!ok) {
        err = "BuildBvh: malformed node " + std::to_string(i);
        return false;
      }
    }
  return true;
}

// The compact form of out.nodes.  The codes' margin: M bounds |ray origin| (origin_bound)
// and every coordinate of the tree (so |org'| <= M as well).
void CompactForm(double origin_bound, BvhOut& out) {
  const std::vector<float>& nodes = out.nodes;
  double M = std::max(origin_bound, 0x1p-60);
  for (uint32_t i = 0; i < out.n_nodes; ++i)
    for (int a = 0; a < 3; ++a)
      for (int s = 0; s < kBvhWidth; ++s)
        for (const float v : {Node4(nodes, i).lo(a, s), Node4(nodes, i).hi(a, s)})
          if (v != kEmptySlotCoord) M = std::max(M, 2.0 * std::fabs((double)v));
  out.cbound = (float)M;
  const double G = std::ldexp(M, -21);
  out.cstep = CompactStep(out, G);
  out.cnodes.resize((size_t)out.n_nodes * kCNodeFloats);
  out.crefs.resize((size_t)out.n_nodes * kBvhWidth);
  for (uint32_t i = 0; i < out.n_nodes; ++i) {
    compact_node(&nodes[(size_t)i * kNode4Floats], out.cstep, G, &out.cnodes[(size_t)i * kCNodeFloats]);
    for (int s = 0; s < kBvhWidth; ++s) out.crefs[(size_t)i * kBvhWidth + s] = Node4(nodes, i).ref(s);
  }
}

// The leaf-ordered triangle records (wgt_geom.h).
void TriRecords(const wgt_triangle* tris, const std::vector<Prim>& prims, BvhOut& out) {
  out.tris.resize(prims.size() * kTriRecordFloats);
  for (size_t i = 0; i < prims.size(); ++i) {
    const wgt_triangle& t = tris[prims[i].idx];
    const Box& b = prims[i].b;
    float* o = &out.tris[i * kTriRecordFloats];
    o[0] = t.v0[0]; o[1] = t.v0[1]; o[2] = t.v0[2];
    std::memcpy(&o[3], &prims[i].idx, 4);
    o[4] = t.e1[0]; o[5] = t.e1[1]; o[6] = t.e1[2]; o[7] = b.lo[0];
    o[8] = t.e2[0]; o[9] = t.e2[1]; o[10] = t.e2[2]; o[11] = b.lo[1];
    o[12] = b.lo[2]; o[13] = b.hi[0]; o[14] = b.hi[1]; o[15] = b.hi[2];
  }
}

// The shading records, in the triangles' original order (wgt_internal.h tshade).
void ShadeRecords(const wgt_triangle* tris, uint32_t n, BvhOut& out) {
  out.tshade.resize((size_t)n * 8);
  for (uint32_t i = 0; i < n; ++i) {
    const wgt_triangle& t = tris[i];
    float* o = &out.tshade[(size_t)i * 8];
    o[0] = t.face_norm[0]; o[1] = t.face_norm[1]; o[2] = t.face_norm[2]; o[3] = t.emissive;
    o[4] = t.col[0]; o[5] = t.col[1]; o[6] = t.col[2]; o[7] = 0.0f;
  }
}

}  // namespace

// The builder's tuning knobs (defaults: the measured best), all read here.
BvhOptions BvhOptionsFromEnv(uint32_t max_depth, uint32_t stack_max, uint32_t stack_narrow, double origin_bound) {
  const auto env = [](const char* name) { const char* v = std::getenv(name); return v && *v ? v : nullptr; };
  const auto real = [&](const char* name, double dflt) { return env(name) ? std::atof(env(name)) : dflt; };
  const auto clamped = [&](const char* name, int dflt, int lo, int hi) {
    return std::max(lo, std::min(env(name) ? std::atoi(env(name)) : dflt, hi));
  };
  const auto u32 = [&](const char* name, uint32_t dflt) {
    return env(name) ? (uint32_t)std::strtoul(env(name), nullptr, 10) : dflt;
  };
  BvhOptions o;
  o.max_depth = max_depth;
  o.origin_bound = origin_bound;
  // WGT_STACK_LIMIT (stack_max): a lower stack bound, for sweeps and tests
  o.stack_limit = std::min(u32("WGT_STACK_LIMIT", stack_max), stack_max);
  // WGT_NARROW (0): the narrow collapse, off since 3-byte stack entries give 6 waves per SIMD the full bound;
  // 1 takes it when its cost is within the default narrow_ratio of the wide tree's, 2 whenever it is feasible
  const uint32_t narrow = u32("WGT_NARROW", 0);
  o.narrow_limit = narrow ? stack_narrow : 0u;
  if (narrow == 2) o.narrow_ratio = 1e30;
  o.sah_bins = clamped("WGT_SAH_BINS", o.sah_bins, 2, kMaxBins);          // (128) 2..256
  o.sah_trav = real("WGT_SAH_TRAV", o.sah_trav);                          // (1.0)
  o.sah_leaf = (uint32_t)clamped("WGT_SAH_LEAF", kLeafMax, 1, kLeafMax);  // (8) 1..8
  o.dp_node = real("WGT_DP_NODE", o.dp_node);                             // (1.0)
  o.dp_tri = real("WGT_DP_TRI", o.dp_tri);                                // (1.0)
  o.dp_leaf = (uint32_t)clamped("WGT_DP_LEAF", 0, 0, kLeafMax);           // (0) 0..8
  // WGT_COLLAPSE (dp): "greedy" selects the greedy collapse, anything else the optimal one
  const char* c = env("WGT_COLLAPSE");
  o.collapse = c && std::strcmp(c, "greedy") == 0 ? BvhOptions::kGreedy : BvhOptions::kOptimal;
  return o;
}

bool BuildBvh(const wgt_triangle* tris, uint32_t n, const BvhOptions& opt, BvhOut& out, std::string& err) {
  out = BvhOut{};
  std::vector<Prim> prims;
  Bvh2 n2;
  if (!MakePrims(tris, n, opt, prims, err) || !BuildBvh2(prims, opt, n2, out, err) ||
      !CollapseBvh2(n2, opt, out, err) || !CheckRefs(out, n, err))
    return false;
  CompactForm(opt.origin_bound, out);
  TriRecords(tris, prims, out);
  ShadeRecords(tris, n, out);
  return true;
}

// The refit keeps the topology, so whatever depends on it alone stays: refs, leaf order, n_nodes,
// stack_need, the depths, and sah_cost (the build's value: it describes the tree as built).
// Internal refs point forward (CheckRefs), so one pass from the last node to the root sees every
// child before its parent.  Boxes are exact min/max unions, as the builder's, and tri_box never
// yields -0, so a refit to the triangles of the build reproduces it bit for bit.
bool RefitBvh(BvhOut& bvh, const wgt_triangle* tris, uint32_t n, double origin_bound, std::string& err) {
  if (n == 0 || bvh.n_nodes == 0 || bvh.tris.size() != (size_t)n * kTriRecordFloats ||
      bvh.nodes.size() != (size_t)bvh.n_nodes * kNode4Floats) {
    err = "RefitBvh: the triangle count differs from the build's";
    return false;
  }
  // the records, in the build's leaf order: the same fp32 operations as MakePrims and TriRecords
  std::vector<float> recs(bvh.tris.size());
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t idx;
    std::memcpy(&idx, &bvh.tris[(size_t)i * kTriRecordFloats + 3], 4);
    if (idx >= n) { err = "RefitBvh: malformed triangle record " + std::to_string(i); return false; }
    const wgt_triangle& t = tris[idx];
    f3 lo, hi;
    tri_box(f3{t.v0[0], t.v0[1], t.v0[2]}, f3{t.e1[0], t.e1[1], t.e1[2]}, f3{t.e2[0], t.e2[1], t.e2[2]}, lo, hi);
    for (const float v : {lo.x, lo.y, lo.z, hi.x, hi.y, hi.z})
      if (!std::isfinite(v)) {
        err = "RefitBvh: non-finite triangle " + std::to_string(idx);
        return false;  // bvh is as it was
      }
    float* o = &recs[(size_t)i * kTriRecordFloats];
    o[0] = t.v0[0]; o[1] = t.v0[1]; o[2] = t.v0[2];
    std::memcpy(&o[3], &idx, 4);
    o[4] = t.e1[0]; o[5] = t.e1[1]; o[6] = t.e1[2]; o[7] = lo.x;
    o[8] = t.e2[0]; o[9] = t.e2[1]; o[10] = t.e2[2]; o[11] = lo.y;
    o[12] = lo.z; o[13] = hi.x; o[14] = hi.y; o[15] = hi.z;
  }
  bvh.tris = std::move(recs);
  for (uint32_t k = bvh.n_nodes; k-- > 0;) {
    const auto node = Node4(bvh.nodes, k);
    for (int s = 0; s < kBvhWidth; ++s) {
      if (!node.live(s)) continue;  // empty slots stay as they are
      Box b;
      b.reset();
      const int32_t r = node.ref(s);
      if (r < 0) {
        for (uint32_t j = leaf_first(r), end = j + leaf_count(r); j < end; ++j) {
          const float* o = &bvh.tris[(size_t)j * kTriRecordFloats];
          b.grow(Box{{o[7], o[11], o[12]}, {o[13], o[14], o[15]}});
        }
      } else {
        const auto child = Node4(bvh.nodes, (size_t)r);
        for (int c = 0; c < kBvhWidth; ++c)
          if (child.live(c))
            b.grow(Box{{child.lo(0, c), child.lo(1, c), child.lo(2, c)}, {child.hi(0, c), child.hi(1, c), child.hi(2, c)}});
      }
      for (int a = 0; a < 3; ++a) {
        node.lo(a, s) = b.lo[a];
        node.hi(a, s) = b.hi[a];
      }
    }
  }
  CompactForm(origin_bound, bvh);
  ShadeRecords(tris, n, bvh);
  return true;
}

uint32_t RebuildLeafFromEnv() {
  const char* v = std::getenv("WGT_REBUILD_LEAF");
  const int leaf = v && *v ? std::atoi(v) : (int)kRebuildLeafDefault;
  return (uint32_t)std::max(1, std::min(leaf, kLeafMax));  // (4) 1..8
}

bool BuildMortonBvh(const wgt_triangle* tris, uint32_t n, uint32_t leaf, double origin_bound, BvhOut& out,
                    std::vector<uint32_t>* level_count, std::string& err) {
  out = BvhOut{};
  const uint32_t L = std::max(1u, std::min(leaf, (uint32_t)kLeafMax));
  if (n == 0) { err = "BuildMortonBvh: no triangles"; return false; }
  if (n > rebuild_max_tris(L)) {
    err = "BuildMortonBvh: too many triangles for a rebuild (max " + std::to_string(rebuild_max_tris(L)) + " at leaf target " +
          std::to_string(L) + ")";
    return false;
  }
  // keys: the centres of the padded boxes between their exact bounds
  std::vector<float> c((size_t)n * 3);
  float cmin[3] = {kInf, kInf, kInf}, cmax[3] = {-kInf, -kInf, -kInf};
  for (uint32_t i = 0; i < n; ++i) {
    const wgt_triangle& t = tris[i];
    f3 lo, hi;
    tri_box(f3{t.v0[0], t.v0[1], t.v0[2]}, f3{t.e1[0], t.e1[1], t.e1[2]}, f3{t.e2[0], t.e2[1], t.e2[2]}, lo, hi);
    const float l[3] = {lo.x, lo.y, lo.z}, h[3] = {hi.x, hi.y, hi.z};
    for (int a = 0; a < 3; ++a) {
      if (!std::isfinite(l[a]) || !std::isfinite(h[a])) {
        err = "BuildMortonBvh: non-finite triangle " + std::to_string(i);
        return false;
      }
      const float v = morton_centre(l[a], h[a]);
      c[(size_t)i * 3 + a] = v;
      cmin[a] = std::min(cmin[a], v);
      cmax[a] = std::max(cmax[a], v);
    }
  }
  std::vector<unsigned long long> key(n);
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t q[3];
    for (int a = 0; a < 3; ++a) q[a] = morton_cell(c[(size_t)i * 3 + a], cmin[a], cmax[a]);
    key[i] = morton_code(q[0], q[1], q[2]);
  }
  // the leaf order: ascending by (code, original index)
  std::vector<uint32_t> order(n);
  for (uint32_t i = 0; i < n; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b] || (key[a] == key[b] && a < b); });
  std::vector<unsigned long long> code(n);
  for (uint32_t i = 0; i < n; ++i) code[i] = key[order[i]];
  out.tris.assign((size_t)n * kTriRecordFloats, 0.0f);
  for (uint32_t i = 0; i < n; ++i) std::memcpy(&out.tris[(size_t)i * kTriRecordFloats + 3], &order[i], 4);

  // the topology, level by level: a node's index is its level's first index + its place in the level
  struct Range { uint32_t b, e, r, path; };
  std::vector<Range> level{{0u, n, 2 * kRebuildLevels, 0u}}, next;
  const auto add_node = [&]() {
    out.nodes.resize(out.nodes.size() + kNode4Floats, 0.0f);
    return Node4(out.nodes, out.n_nodes++);
  };
  const auto finish = [&](const Node4T<float>& o, const int* refs, int live) {
    for (int s = 0; s < kBvhWidth; ++s) {
      for (int a = 0; a < 3; ++a) o.lo(a, s) = o.hi(a, s) = s < live ? 0.0f : kEmptySlotCoord;  // a live box: the refit's
      o.set_ref(s, s < live ? refs[s] : refs[0]);
      o.pad(s) = 0.0f;
    }
  };
  if (level_count) level_count->clear();
  if (n <= L) {  // the single-leaf root with one empty slot, as BuildBvh2 makes it: two slots, so one stack entry
    const int refs[kBvhWidth] = {leaf_ref(0, n)};
    finish(add_node(), refs, 1);
    out.n_leaves = 1; out.max_leaf = n; out.max_depth = 1; out.stack_need = 1;
    if (level_count) level_count->push_back(1u);
  } else {
    while (!level.empty()) {
      const uint32_t next_begin = out.n_nodes + (uint32_t)level.size();
      next.clear();
      for (const Range& g : level) {
        uint32_t cut[kBvhWidth + 1];
        const int slots = morton_slots(code.data(), g.b, g.e, g.r, L, cut);
        const uint32_t path = g.path + (uint32_t)(slots - 1);
        out.stack_need = std::max(out.stack_need, path);
        int refs[kBvhWidth] = {};
        for (int s = 0; s < slots; ++s) {
          const uint32_t cnt = cut[s + 1] - cut[s];
          if (cnt <= L) {
            refs[s] = leaf_ref(cut[s], cnt);
            out.n_leaves++;
            out.max_leaf = std::max(out.max_leaf, cnt);
          } else {
            refs[s] = (int)(next_begin + (uint32_t)next.size());
            next.push_back(Range{cut[s], cut[s + 1], g.r - 2, path});
          }
        }
        finish(add_node(), refs, slots);
      }
      out.max_depth++;
      if (level_count) level_count->push_back((uint32_t)level.size());
      level.swap(next);
    }
  }
  if (!CheckRefs(out, n, err)) return false;
  return RefitBvh(out, tris, n, origin_bound, err);
}

BvhImage DeviceImage(const BvhOut& bvh) {
  constexpr size_t kRecWords = kCRecordFloat4s * 4;
  BvhImage im{bvh.nodes, std::vector<uint32_t>(bvh.n_nodes * kRecWords), std::vector<uint8_t>(bvh.n_nodes, 0)};
  for (size_t i = 0; i < bvh.n_nodes; ++i) {
    uint32_t* rec = &im.crecs[i * kRecWords];
    std::memcpy(rec, &bvh.cnodes[i * kCNodeFloats], kCNodeFloats * 4);
    for (int s = 0; s < kBvhWidth; ++s) {
      const int32_t r = Node4(bvh.nodes, i).ref(s), c = bvh.crefs[i * kBvhWidth + s];
      Node4(im.nodes, i).set_ref(s, r >= 0 ? r * (int32_t)(kNode4Floats * 4) : r);
      const int32_t cr = c >= 0 ? c * (int32_t)(kRecWords * 4) : c;
      std::memcpy(&rec[kCNodeFloats + s], &cr, 4);
      // preorder refs point forward, so one pass sets a child's level after its parent's
      if (c >= 0 && (size_t)c < bvh.n_nodes) im.level[c] = (uint8_t)std::min(255, im.level[i] + 1);
    }
  }
  return im;
}

void ExportImage(const float* dev_nodes, const uint32_t* dev_crecs, uint32_t n_nodes, float* nodes_out,
                 uint32_t* cnodes_out, int32_t* crefs_out) {
  constexpr size_t kRecWords = kCRecordFloat4s * 4;
  for (size_t i = 0; i < n_nodes; ++i) {
    if (nodes_out) {
      std::memcpy(&nodes_out[i * kNode4Floats], &dev_nodes[i * kNode4Floats], kNode4Floats * 4);
      const Node4T<float> o{&nodes_out[i * kNode4Floats]};
      for (int s = 0; s < kBvhWidth; ++s)
        if (o.ref(s) >= 0) o.set_ref(s, o.ref(s) / (int32_t)(kNode4Floats * 4));
    }
    const uint32_t* rec = &dev_crecs[i * kRecWords];
    if (cnodes_out) std::memcpy(&cnodes_out[i * kCNodeFloats], rec, kCNodeFloats * 4);
    if (crefs_out)
      for (int s = 0; s < kBvhWidth; ++s) {
        int32_t c;
        std::memcpy(&c, &rec[kCNodeFloats + s], 4);
        crefs_out[i * kBvhWidth + s] = c >= 0 ? c / (int32_t)(kRecWords * 4) : c;
      }
  }
}

}  // namespace wgt
