// rebuild_fuzz.cpp — the host side of the BVH rebuild under AddressSanitizer + UBSan (CPU only; built
// and run by tests/test_rebuild_sanitize.py): the specification BuildMortonBvh over seeded random
// and degenerate meshes for every leaf target, and what wgt_rebuild_triangles plans on the host
// (launch_plan.h check_rebuild_records, rebuild_node_cap, tree_layout, plan_rebuild_scratch,
// plan_tree_form, level_begin_of).  Exits non-zero on a failed invariant; the sanitizers abort on
// the first finding.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../include/wgt_api.h"
#include "../../webgputracer_amd/csrc/host/bvh.h"
#include "../../webgputracer_amd/csrc/host/launch_plan.h"

static int g_fail = 0;
#define CHECK(c)                                                         \
  do {                                                                   \
    if (!(c)) {                                                          \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                                          \
    }                                                                    \
  } while (0)

static wgt_triangle tri(float x, float y, float z, float ex, float ey, float ez) {
  wgt_triangle t{};
  t.v0[0] = x; t.v0[1] = y; t.v0[2] = z;
  t.e1[0] = ex; t.e1[1] = 0.0f; t.e1[2] = 0.0f;
  t.e2[0] = 0.0f; t.e2[1] = ey; t.e2[2] = ez;
  t.face_norm[1] = 1.0f;
  t.col[0] = 0.5f;
  return t;
}

// Seeded meshes: a uniform soup, a clustered one (most codes share long prefixes), a geometric chain
// (unbalanced codes), copies of one triangle, a sheet without extent on one axis, zero-area triangles.
static std::vector<wgt_triangle> mesh(std::mt19937& g, int kind, uint32_t n) {
  std::uniform_real_distribution<float> u(0.0f, 1.0f);
  std::vector<wgt_triangle> t;
  for (uint32_t i = 0; i < n; ++i) {
    switch (kind) {
      case 0: t.push_back(tri(500.0f * u(g), 500.0f * u(g), 500.0f * u(g), 5.0f * u(g), 5.0f * u(g), 5.0f * u(g))); break;
      case 1: {
        const float c = (float)(i % 3) * 1e4f;
        t.push_back(tri(c + u(g), c + u(g), 1e-3f * u(g), 0.01f, 0.01f, 0.0f));
        break;
      }
      case 2: t.push_back(tri(std::ldexp(1.0f, (int)(i % 30)), 0.0f, u(g), 0.5f, 0.5f, 0.0f)); break;
      case 3: t.push_back(tri(1.0f, 2.0f, 3.0f, 1.0f, 1.0f, 1.0f)); break;
      case 4: t.push_back(tri(100.0f * u(g), 7.0f, 100.0f * u(g), 1.0f, 0.0f, 1.0f)); break;
      default: t.push_back(tri(10.0f * u(g), 10.0f * u(g), 10.0f * u(g), 0.0f, 0.0f, 0.0f)); break;
    }
  }
  return t;
}

// Every triangle in exactly one leaf of at most `leaf`, refs forward and in range, levels contiguous,
// the stack need as the paths give it.
static void check_tree(const wgt::BvhOut& t, uint32_t n, uint32_t leaf, const std::vector<uint32_t>& level_count) {
  using namespace wgt;
  CHECK(t.n_nodes >= 1 && t.n_nodes <= rebuild_node_cap(n));
  CHECK(t.nodes.size() == (size_t)t.n_nodes * kNode4Floats && t.tris.size() == (size_t)n * kTriRecordFloats);
  CHECK(t.cnodes.size() == (size_t)t.n_nodes * kCNodeFloats && t.crefs.size() == (size_t)t.n_nodes * kBvhWidth);
  CHECK(t.max_depth == level_count.size() && t.max_depth <= kRebuildLevels);
  CHECK(t.stack_need >= 1 && t.stack_need <= (uint32_t)kStackMax);
  CHECK(t.n_nodes2 == 0 && t.depth2 == 0 && t.sah_cost == 0.0);
  const std::vector<uint32_t> begin = level_begin_of(level_count);
  CHECK(begin.back() == t.n_nodes);
  std::vector<uint32_t> seen(n, 0u), path(t.n_nodes, 0u), level(t.n_nodes, 0u);
  uint32_t need = 0, leaves = 0, max_leaf = 0;
  for (uint32_t k = 0; k < t.n_nodes; ++k) {
    const auto node = Node4(t.nodes, k);
    uint32_t live = 0;
    for (int s = 0; s < kBvhWidth; ++s) live += node.live(s) ? 1u : 0u;
    CHECK(live >= 1);
    const uint32_t here = path[k] + std::max(live, 2u) - 1u;  // the single-leaf root counts its empty slot
    need = std::max(need, here);
    CHECK(k >= begin[level[k]] && k < begin[level[k] + 1]);
    for (int s = 0; s < kBvhWidth; ++s) {
      const int32_t r = node.ref(s);
      CHECK(r == t.crefs[(size_t)k * kBvhWidth + s]);
      if (!node.live(s)) { CHECK(r == node.ref(0)); continue; }
      if (r < 0) {
        const uint32_t first = leaf_first(r), cnt = leaf_count(r);
        CHECK(cnt <= leaf && (uint64_t)first + cnt <= n);
        for (uint32_t j = first; j < first + cnt && j < n; ++j) seen[j]++;
        ++leaves;
        max_leaf = std::max(max_leaf, cnt);
      } else {
        CHECK((uint32_t)r > k && (uint32_t)r < t.n_nodes);
        if ((uint32_t)r < t.n_nodes) { path[r] = here; level[r] = level[k] + 1; }
      }
    }
  }
  CHECK(need == t.stack_need && leaves == t.n_leaves && max_leaf == t.max_leaf);
  std::vector<uint32_t> idx(n);
  for (uint32_t i = 0; i < n; ++i) {
    CHECK(seen[i] == 1);
    std::memcpy(&idx[i], &t.tris[(size_t)i * kTriRecordFloats + 3], 4);
  }
  std::sort(idx.begin(), idx.end());
  for (uint32_t i = 0; i < n; ++i) CHECK(idx[i] == i);
}

static void fuzz_specification() {
  using namespace wgt;
  std::mt19937 g(20);
  const uint32_t counts[] = {1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64, 65, 255, 256, 257, 1000, 4099};
  for (int kind = 0; kind < 6; ++kind)
    for (const uint32_t n : counts)
      for (const uint32_t leaf : {1u, 4u, 8u}) {
        const std::vector<wgt_triangle> t = mesh(g, kind, n);
        const double extent = scene_extent(nullptr, 0, nullptr, 0, t.data(), n);
        BvhOut a, b;
        std::vector<uint32_t> level_count;
        std::string err;
        CHECK(BuildMortonBvh(t.data(), n, leaf, 4.0 * extent, a, &level_count, err));
        if (!err.empty()) { std::fprintf(stderr, "kind %d n %u leaf %u: %s\n", kind, n, leaf, err.c_str()); continue; }
        check_tree(a, n, leaf, level_count);
        // a refit of the rebuilt tree to its own triangles reproduces it, and the build is deterministic
        CHECK(BuildMortonBvh(t.data(), n, leaf, 4.0 * extent, b, nullptr, err));
        CHECK(a.nodes.size() == b.nodes.size() && std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * 4) == 0);
        CHECK(RefitBvh(b, t.data(), n, 4.0 * extent, err));
        CHECK(std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * 4) == 0);
        CHECK(std::memcmp(a.cnodes.data(), b.cnodes.data(), a.cnodes.size() * 4) == 0);
        // what the counts decide of the scene
        DevScene sc{};
        plan_tree_form(a, n, sc);
        CHECK(sc.n_tris == n && sc.n_nodes == a.n_nodes && sc.stack == stack_entries(a) && sc.stack <= (uint32_t)kStackMax + 1);
        CHECK(sc.ps_waves == 6 && ps_form(sc).cap == sc.stack);
      }
  // refusals of the specification itself
  BvhOut o;
  std::string err;
  const wgt_triangle one = tri(0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f);
  CHECK(!BuildMortonBvh(&one, 0, 4, 1.0, o, nullptr, err) && err.find("no triangles") != std::string::npos);
  CHECK(!BuildMortonBvh(&one, (uint32_t)rebuild_max_tris(1) + 1u, 1, 1.0, o, nullptr, err) &&
        err.find("too many triangles for a rebuild") != std::string::npos);  // before a record is read
  wgt_triangle nan = one;
  nan.v0[1] = std::numeric_limits<float>::quiet_NaN();
  const wgt_triangle two[2] = {one, nan};
  CHECK(!BuildMortonBvh(two, 2, 4, 1.0, o, nullptr, err) && err.find("non-finite triangle 1") != std::string::npos);
}

static void fuzz_planning() {
  using namespace wgt;
  alignas(16) static const char buf[32] = {};
  // the checks' order: null, count 0, too many, alignment
  CHECK(check_rebuild_records(nullptr, 0, 4, true).find("null") != std::string::npos);
  CHECK(check_rebuild_records(buf + 4, 0, 4, true).find("count 0") != std::string::npos);
  for (const uint32_t leaf : {1u, 2u, 4u, 8u}) {
    const uint64_t lim = rebuild_max_tris(leaf);
    CHECK(lim == (uint64_t)leaf * 1048576u);
    CHECK(check_rebuild_records(buf, (uint32_t)lim, leaf, true).empty());
    CHECK(check_rebuild_records(buf + 4, (uint32_t)lim + 1u, leaf, true).find("too many triangles for a rebuild") != std::string::npos);
  }
  CHECK(check_rebuild_records(buf, 0xffffffffu, 8, true).find("too many") != std::string::npos);
  CHECK(check_rebuild_records(buf + 4, 5, 4, true).find("misaligned") != std::string::npos);
  CHECK(check_rebuild_records(buf + 4, 5, 4, false).empty());  // the host form has no alignment rule
  CHECK(check_rebuild_records(buf + 16, 5, 4, true).empty());
  std::mt19937 g(21);
  std::uniform_int_distribution<uint32_t> un(1u, (uint32_t)rebuild_max_tris(8));
  for (int it = 0; it < 2000; ++it) {
    const uint32_t n = it < 8 ? (uint32_t)it + 1u : un(g), cap = rebuild_node_cap(n);
    CHECK(cap >= 1 && cap <= std::max(n, 2u) - 1u);
    size_t off[kSceneParts] = {};
    const size_t total = tree_layout(n, cap, off);
    const size_t sizes[kSceneParts] = {0, 0, (size_t)cap * 128, (size_t)n * 64, (size_t)n * 32, (size_t)cap * 80, cap};
    for (int p = kPartNodes; p < kSceneParts; ++p) {
      CHECK(off[p] % 256 == 0 && off[p] + sizes[p] <= (p + 1 < kSceneParts ? off[p + 1] : total));
    }
    const size_t temp = (size_t)(it % 5) * 1000u + 1u;
    const RebuildScratch ws = plan_rebuild_scratch(n, temp);
    // the parts in order, none overlapping, each large enough
    const size_t at[] = {ws.key[0], ws.key[1], ws.val[0], ws.val[1], ws.list[0], ws.list[1], ws.cuts, ws.count,
                         ws.offset, ws.bounds, ws.stats, ws.temp, ws.bytes};
    const size_t need[] = {(size_t)n * 8, (size_t)n * 8, (size_t)n * 4, (size_t)n * 4, (size_t)cap * 16, (size_t)cap * 16,
                           (size_t)cap * 16, ((size_t)cap + 1) * 4, ((size_t)cap + 1) * 4, sizeof(RebuildBounds),
                           sizeof(RebuildStats), temp};
    for (int p = 0; p < 12; ++p) CHECK(at[p] % 256 == 0 && at[p] + need[p] <= at[p + 1]);
  }
  CHECK(level_begin_of({}).size() == 1 && level_begin_of({}).front() == 0u);
  const std::vector<uint32_t> b = level_begin_of({1u, 4u, 9u});
  CHECK(b.size() == 4 && b[0] == 0 && b[1] == 1 && b[2] == 5 && b[3] == 14);
}

int main() {
  fuzz_specification();
  fuzz_planning();
  if (g_fail) {
    std::fprintf(stderr, "rebuild_fuzz: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("rebuild_fuzz: ok\n");
  return 0;
}
