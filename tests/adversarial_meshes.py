"""Deterministic meshes the BVH builder and the traversal kernels find hard.  TEST INFRASTRUCTURE ONLY.

Shared by tests/test_bvh_adversarial.py (the builder, the split-stack model and the oracle, on the
CPU) and tests/test_gpu_adversarial.py (the kernels).  Every other mesh of the suite is benign: the
bunny and sponza stand-ins, soups with edges from N(0, 3..80), lattices and one flat box.  These
force the builder's depth limit and the 31-entry stack bound, put zero-area triangles, exact
duplicates and scene-sized triangles into leaves beside live ones, and sit next to either limit of
the 3-byte stack entry (Stack24: fewer than 2^16 nodes and fewer than 2^20 triangles).

The six small meshes draw from one default_rng(0) in the order of SMALL; small_meshes() builds them
all in that order, because each mesh's data depends on what the earlier ones drew.
"""
import functools

import numpy as np

f32 = np.float32
SMALL = ("geometric", "copies300", "degenerate", "huge_tiny", "coplanar_x2", "slivers")
# geometric_up: geometric without the 5 of its 2,080 triangles that have an edge component beyond 2^30,
# which an upload refuses (host/launch_plan.h kEdgeLimit); the same depth and stack bound.  The GPU
# tests run it in geometric's place, the host tests both.
HOST = SMALL + ("geometric_up",)
GPU = ("geometric_up",) + SMALL[1:]
TRUTH = ("geometric", "geometric_up", "huge_tiny", "degenerate", "slivers")  # checked against float64; the others are all ties
EDGE_LIMIT = 2.0 ** 30
LIMITS = ("nodes_65535", "nodes_65536", "tris_2p20m8")

# nodes_65535 / nodes_65536: prefixes of the 400,000-triangle soup (find_node_prefix searches them again)
SOUP_N, PREFIX_65535, PREFIX_65536 = 400_000, 293_922, 293_924
CLUSTERS_2P20M8 = 131_071  # tris_2p20m8: 8 per cluster, 2^20 - 8 triangles


def _wgt():
    import webgputracer_amd

    return webgputracer_amd


def tri_at(c, size, rng):
    """For each centre: v0 = c, v1 = v0 + N(0, 1)^3 size, v2 = v0 + N(0, 1)^3 size, (n, 3, 3) float32."""
    c = np.asarray(c, np.float64)
    size = np.asarray(size, np.float64).reshape(-1, 1) if np.ndim(size) else float(size)
    v1 = c + rng.normal(0.0, 1.0, c.shape) * size
    v2 = c + rng.normal(0.0, 1.0, c.shape) * size
    return np.stack([c, v1, v2], axis=1).astype(f32)


def _geometric(rng):
    x = np.repeat(1.1 ** np.arange(260), 8)
    c = np.stack([x, 0.3 * x, -0.2 * x], axis=1)
    return tri_at(c, 0.01 * x, rng)


def _copies300(rng):
    return np.tile(np.array([[[0, 0, 0], [10, 0, 0], [0, 10, 0]]], f32), (300, 1, 1))


def _degenerate(rng):
    v = tri_at(rng.uniform(0.0, 500.0, (500, 3)), 20.0, rng)
    v[0::3, 2] = v[0::3, 1]   # collinear: v2 = v1
    v[1::7, 1] = v[1::7, 0]   # a point: v1 = v2 = v0
    v[1::7, 2] = v[1::7, 0]
    return v


HUGE = np.array([[-1e4, 250, -1e4], [2e4, 250, -1e4], [-1e4, 250, 2e4]], f32)


def _huge_tiny(rng):
    v = tri_at(rng.uniform(0.0, 500.0, (3000, 3)), 0.5, rng)
    return np.concatenate([HUGE[None], v, (HUGE + f32([0, 1, 0]))[None]])


def _coplanar_x2(rng):
    i, j = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
    x, y = 16.0 * i.ravel(), 16.0 * j.ravel()
    z = np.full(x.size, 100.0)
    p00, p10 = np.stack([x, y, z], 1), np.stack([x + 16, y, z], 1)
    p11, p01 = np.stack([x + 16, y + 16, z], 1), np.stack([x, y + 16, z], 1)
    one = np.stack([np.stack([p00, p10, p11], 1), np.stack([p00, p11, p01], 1)], 1).reshape(-1, 3, 3)
    return np.concatenate([one, one]).astype(f32)


def _slivers(rng):
    o = rng.uniform(0.0, 500.0, (2000, 3))
    d = rng.normal(0.0, 1.0, (2000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    v1 = o + 400.0 * d
    return np.stack([o, v1, v1 + rng.normal(0.0, 0.05, (2000, 3))], axis=1).astype(f32)


@functools.lru_cache(maxsize=None)
def small_meshes():
    """name -> triangles (what make_triangles gives) of the six small meshes, from one default_rng(0)."""
    rng = np.random.default_rng(0)
    make = {"geometric": _geometric, "copies300": _copies300, "degenerate": _degenerate, "huge_tiny": _huge_tiny,
            "coplanar_x2": _coplanar_x2, "slivers": _slivers}
    out = {name: _wgt().make_triangles(make[name](rng)) for name in SMALL}
    g = out["geometric"]
    out["geometric_up"] = g[~((np.abs(g["e1"][:, :3]) > EDGE_LIMIT).any(1) | (np.abs(g["e2"][:, :3]) > EDGE_LIMIT).any(1))]
    return out


def small_mesh(name):
    return small_meshes()[name]


@functools.lru_cache(maxsize=None)
def _soup_400k():
    """test_bvh.random_soup's form, 400,000 triangles from default_rng(7), drawn once."""
    rng = np.random.default_rng(7)
    v0 = rng.uniform(0, 500.0, (SOUP_N, 3)).astype(f32)
    v = np.stack([v0, v0 + rng.normal(0, 20.0, (SOUP_N, 3)).astype(f32), v0 + rng.normal(0, 20.0, (SOUP_N, 3)).astype(f32)], 1)
    return _wgt().make_triangles(v)


def soup_prefix(n):
    return _soup_400k()[:n]


def find_node_prefix(target_nodes=65_535):
    """Search the prefix lengths again after a builder change: bisect the 400k soup for a prefix whose
    tree has about target_nodes nodes (the count grows with the prefix but not monotonically),
    then scan +-30 around it (about 80 builds, a few minutes).  -> {n_nodes: shortest prefix} for
    target_nodes and target_nodes + 1."""
    w = _wgt()
    lo, hi = 1, SOUP_N
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if w.bvh_build(soup_prefix(mid))[0]["bvh_nodes"] < target_nodes:
            lo = mid
        else:
            hi = mid
    found = {}
    for n in range(max(1, hi - 30), min(SOUP_N, hi + 30) + 1):
        k = w.bvh_build(soup_prefix(n))[0]["bvh_nodes"]
        if k in (target_nodes, target_nodes + 1):
            found.setdefault(k, n)
    return found


def clusters(n_clusters):
    """n_clusters clusters of 8 near-copies from default_rng(1): a centre in U(0, 555)^3, a base
    triangle centre + N(0, 1.5)^(3 x 3), and 8 copies of it + N(0, 0.01)."""
    rng = np.random.default_rng(1)
    c = rng.uniform(0.0, 555.0, (n_clusters, 1, 3))
    base = c + rng.normal(0.0, 1.5, (n_clusters, 3, 3))
    v = base[:, None, :, :] + rng.normal(0.0, 0.01, (n_clusters, 8, 3, 3))
    return _wgt().make_triangles(v.reshape(-1, 3, 3).astype(f32))


@functools.lru_cache(maxsize=None)
def limit_mesh(name):
    if name == "nodes_65535":
        return soup_prefix(PREFIX_65535)
    if name == "nodes_65536":
        return soup_prefix(PREFIX_65536)
    if name == "tris_2p20m8":
        return clusters(CLUSTERS_2P20M8)
    raise KeyError(name)


def aimed_rays(tris, n, seed):
    """n rays at interior points of random triangles: target = v0 + u e1 + v e2 with u in
    U(0.15, 0.7) and v in U(0.15, 0.85) (1 - u); origin = target + N(0, 1)^3 (0.2 |target| + 50);
    d = target - o.  length / size stays well inside the 1e5 of DESIGN.md 3.4."""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, len(tris), n)
    u = rng.uniform(0.15, 0.7, (n, 1))
    v = rng.uniform(0.15, 0.85, (n, 1)) * (1.0 - u)
    v0, e1, e2 = (tris[f][k, :3].astype(np.float64) for f in ("v0", "e1", "e2"))
    target = v0 + u * e1 + v * e2
    o = (target + rng.normal(0.0, 1.0, (n, 3)) * (0.2 * np.linalg.norm(target, axis=1, keepdims=True) + 50.0)).astype(f32)
    d = (target - o.astype(np.float64)).astype(f32)
    return o, d


# ------------------------------------------------------------------ the refs a traversal pushes
NOREF = 0x7FFFFFFF


def push_walk(tree, o, d):
    """tests/test_split_stack.py's Lane with the whole stack in LDS (the default, unparked
    k_render_ps: node_step, trav_resolve, tri_step of wgt_trav_ps.h), for all rays at once in numpy
    float64 over a test_split_stack.Tree.  A ray with a node to visit takes a node step, a ray with
    only an open leaf tests that leaf; any order is exact.  Checks on the way that every stack
    write lands below DevScene::stack (tree.stack).  Returns per ray:
      bt, bi     the closest hit (the model's float64 arithmetic; bi = 0xffffffff for a miss),
      max_node   the largest internal ref it pushed (advanced the top over), -1 for none,
      min_leaf   the smallest (most negative) leaf ref it pushed, 0 for none,
      depth      the highest stack top it reached."""
    import test_split_stack as ss

    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    R, S = len(o), tree.stack
    with np.errstate(divide="ignore"):
        inv = np.where(np.abs(d) < 2.0 ** -87, np.copysign(2.0 ** 87, d), 1.0 / d)
    stack = np.zeros((R, S), np.int64)
    sp = np.zeros(R, np.int64)
    ref = np.zeros(R, np.int64)
    lf, le = np.zeros(R, np.int64), np.zeros(R, np.int64)
    bt, bi = np.full(R, ss.RAY_MAX), np.full(R, 0xFFFFFFFF, np.int64)
    max_node, min_leaf, depth = np.full(R, -1, np.int64), np.zeros(R, np.int64), np.zeros(R, np.int64)
    refs_all = tree.refs.astype(np.int64)

    def push(k, v, really):
        """Lane.st(sp, v) for rays k, the top advancing where `really`."""
        assert (sp[k] < S).all(), "a stack write at or above DevScene::stack"
        stack[k, sp[k]] = v
        kk, vv = k[really], v[really]
        sp[kk] += 1
        depth[kk] = np.maximum(depth[kk], sp[kk])
        node = vv >= 0
        max_node[kk[node]] = np.maximum(max_node[kk[node]], vv[node])
        min_leaf[kk[~node]] = np.minimum(min_leaf[kk[~node]], vv[~node])

    def resolve(k, cand):
        cand = cand.copy()
        live = np.ones(len(k), bool)
        out = np.full(len(k), NOREF, np.int64)
        for _ in range(3):
            pop = live & (cand == NOREF)
            live &= ~(pop & (sp[k] == 0))
            pop &= live
            sp[k[pop]] -= 1
            cand[pop] = stack[k[pop], sp[k[pop]]]
            node = live & (cand >= 0)
            out[node] = cand[node]
            live &= ~node
            opens = live & (lf[k] >= le[k])
            u = (~cand[opens]) & 0xFFFFFFFF
            lf[k[opens]] = u >> 3
            le[k[opens]] = (u >> 3) + (u & 7) + 1
            cand[opens] = NOREF
            waits = live & ~opens
            push(k[waits], cand[waits], np.ones(int(waits.sum()), bool))
            live &= ~waits
        ref[k] = out

    for _ in range(100000):
        k = np.flatnonzero(ref != NOREF)
        if k.size:  # node_step
            r = ref[k]
            t0 = (tree.lo[r] - o[k, None, :]) * inv[k, None, :]
            t1 = (tree.hi[r] - o[k, None, :]) * inv[k, None, :]
            near = np.maximum(np.minimum(t0, t1).max(2), ss.RAY_MIN)
            far = np.minimum(np.maximum(t0, t1).min(2), bt[k, None])
            key = np.where(near <= far, near, np.inf)
            cr = refs_all[r]
            for a, b in ((0, 1), (2, 3), (0, 2)):
                sw = key[:, b] < key[:, a]
                key[sw, a], key[sw, b] = key[sw, b], key[sw, a]
                cr[sw, a], cr[sw, b] = cr[sw, b], cr[sw, a]
            for c in (3, 2, 1):
                push(k, cr[:, c], key[:, c] != np.inf)
            resolve(k, np.where(key[:, 0] != np.inf, cr[:, 0], NOREF))
        m = np.flatnonzero((ref == NOREF) & (lf < le))
        m = np.setdiff1d(m, k, assume_unique=True)  # one step per ray and round
        if m.size:  # tri_step, the whole open leaf
            j = lf[m, None] + np.arange(8)[None, :]
            ok = j < le[m, None]
            j = np.where(ok, j, lf[m, None])
            v0, e1, e2 = tree.v0[j], tree.e1[j], tree.e2[j]
            dd, oo = d[m, None, :], o[m, None, :]
            with np.errstate(all="ignore"):
                p = np.cross(dd, e2)
                det = np.einsum("ijk,ijk->ij", e1, p)
                tv = oo - v0
                u = np.einsum("ijk,ijk->ij", tv, p) / det
                q = np.cross(tv, e1)
                v = np.einsum("ijk,ijk->ij", np.broadcast_to(dd, q.shape), q) / det
                t = np.einsum("ijk,ijk->ij", e2, q) / det
                hit = ok & (np.abs(det) >= 1e-12) & (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= ss.RAY_MIN) & (t <= ss.RAY_MAX)
            idx = tree.idx[j].astype(np.int64)
            t = np.where(hit, t, np.inf)
            tm = t.min(1)
            im = np.where(t == tm[:, None], idx, 1 << 40).min(1)
            better = (tm < bt[m]) | ((tm == bt[m]) & (im < bi[m]))
            better &= np.isfinite(tm)
            bt[m[better]], bi[m[better]] = tm[better], im[better]
            lf[m] = le[m]
            resolve(m, np.full(m.size, NOREF, np.int64))
        if not k.size and not m.size:
            break
    else:
        raise AssertionError("the walk did not end")
    assert (sp == 0).all()
    return {"bt": bt, "bi": bi, "max_node": max_node, "min_leaf": min_leaf, "depth": depth}


# ------------------------------------------------------------------ trees and ray sets, built once
@functools.lru_cache(maxsize=None)
def built(name):
    """(info, nodes, recs) of wgt.bvh_build on the named mesh under the builder's defaults."""
    tris = small_mesh(name) if name in HOST else limit_mesh(name)
    return _wgt().bvh_build(tris)


@functools.lru_cache(maxsize=None)
def tree(name):
    import test_split_stack as ss

    return ss.Tree(None, built=built(name))


NODE_LIMIT = 65_024                    # 128-B byte offset >= 2^23 - 2^16
LEAF_LIMIT = -(1 << 23) + (1 << 12)    # leaf ref <= -2^23 + 2^12: the last 512 records


def limit_targets(name):
    """The triangles (indices into the mesh) to aim at so that a traversal pushes a ref at the
    3-byte entry's limit: those in the leaves under the last 512 nodes (node meshes), or in the
    last 512 leaf-ordered records (tris_2p20m8)."""
    info, nodes, recs = built(name)
    idx = recs[:, 0, 3].view(np.uint32)
    if name == "tris_2p20m8":
        return idx[-512:].astype(np.int64)
    refs = nodes[-512:, 6, :].view(np.int32).astype(np.int64)
    live = ~((nodes[-512:, 0, :] == f32(3e38)) & (nodes[-512:, 1, :] == f32(3e38)))
    out = []
    for r in refs[live & (refs < 0)]:
        u = (~r) & 0xFFFFFFFF
        out.append(idx[(u >> 3):(u >> 3) + (u & 7) + 1])
    return np.unique(np.concatenate(out)).astype(np.int64)


def at_limit(name, walk):
    """Per ray of a push_walk: did it push a ref at the limit?"""
    return walk["min_leaf"] <= LEAF_LIMIT if name == "tris_2p20m8" else walk["max_node"] >= NODE_LIMIT


@functools.lru_cache(maxsize=None)
def limit_rays(name, n=1000, seed=9):
    """n rays at limit_targets(name), from random sides (aimed_rays' recipe)."""
    tris = limit_mesh(name)
    return aimed_rays(tris[limit_targets(name)], n, seed)


def scene_parts(name):
    """What a mesh is uploaded with besides its triangles: the Cornell light, Q[:5] and the dummy
    sphere; for geometric the light and a far sphere only (f64_truth.tri_scene(far_sphere=True)),
    so that no wall cuts the rays."""
    import f64_truth as ft

    L, Q, S = _wgt().cornell_scene()
    if name.startswith("geometric"):
        L, S = ft.tri_scene(far_sphere=True)
        return L, Q[:0].copy(), S
    return L, Q[:5].copy(), S


# ------------------------------------------------------------------ cameras
W, H, SPP = 48, 27, 4


def _cam(origin, target, fovy, seed):
    cam = _wgt().camera_param(W / H, SPP, seed, fovy=fovy)
    cam["origin"], cam["target"] = origin, target
    return cam


def cameras(name):
    """[(tag, camera)] of the 48 x 27 / 4 spp frames of a small mesh, each chosen so that at least
    30 % of the pixels' first hits are on the mesh."""
    if name.startswith("geometric"):
        # the centres lie on the line x (1, 0.3, -0.2): from beyond the far end looking down the
        # progression, and from behind the first centre looking outwards.  Each target is a short way
        # in front of its camera: a pixel's ray is as long as the focal distance, a render refuses
        # primary directions beyond 2^32 (host/launch_plan.h), and beyond |d| |o - c| = 1.8e19 the
        # dummy sphere's discriminant overflows (f64_truth.sphere_terms)
        line = np.array([1.0, 0.3, -0.2])
        last = 1.1 ** 259 * line
        far, unit = 1.1 * last, line / np.linalg.norm(line)
        return [("far", _cam(far, far - 1e8 * unit, 5.0, 5)), ("near", _cam(-2.0 * line, -2.0 * line + 1e3 * unit, 1.5, 6))]
    if name == "copies300":
        return [("front", _cam((4.0, 4.0, -10.0), (4.0, 4.0, 0.0), 40.0, 7))]
    if name == "degenerate":
        # 20 in front of triangle 2 (a live one), the rest of the soup behind it
        t = small_mesh("degenerate")[2]
        v0, e1, e2 = (t[f][:3].astype(np.float64) for f in ("v0", "e1", "e2"))
        c, n = v0 + (e1 + e2) / 3.0, np.cross(e1, e2)
        return [("close", _cam(c + 20.0 * n / np.linalg.norm(n), c, 40.0, 8))]
    if name == "huge_tiny":
        return [("above", _cam((250.0, 420.0, -250.0), (250.0, 250.0, 250.0), 50.0, 9))]
    if name == "coplanar_x2":
        return [("front", _cam((256.0, 256.0, -500.0), (256.0, 256.0, 100.0), 40.0, 10))]
    if name == "slivers":
        # beside the middle of sliver 0 (0.05 wide), one unit away
        t = small_mesh("slivers")[0]
        v0, e1, e2 = (t[f][:3].astype(np.float64) for f in ("v0", "e1", "e2"))
        mid = v0 + 0.5 * e1 + 0.25 * (e2 - e1)
        n = np.cross(e1, e2)
        return [("beside", _cam(mid + n / np.linalg.norm(n), mid, 2.0, 11))]
    raise KeyError(name)
