"""Meshes for the rebuild tests.  TEST INFRASTRUCTURE ONLY.

Shared by tests/test_rebuild_host.py (wgt_bvh_build_morton against tests/rebuild_restatement.py, on
the CPU) and tests/test_gpu_rebuild.py (wgt_rebuild_triangles against wgt_bvh_build_morton).  Each
mesh is the smallest at which one step of the build can go wrong; the largest of CASES has 4096
triangles.  SCALE holds what only happens at scale (tests/test_gpu_rebuild_scale.py): levels 8 to 10
and level lists of 10^4 nodes, the node and triangle limits of the 3-byte stack entry, and the sort
for more than 2^20 keys.
"""
import contextlib
import functools
import os

import numpy as np

import adversarial_meshes as am
import refit_cases as rc

f32 = np.float32
LEAF = 4  # the default leaf target (wgt_morton.h kRebuildLeafDefault)

# leaf and level edges for the leaf target L, the 256-lane block's edge, then the shaped meshes
COUNTS = ("n1", "n2", "nL", "nL+1", "n4L", "n4L+1", "n16L+1", "n255", "n256", "n257")
SHAPED = ("one", "nine", "bunny2000", "chain", "same64", "sheet", "tiny", "huge", "grid4096")
CASES = COUNTS + SHAPED

# The cases at scale, each with the leaf target it is built for.  They are no part of CASES: the device
# is compared with the specification on them in tests/test_gpu_rebuild_scale.py, and of the four only
# nodes_below is restated in numpy (tests/test_rebuild_host.py).
SCALE = {"soup100k": 4, "nodes_below": 1, "nodes_above": 1, "tris_2p20p8": 4}
SOUP100K = 100_000  # the shortest prefix of the soup, in steps of 10,000, of depth 10 and stack need >= 25 at L = 4
# prefixes of the 400,000-triangle soup at L = 1 (find_leaf1_prefixes searches them again): the tree of
# nodes_below has 65,024..65,535 nodes, the last ones the 3-byte stack entry holds; nodes_above's has at
# least 66,048, so that its last 512 nodes all lie beyond 2^16
PREFIX_BELOW, PREFIX_ABOVE = 131_400, 132_600
NODES_BELOW, NODES_ABOVE = 65_495, 66_052
CLUSTERS_2P20P8 = 131_073  # tris_2p20p8: 8 exact copies per cluster, 2^20 + 8 triangles
COPY_STRIDE = 1 << 17      # the distance between two copies' indices


def _wgt():
    import webgputracer_amd

    return webgputracer_amd


def count_of(name, L):
    """The triangle count of a COUNTS case for the leaf target L."""
    return {"n1": 1, "n2": 2, "nL": L, "nL+1": L + 1, "n4L": 4 * L, "n4L+1": 4 * L + 1, "n16L+1": 16 * L + 1,
            "n255": 255, "n256": 256, "n257": 257}[name]


@functools.lru_cache(maxsize=None)
def case(name, L=LEAF):
    """Triangles (TRI_DTYPE) of one case."""
    w = _wgt()
    if name in COUNTS:  # the first n triangles of the bunny
        return rc.mesh("bunny2000")[:count_of(name, L)].copy()
    if name in rc.MESHES:
        return rc.mesh(name)
    if name == "same64":  # all codes equal: the order is the indices', every split the median
        return np.repeat(rc.mesh("one"), 64)
    if name == "sheet":  # a coplanar sheet: every centre has the same y, so that axis has no extent
        g = np.arange(12, dtype=np.float64) * 20.0
        x, z = [a.reshape(-1) for a in np.meshgrid(g, g)]
        y = np.full_like(x, 100.0)
        v0 = np.stack([x, y, z], 1)
        v = np.stack([v0, v0 + [15.0, 0.0, 0.0], v0 + [0.0, 0.0, 15.0]], 1)
        return w.make_triangles(v.astype(f32))
    if name in ("tiny", "huge"):  # the bunny scaled by 2^-12 and by 2^20: the compact step moves
        return w.make_triangles((rc.vertices(rc.mesh("bunny2000")) * (2.0 ** -12 if name == "tiny" else 2.0 ** 20)).astype(f32))
    if name == "grid4096":  # a 16 x 16 x 16 lattice: balanced at L = 4, so one level has exactly 256 nodes
        g = np.arange(16, dtype=np.float64) * 30.0 + 20.0
        v0 = np.stack([a.reshape(-1) for a in np.meshgrid(g, g, g, indexing="ij")], 1)
        v = np.stack([v0, v0 + [4.0, 0.0, 1.0], v0 + [0.0, 4.0, 2.0]], 1)
        return w.make_triangles(v.astype(f32))
    if name == "soup100k":
        return am.soup_prefix(SOUP100K)
    if name == "nodes_below":
        return am.soup_prefix(PREFIX_BELOW)
    if name == "nodes_above":
        return am.soup_prefix(PREFIX_ABOVE)
    if name == "tris_2p20p8":
        return exact_clusters(CLUSTERS_2P20P8)
    raise KeyError(name)


def exact_clusters(n_clusters):
    """adversarial_meshes.clusters' centres and base triangles (default_rng(1)), the 8 members of a
    cluster exact copies of its base.  Copy j of cluster c < 2^17 has the index j 2^17 + c, so equal
    codes meet the sort with their indices 2^17 apart; the copies of the clusters from 2^17 on follow
    at the end, cluster by cluster."""
    rng = np.random.default_rng(1)
    c = rng.uniform(0.0, 555.0, (n_clusters, 1, 3))
    base = (c + rng.normal(0.0, 1.5, (n_clusters, 3, 3))).astype(f32)
    return _wgt().make_triangles(np.concatenate([np.tile(base[:COPY_STRIDE], (8, 1, 1)), np.repeat(base[COPY_STRIDE:], 8, axis=0)]))


def cluster_first(i):
    """The lowest index among the exact copies of tris_2p20p8's triangle i: what the tie rule answers."""
    i = np.asarray(i, np.int64)
    n = COPY_STRIDE * 8
    return np.where(i < n, i % COPY_STRIDE, n + (i - n) // 8 * 8)


def find_leaf1_prefixes(step=100):
    """Search PREFIX_BELOW and PREFIX_ABOVE again after a change of the build or of the soup, in the style
    of adversarial_meshes.find_node_prefix: bisect the soup for the prefix at which the specification's
    tree at L = 1 passes 65,535 nodes (the count grows with the prefix, not monotonically), then scan
    multiples of `step` around it.  -> ((prefix, nodes) below, (prefix, nodes) above): the longest
    scanned prefix before the first with more than 65,535 nodes, and the shortest with at least 66,048."""
    w = _wgt()

    def nodes(n):
        return w.bvh_build_morton(am.soup_prefix(n))[0]["bvh_nodes"]

    with leaf_target(1):
        lo, hi = 1, am.SOUP_N
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if nodes(mid) <= 65_535 else (lo, mid)
        below = above = None
        for n in range((hi // step - 20) * step, (hi // step + 40) * step, step):
            k = nodes(n)
            if k > 65_535 and below is None:
                below = (n - step, nodes(n - step))
            if k >= 66_048:
                above = (n, k)
                break
    return below, above


@contextlib.contextmanager
def leaf_target(L):
    """WGT_REBUILD_LEAF = L within the block: the specification and the rebuild read it on every call."""
    old = os.environ.get("WGT_REBUILD_LEAF")
    os.environ["WGT_REBUILD_LEAF"] = str(L)
    try:
        yield
    finally:
        if old is None:
            del os.environ["WGT_REBUILD_LEAF"]
        else:
            os.environ["WGT_REBUILD_LEAF"] = old


@functools.lru_cache(maxsize=None)
def spec(name, L=None):
    """wgt_bvh_build_morton of a case (info, nodes, recs, cnodes, crefs, step), computed once; a SCALE case
    at its own leaf target."""
    L = SCALE.get(name, LEAF) if L is None else L
    with leaf_target(L):
        return _wgt().bvh_build_morton(case(name, L))


def level_sizes(nodes):
    """Nodes per level of exported nodes, from the refs alone (they point forward)."""
    refs, live = rc.refs_of(nodes), rc.live_slots(nodes)
    level = np.zeros(len(nodes), np.int64)
    for k in range(len(nodes)):
        r = refs[k][live[k] & (refs[k] >= 0)]
        level[r] = level[k] + 1
    return np.bincount(level).tolist()


@functools.lru_cache(maxsize=None)
def spec_tree(name, L=None):
    """The specification's tree as adversarial_meshes.push_walk takes it."""
    import test_split_stack as ss

    return ss.Tree(None, built=spec(name, L)[:3])


# ------------------------------------------------------------------ refs that 3 bytes cannot hold
# What a traversal of the case must push for the test to be able to fail: kept at 6 waves, nodes_above's
# refs from 2^16 on and tris_2p20p8's leaf refs from record 2^20 on would be cut; nodes_below's last
# nodes are the last the entry holds (adversarial_meshes.NODE_LIMIT).
OVER = {"nodes_above": 1 << 16, "nodes_below": am.NODE_LIMIT, "tris_2p20p8": -(1 << 23)}


def over_limit(name, walk):
    """Per ray of a push_walk over spec_tree(name): did it push such a ref?"""
    return walk["min_leaf"] <= OVER[name] if name == "tris_2p20p8" else walk["max_node"] >= OVER[name]


@functools.lru_cache(maxsize=None)
def limit_targets(name, last=512):
    """adversarial_meshes.limit_targets on the specification's tree: the triangles under its last 512
    nodes, or those of its last 512 leaf-ordered records (tris_2p20p8)."""
    _, nodes, recs = spec(name)[:3]
    idx = rc.bits(recs[:, 0, 3])
    if name == "tris_2p20p8":
        return idx[-last:].astype(np.int64)
    refs, live = rc.refs_of(nodes[-last:]).astype(np.int64), rc.live_slots(nodes[-last:])
    u = (~refs[live & (refs < 0)]) & 0xFFFFFFFF
    return np.unique(np.concatenate([idx[f:f + c] for f, c in zip(u >> 3, (u & 7) + 1)])).astype(np.int64)


@functools.lru_cache(maxsize=None)
def limit_rays(name, n=1000, seed=9):
    """n rays at limit_targets(name) from random sides.  Of tris_2p20p8's records only the last 8 (one
    cluster, two leaves at L = 4) begin at 2^20 or later, so that case gets 200 more rays at those."""
    T = case(name)
    o, d = am.aimed_rays(T[limit_targets(name)], n, seed)
    if name == "tris_2p20p8":
        o2, d2 = am.aimed_rays(T[limit_targets(name, 8)], 200, seed + 1)
        o, d = np.concatenate([o, o2]), np.concatenate([d, d2])
    return o, d


def limit_camera(name):
    """At the centre of the limit targets' bounding box, looking at the mean corner of the triangles under
    the last 128 nodes.  (From 0.3 of the way through the box, as test_gpu_adversarial._limit_camera
    stands, fewer than 100 primary rays push a ref at the limit: test_rebuild_host.py counts them.)"""
    v0 = case(name)["v0"][:, :3].astype(np.float64)
    box = v0[limit_targets(name)]
    return am._cam((box.min(0) + box.max(0)) / 2, v0[limit_targets(name, 128)].mean(0), 40.0, 12)


@functools.lru_cache(maxsize=None)
def permuted(seed=12):
    """bunny2000 with its triangles' positions permuted among the indices: triangle i lies where triangle
    perm[i] lay, so every node of a tree refit to it spans the mesh."""
    A = rc.mesh("bunny2000")
    return A[np.random.default_rng(seed).permutation(len(A))].copy()
