"""wgt_bvh_build_morton, the host specification of a rebuild, on the CPU.

Its topology is compared with the numpy statement (tests/rebuild_restatement.py), its boxes with
refit_cases.expected_nodes and its compact codes with refit_cases.compact_margin_violations, on the
meshes of tests/rebuild_cases.py, for the leaf targets 1, 4 and 8.  No GPU is needed: the device
build is compared with this specification in tests/test_gpu_rebuild.py.  The cases at scale
(rebuild_cases.SCALE) are shown here to meet the conditions they are built for; the device runs them in
tests/test_gpu_rebuild_scale.py.
"""
import numpy as np
import pytest

import rebuild_cases as cases
import rebuild_restatement as rr
import refit_cases as rc

LEAVES = (1, 4, 8)
# every case at every leaf target, and the one case at scale that is restated (65,495 nodes)
RESTATED = [(name, L) for L in LEAVES for name in cases.CASES] + [("nodes_below", 1)]
RESEARCH = "rebuild_cases.find_leaf1_prefixes() searches the prefix lengths again"


def _tree(wgt, monkeypatch, name, L):
    monkeypatch.setenv("WGT_REBUILD_LEAF", str(L))
    T = cases.case(name, L)
    return (T,) + wgt.bvh_build_morton(T)


@pytest.mark.parametrize("name,L", RESTATED)
def test_topology_equals_the_restatement(wgt, monkeypatch, name, L):
    """Refs, leaf order, stack need, depth and the counts are the numpy statement's."""
    T, info, nodes, recs, cn, cr, step = _tree(wgt, monkeypatch, name, L)
    order, refs, live, level, stack_need, depth, leaves = rr.tree(T, L)
    assert np.array_equal(rc.bits(recs[:, 0, 3]), order), "leaf order"
    assert np.array_equal(rc.refs_of(nodes), refs), "refs"
    assert np.array_equal(cr, refs), "compact refs"
    assert np.array_equal(rc.live_slots(nodes).sum(1), live), "live slots"
    assert not rc.live_slots(nodes)[np.arange(4)[None, :] >= np.array(live)[:, None]].any(), "live slots come first"
    assert info["bvh_nodes"] == len(refs) and info["bvh_leaves"] == len(leaves)
    assert info["bvh_max_leaf"] == max(c for _, c in leaves)
    assert info["bvh_max_depth"] == depth <= rr.LEVELS
    assert info["bvh_stack"] == stack_need <= 31
    assert info["n_tris"] == len(T) and info["bvh_width"] == 4
    assert info["sah_cost"] == 0.0 and info["bvh2_nodes"] == 0 and info["bvh2_depth"] == 0
    # nodes are numbered level by level
    assert level == sorted(level)


@pytest.mark.parametrize("name,L", RESTATED)
def test_tree_is_well_formed(wgt, monkeypatch, name, L):
    """Every triangle in exactly one leaf of at most L, refs forward and in range, the boxes the exact
    unions of the records', the compact codes with their margin."""
    T, info, nodes, recs, cn, cr, step = _tree(wgt, monkeypatch, name, L)
    n, refs, live = len(T), rc.refs_of(nodes), rc.live_slots(nodes)
    assert sorted(rc.bits(recs[:, 0, 3]).tolist()) == list(range(n)), "the records hold a permutation"
    seen = np.zeros(n, np.int64)
    for k in range(len(nodes)):
        for s in range(4):
            if not live[k, s]:
                assert refs[k, s] == refs[k, 0] and np.all(nodes[k, :6, s] == rc.EMPTY)
                continue
            r = int(refs[k, s])
            if r < 0:
                u = ~r & 0xFFFFFFFF
                first, cnt = u >> 3, (u & 7) + 1
                assert cnt <= L and first + cnt <= n
                seen[first:first + cnt] += 1
            else:
                assert k < r < len(nodes)
    assert np.all(seen == 1), "every triangle in exactly one leaf"
    lo, hi = rc.tri_boxes(T)
    idx = rc.bits(recs[:, 0, 3])
    assert np.array_equal(rc.bits(recs[:, 1, 3]), rc.bits(lo[idx, 0])) and np.array_equal(rc.bits(recs[:, 3, 1:4]), rc.bits(hi[idx]))
    assert np.array_equal(rc.bits(nodes), rc.bits(rc.expected_nodes(nodes, recs))), "boxes"
    assert np.all(nodes[:, 7, :] == 0.0)
    assert rc.compact_margin_violations(nodes, cn, step, 4.0 * rc.extent(T)) == 0
    assert info["bvh_compact_step"] == step


def test_leaf_knob_is_clamped(wgt, monkeypatch):
    T = cases.case("bunny2000")
    want = {"0": 1, "1": 1, "8": 8, "9": 8, "": 4}
    for value, L in want.items():
        monkeypatch.setenv("WGT_REBUILD_LEAF", value)
        info = wgt.bvh_build_morton(T)[0]
        assert info["bvh_max_leaf"] <= L
        assert info["bvh_nodes"] == len(rr.tree(T, L)[1]), value


def test_the_restatement_meets_the_median_fallback_and_equal_codes():
    """The cases reach what they are there for: chain needs the median (its highest-bit split alone would
    exceed the depth budget), same64 has one code, sheet one axis without extent."""
    assert len(set(rr.codes(cases.case("same64")))) == 1
    assert np.all(rr.cells(cases.case("sheet"))[:, 1] == 0) and len(set(rr.codes(cases.case("sheet")))) > 100
    _, code = rr.leaf_order(cases.case("chain"))

    def depth_without_median(b, e):
        if e - b <= cases.LEAF or code[b] == code[e - 1]:
            return 0
        h = (code[b] ^ code[e - 1]).bit_length() - 1
        p = next(i for i in range(b, e) if (code[i] >> h) & 1)
        return 1 + max(depth_without_median(b, p), depth_without_median(p, e))

    assert depth_without_median(0, len(code)) > 2 * rr.LEVELS


def test_too_many_triangles_is_a_planning_refusal(wgt, monkeypatch):
    """n = L * 4^10 + 1 is refused by the check that the calls make before they read a record: the
    pointer is never dereferenced, so no such mesh is built."""
    import ctypes

    from webgputracer_amd import _lib

    lib = _lib.lib()
    one = cases.case("one")
    info = _lib.WgtSceneInfo()
    step = ctypes.c_float(0.0)
    for leaf in LEAVES:
        monkeypatch.setenv("WGT_REBUILD_LEAF", str(leaf))
        n = rr.max_tris(leaf) + 1
        rcode = lib.wgt_bvh_build_morton(_lib.ptr(one), n, None, 0, None, None, None, ctypes.byref(step), ctypes.byref(info))
        assert rcode == _lib.WGT_E_INVALID
        assert b"too many triangles for a rebuild" in lib.wgt_last_error(None)


# ------------------------------------------------------------------ the cases at scale meet their conditions
def test_grid4096_has_a_level_of_exactly_256_nodes():
    """Balanced at L = 4: the levels have 1, 4, 16, 64 and 256 nodes, so the last level's list fills one
    256-lane block and the count kernel's extra lane (j == count) falls into a block of its own."""
    T = cases.case("grid4096")
    assert len(T) == 4096
    for L, want in ((1, [1, 4, 16, 64, 256, 1024]), (4, [1, 4, 16, 64, 256]), (8, [1, 4, 16, 64, 256])):
        level = rr.tree(T, L)[3]
        assert np.bincount(level).tolist() == want, L


def test_soup100k_reaches_the_level_cap():
    info = cases.spec("soup100k")[0]
    print(f"soup100k: {info['bvh_nodes']} nodes, depth {info['bvh_max_depth']}, stack {info['bvh_stack']}")
    assert info["n_tris"] == cases.SOUP100K and info["bvh_max_depth"] == rr.LEVELS == 10 and info["bvh_stack"] >= 25
    sizes = cases.level_sizes(cases.spec("soup100k")[1])
    print(f"soup100k: level sizes {sizes}")
    assert len(sizes) == 10 and max(sizes) > 16 * 256  # level lists of many blocks, a scan over more than one


def test_node_limit_prefixes():
    """nodes_below keeps the 3-byte stack entry (6 waves) with nodes beyond adversarial_meshes.NODE_LIMIT;
    nodes_above loses it (5 waves) and its last 512 nodes all lie beyond 2^16."""
    below, above = cases.spec("nodes_below")[0], cases.spec("nodes_above")[0]
    got = (below["n_tris"], below["bvh_nodes"], above["n_tris"], above["bvh_nodes"])
    assert got == (cases.PREFIX_BELOW, cases.NODES_BELOW, cases.PREFIX_ABOVE, cases.NODES_ABOVE), (got, RESEARCH)
    assert 65_024 <= below["bvh_nodes"] <= 65_535 and above["bvh_nodes"] >= 66_048, RESEARCH
    assert (below["ps_waves"], above["ps_waves"]) == (6, 5)
    for info in (below, above):
        print(f"{info['n_tris']} triangles: {info['bvh_nodes']} nodes, depth {info['bvh_max_depth']}, stack {info['bvh_stack']}")
        assert info["bvh_max_leaf"] == 1 and info["bvh_max_depth"] == 10 and info["bvh_stack"] <= 31


def test_tris_2p20p8_copies_and_order():
    """2^20 + 8 triangles in clusters of 8 exact copies whose indices lie 2^17 apart; the specification
    keeps the original indices ascending within every run of equal codes and gives 5 waves."""
    T = cases.case("tris_2p20p8")
    n = (1 << 20) + 8
    assert len(T) == n > 1 << 20
    geom = np.concatenate([T["v0"][:, :3], T["e1"][:, :3], T["e2"][:, :3]], 1)
    first = cases.cluster_first(np.arange(n))
    assert np.array_equal(rc.bits(geom), rc.bits(geom[first])), "copies are exact"
    assert np.array_equal(np.bincount(first, minlength=n)[np.unique(first)], np.full(cases.CLUSTERS_2P20P8, 8))
    assert np.array_equal(first[:1 << 20], np.arange(1 << 20) % cases.COPY_STRIDE) and first[-1] == 1 << 20
    info, nodes, recs = cases.spec("tris_2p20p8")[:3]
    assert info["ps_waves"] == 5 and info["bvh_nodes"] < 1 << 20 and info["bvh_max_leaf"] <= 4
    idx = rc.bits(recs[:, 0, 3]).astype(np.int64)
    same = first[idx[1:]] == first[idx[:-1]]  # neighbours in leaf order from one cluster: equal codes
    assert same.sum() >= 7 * (cases.CLUSTERS_2P20P8 - 100), "clusters stay together"
    assert (idx[1:][same] > idx[:-1][same]).all()
    refs, live = rc.refs_of(nodes), rc.live_slots(nodes)
    assert refs[live].min() <= cases.OVER["tris_2p20p8"]
    print(f"tris_2p20p8: {info['bvh_nodes']} nodes, depth {info['bvh_max_depth']}, stack {info['bvh_stack']}, "
          f"smallest leaf ref {refs[live].min()}")


@pytest.mark.parametrize("name", ["nodes_above", "nodes_below", "tris_2p20p8"])
def test_limit_rays_push_refs_beyond_the_3_byte_entry(name):
    """What makes tests/test_gpu_rebuild_scale.py able to fail, from the host: at least 100 of the limit
    rays, and for the node cases at least 100 primary rays of the limit frame (test_gpu_gbuffer's
    restatement of the camera rays), push a ref that a 3-byte entry would cut (nodes_below: one at
    adversarial_meshes.NODE_LIMIT or later)."""
    import adversarial_meshes as am
    from test_gpu_gbuffer import camera_rays

    tree = cases.spec_tree(name)
    o, d = cases.limit_rays(name)
    walk = am.push_walk(tree, o, d)
    n = int(cases.over_limit(name, walk).sum())
    print(f"{name}: {n} of {len(o)} limit rays push such a ref; largest node {walk['max_node'].max()}, smallest leaf ref "
          f"{walk['min_leaf'].min()}, deepest top {walk['depth'].max()} of {tree.stack}")
    assert n >= 100
    if name != "tris_2p20p8":
        ro, rd = camera_rays(cases.limit_camera(name), am.W, am.H)
        walk = am.push_walk(tree, ro.reshape(-1, 3), rd.reshape(-1, 3))
        n = int(cases.over_limit(name, walk).sum())
        print(f"{name}: {n} of {am.W * am.H} primary rays of the limit frame push such a ref")
        assert n >= 100
