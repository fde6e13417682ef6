"""The builder, the split-stack model and the oracle on the meshes of tests/adversarial_meshes.py
(CPU only).  tests/test_bvh.py walks benign trees; here the depth-limited median fallback runs, the
stack bound is met exactly (kStackMax = 31), leaves hold zero-area triangles and exact duplicates
beside live triangles, two triangles are larger than the scene, and three trees sit next to either
limit of the 3-byte stack entry (host/launch_plan.cpp ps_form_for: fewer than 2^16 nodes and fewer
than 2^20 triangles give 6 waves per SIMD).

What is checked, per mesh: test_bvh.check_tree and check_compact; the property the mesh is built
for; the oracle's BVH against its brute-force scan bit for bit; the oracle against float64
geometry (tests/f64_truth.py) where rays can be decided; the split-stack model of
tests/test_split_stack.py at the whole-stack-in-LDS form and at the smallest LDS stack; and, for
the limit meshes, that the ray sets tests/test_gpu_adversarial.py traces really push refs at the
limit (adversarial_meshes.push_walk).  Each test prints its figures.
"""
import numpy as np
import pytest

import adversarial_meshes as am
import f64_truth as ft
import test_split_stack as ss
import webgputracer_amd as w
from test_bvh import EMPTY, check_compact, check_tree, stack24_roundtrip

f32 = np.float32
NO_HIT = 0xFFFFFFFF
# required shares of decided rays (2,000 aimed_rays, seed 5): degenerate and slivers are undecided by
# construction (the aim lands on zero-area triangles and on 0.05-wide ones)
SHARE = {"geometric": 0.95, "geometric_up": 0.95, "huge_tiny": 0.95, "degenerate": 0.60, "slivers": 0.60}
RESEARCH = "adversarial_meshes.find_node_prefix() searches the prefix lengths again"


@pytest.fixture(scope="module")
def aimed():
    """name -> the 3,000 aimed rays (seed 3) of each small mesh."""
    return {name: am.aimed_rays(am.small_mesh(name), 3000, 3) for name in am.HOST}


def _oracle_scene(oracle, name):
    L, Q, S = am.scene_parts(name)
    return oracle.OracleScene(L, Q[:0], S, am.small_mesh(name)), len(L)


def _leaves(nodes):
    """(first, count) of every leaf ref of exported nodes."""
    refs = nodes[:, 6, :].view(np.int32).astype(np.int64)
    live = ~((nodes[:, 0, :] == EMPTY) & (nodes[:, 1, :] == EMPTY))
    u = (~refs[live & (refs < 0)]) & 0xFFFFFFFF
    return u >> 3, (u & 7) + 1


def _property(name, tris, info, nodes, recs, tid):
    """The third column of the issue's table; tid: the oracle's brute-force winners on the aimed rays."""
    hit = tid != NO_HIT
    if name.startswith("geometric"):
        # the depth limit is reached (the median fallback ran) and the stack bound met exactly
        assert info["bvh2_depth"] == 24 and info["bvh_stack"] == 31  # kStackMax
        assert (len(tris), info["bvh_nodes"]) == ((2080, 680) if name == "geometric" else (2075, 679)) and info["ps_waves"] == 6
        edge = max(np.abs(tris["e1"][:, :3]).max(), np.abs(tris["e2"][:, :3]).max())
        assert (edge <= am.EDGE_LIMIT) == (name == "geometric_up")  # what an upload accepts
    elif name == "copies300":
        assert hit.all() and (tid == 0).all()  # all ties: the lowest index wins
    elif name == "degenerate":
        e1, e2 = recs[:, 1, :3].astype(np.float64), recs[:, 2, :3].astype(np.float64)
        dead = np.linalg.norm(np.cross(e1, e2), axis=1) == 0.0
        point = (e1 == 0).all(1) & (e2 == 0).all(1)
        assert dead.sum() == 167 + 72 - 24 and point.sum() == 72  # every 3rd, every 7th from 1, 24 both
        lo = np.stack([recs[:, 1, 3], recs[:, 2, 3], recs[:, 3, 0]], 1)
        hi = recs[:, 3, 1:4]
        assert ((hi - lo)[point] < 0.05).all()  # a point's box is its padding
        first, count = _leaves(nodes)
        mixed = sum(1 for f, c in zip(first, count) if dead[f:f + c].any() and not dead[f:f + c].all())
        print(f"degenerate: {dead.sum()} zero-area records ({point.sum()} points), {mixed} leaves hold them beside live triangles")
        assert mixed >= 1
        idx = recs[:, 0, 3].view(np.uint32)
        # a point's determinant is exactly zero: never hit.  A collinear triangle's (e1 == e2) is a
        # rounding residue that can pass the |det| >= 1e-12 rule; float64 leaves such rays undecided
        assert not np.isin(tid[hit], idx[point]).any()
        print(f"degenerate: {int(np.isin(tid[hit], idx[dead]).sum())} of {int(hit.sum())} hits are on collinear triangles")
    elif name == "huge_tiny":
        assert info["bvh_stack"] == 23
        idx = recs[:, 0, 3].view(np.uint32)
        lo = np.stack([recs[:, 1, 3], recs[:, 2, 3], recs[:, 3, 0]], 1)
        hi = recs[:, 3, 1:4]
        big = np.isin(idx, [0, len(tris) - 1])
        assert big.sum() == 2
        for k in np.flatnonzero(big):  # in x and z the two boxes contain the whole scene
            assert (lo[k, [0, 2]] <= lo[~big][:, [0, 2]].min(0)).all() and (hi[k, [0, 2]] >= hi[~big][:, [0, 2]].max(0)).all()
        assert np.isin([0, len(tris) - 1], tid).all()  # and both are closest hits of some rays
    elif name == "coplanar_x2":
        lo, hi = nodes[:, 4, :], nodes[:, 5, :]
        live = ~((nodes[:, 0, :] == EMPTY) & (nodes[:, 1, :] == EMPTY))
        assert ((hi - lo)[live] < 0.05).all()  # every box is flat in z: its padding alone
        v = np.stack([tris["v0"], tris["e1"], tris["e2"]], 1)
        assert np.array_equal(v[:2048], v[2048:])
        assert hit.all() and (tid < 2048).all()  # of two exact duplicates the lower index
    elif name == "slivers":
        assert info["bvh_stack"] == 27
        e1, e2 = tris["e1"][:, :3].astype(np.float64), tris["e2"][:, :3].astype(np.float64)
        area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
        ext = np.maximum(np.abs(e1), np.abs(e2))
        box = 2 * (ext[:, 0] * ext[:, 1] + ext[:, 1] * ext[:, 2] + ext[:, 2] * ext[:, 0])
        vol = ext.prod(1)
        print(f"slivers: median box area / triangle area {np.median(box / area):.3g}, box volume / area {np.median(vol / area):.3g}")
        # a 400-unit edge in a random direction spans a box of about 400^2 x 0.6 in area beside a
        # triangle of about 400 x 0.05 / 2: four orders of magnitude
        assert np.median(box / area) > 3e3


@pytest.mark.parametrize("name", am.HOST)
def test_small_mesh_tree_and_oracle(oracle, aimed, name):
    """The exported tree passes the full walk and the compact-code check, the mesh has the property it
    is built for, and the oracle's BVH equals its brute-force scan bit for bit on 3,000 aimed rays."""
    tris = am.small_mesh(name)
    info = check_tree(tris)
    check_compact(tris)
    _, nodes, recs = am.built(name)
    assert am.built(name)[0] == info
    o, d = aimed[name]
    osc, _ = _oracle_scene(oracle, name)
    res = {}
    for brute in (True, False):
        tid, t = osc.trace_tris(o, d, brute=brute)
        prim, dist = osc.trace(o, d, brute=brute)
        res[brute] = (tid, t.view(np.uint32), prim, dist.view(np.uint32))
    for a, b in zip(res[True], res[False]):
        assert np.array_equal(a, b)
    tid = res[True][0]
    print(f"{name}: {len(tris)} triangles, depth {info['bvh2_depth']}, stack {info['bvh_stack']}, nodes {info['bvh_nodes']}, "
          f"waves {info['ps_waves']}, aimed rays that hit a triangle {np.mean(tid != NO_HIT):.3f}")
    _property(name, tris, info, nodes, recs, tid)


@pytest.mark.parametrize("name", am.TRUTH)
def test_small_mesh_oracle_vs_float64(oracle, name):
    """The oracle's closest triangle on 2,000 aimed rays (seed 5) against a float64 scan: the exact
    triangle on every decided ray and t within check_closest's 4 E_t, brute force and BVH."""
    tris = am.small_mesh(name)
    o, d = am.aimed_rays(tris, 2000, 5)
    truth = ft.scan_tris(o, d, tris)
    share = ft.check_share(name, truth, SHARE[name])
    osc, _ = _oracle_scene(oracle, name)
    worst = 0.0
    for brute in (True, False):
        tid, t = osc.trace_tris(o, d, brute=brute)
        worst = max(worst, ft.check_closest(f"{name}: trace_tris(brute={brute})", truth, tid, t32=t))
    print(f"{name}: decided {share:.3f}, max error / E_t {worst:.3f}")


@pytest.mark.parametrize("cap", [None, 8])
@pytest.mark.parametrize("name", ["geometric", "geometric_up", "slivers"])
def test_split_stack_model_on_deep_trees(aimed, name, cap):
    """tests/test_split_stack.py's model on the two deepest trees (stack bounds 31 and 27), with the
    whole stack in LDS (None: the default, unparked k_render_ps, which has no bound check) and with
    the smallest LDS stack: every LDS write lands below the LDS size and the global part stays within
    DevScene::stack (Lane's own assertions), and the hits equal the model's brute force.  The
    all-rays walk (adversarial_meshes.push_walk) agrees and reaches the depths printed."""
    tr = am.tree(name)
    assert tr.stack == am.built(name)[0]["bvh_stack"] + 1
    c = tr.stack if cap is None else cap
    o, d = (a.astype(np.float64) for a in aimed[name])
    walk = am.push_walk(tr, o, d)
    deep = np.argsort(-walk["depth"])[:20]  # the rays that go deepest, and 20 others
    pick = np.concatenate([deep, np.setdiff1d(np.arange(len(o)), deep)[:20]])
    rng = np.random.default_rng(1)
    spills = refills = 0
    for k in pick:
        lane = ss.Lane(tr, c, o[k], d[k], rng)
        got = lane.run()
        assert got == ss.brute(tr, o[k], d[k]), k
        assert got[1] == walk["bi"][k]
        spills, refills = spills + lane.spills, refills + lane.refills
    print(f"{name} cap {c}: deepest stack top {walk['depth'].max()} of {tr.stack}, spills {spills}, refills {refills}")
    assert walk["depth"].max() > 20  # the rays do go deep
    assert (spills > 0 and refills > 0) if cap == 8 else (spills == 0 and refills == 0)


def _device_refs(nodes):
    refs = nodes[:, 6, :].view(np.int32).astype(np.int64)
    live = ~((nodes[:, 0, :] == EMPTY) & (nodes[:, 1, :] == EMPTY))
    return refs[live]


@pytest.mark.parametrize("name,n_tris,n_nodes,waves", [("nodes_65535", am.PREFIX_65535, 65_535, 6),
                                                        ("nodes_65536", am.PREFIX_65536, 65_536, 5),
                                                        ("tris_2p20m8", (1 << 20) - 8, 61_806, 6)])
def test_limit_mesh_form_and_pushed_refs(name, n_tris, n_nodes, waves):
    """The trees next to the 3-byte stack entry's limits have the form the GPU tests rely on, every
    device ref of the 6-wave ones survives the entry at both node strides, and at least 100 of the
    1,000 limit rays push a ref at the limit: a node of the last 512 (128-B offset >= 2^23 - 2^16)
    or a leaf ref of the last 512 records (<= -2^23 + 2^12)."""
    info, nodes, _ = am.built(name)
    got = (info["n_tris"], info["bvh_nodes"], info["ps_waves"])
    assert got == (n_tris, n_nodes, waves), f"{name}: (triangles, nodes, waves) {got}; {RESEARCH}"
    refs = _device_refs(nodes)
    if name == "tris_2p20m8":
        assert info["bvh_max_leaf"] == 8 and refs.min() <= -(1 << 23) + 128
    else:
        assert refs.max() == n_nodes - 1
    for stride in (128, 80):
        dev = np.where(refs >= 0, refs * stride, refs)
        # (the rule is on the safe side by one: 65,536 nodes still end at offset 2^23 - 128)
        assert np.array_equal(stack24_roundtrip(dev), dev), (name, stride)
    o, d = am.limit_rays(name)
    walk = am.push_walk(am.tree(name), o, d)
    n = int(am.at_limit(name, walk).sum())
    print(f"{name}: {n} of {len(o)} limit rays push a ref at the limit; largest node {walk['max_node'].max()} "
          f"(128-B offset {walk['max_node'].max() * 128:#x}), smallest leaf ref {walk['min_leaf'].min()} "
          f"(-2^23 + {walk['min_leaf'].min() + (1 << 23)}), deepest top {walk['depth'].max()}")
    assert n >= 100


def test_2p20_triangles_get_5_waves():
    """tris_2p20m8's neighbour, one cluster more (2^20 triangles), falls back to 5 waves."""
    info, _, _ = w.bvh_build(am.clusters(am.CLUSTERS_2P20M8 + 1))
    assert info["n_tris"] == 1 << 20 and info["bvh_nodes"] < 1 << 16
    assert info["ps_waves"] == 5


def test_rebuilt_trees_go_deeper_than_the_smallest_lds_stack():
    """tests/test_gpu_rebuild_adversarial.py runs these meshes through the tree of a rebuild
    (wgt_bvh_build_morton).  Its parked-cap8 form tests a spill only if primary rays of some mesh's
    frames reach a stack top above 8 in that tree: the host walk over the restated camera rays
    (test_gpu_gbuffer.camera_rays) shows it for geometric_up and copies300, within the tree's bound."""
    from test_gpu_gbuffer import camera_rays

    deep = {}
    for name in am.GPU:
        built = w.bvh_build_morton(am.small_mesh(name))[:3]
        tr = ss.Tree(None, built=built)
        assert built[0]["bvh_max_depth"] <= 10 and tr.stack <= 31
        top = 0
        for _, cam in am.cameras(name):
            ro, rd = camera_rays(cam, am.W, am.H)
            top = max(top, int(am.push_walk(tr, ro.reshape(-1, 3), rd.reshape(-1, 3))["depth"].max()))
        print(f"{name}: {built[0]['bvh_nodes']} nodes, depth {built[0]['bvh_max_depth']}, stack {built[0]['bvh_stack']}, "
              f"deepest primary stack top {top}")
        assert top <= tr.stack
        deep[name] = top
    assert deep["geometric_up"] > 8 and deep["copies300"] > 8
