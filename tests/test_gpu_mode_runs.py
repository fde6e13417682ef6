"""The two step modes of k_render_ps and the placement of leaves (trav_resolve) against the oracle,
bit for bit as tests/test_gpu_parity.py compares: trees whose leaves have every size 1..8 (so a
triangle step's second slot is live and dead in turn, and the last record of the triangle array
is a step's only live slot), trees that are one leaf, and a small mesh at 4 spp whose phases flip
between node and triangle steps many times; both node forms and the sampled entry point.
"""
import numpy as np
import pytest

from test_gpu_parity import assert_radiance, check_counters

pytestmark = pytest.mark.gpu

EMPTY = np.float32(3e38)  # kEmptySlotCoord (wgt_geom.h)
NODE_FORMS = [{}, {"WGT_CNODE": "0"}]
FORM_IDS = ["compact", "128B"]


def leaf_ranges(nodes):
    """(first, count) of every leaf of an exported tree (wgt_bvh_build's nodes), in array order."""
    n = nodes.reshape(-1, 8, 4)
    refs = n[:, 6, :].view(np.int32)
    live = ~((n[:, 0, :] == EMPTY) & (n[:, 1, :] == EMPTY))
    u = (~refs[live & (refs < 0)]).astype(np.uint32)
    first, count = u >> 3, (u & 7) + 1
    o = np.argsort(first)
    return first[o], count[o]


def ladder_mesh(wgt):
    """Sixteen clusters of 1..8 nearly coincident triangles (each size twice), far enough apart that
    the builder keeps each cluster as one leaf: a split of a cluster would add a node visit and
    save no triangle test."""
    rng = np.random.default_rng(3)
    sizes = [k for _ in range(2) for k in range(1, 9)]
    rng.shuffle(sizes)
    verts = []
    for i, k in enumerate(sizes):
        centre = np.array([90 + 125 * (i % 4), 60 + 110 * (i // 4), 150 + 60 * (i % 3)], np.float32)
        base = rng.uniform(-60, 60, (3, 3)).astype(np.float32)
        for _ in range(k):
            verts.append(centre + base + rng.uniform(-1.5, 1.5, (3, 3)).astype(np.float32))
    return wgt.make_triangles(np.array(verts, np.float32))


def compare(g, r, oracle):
    assert_radiance(g["f32"], r["f32"])
    assert np.array_equal(g["u8"], r["u8"])
    assert np.array_equal(g["hit"], r["hit"])
    check_counters(g["stats"], r["counters"], oracle)


LADDER_FRAMES = [(16, 16, 1), (16, 16, 2), (40, 24, 1), (40, 24, 2)]  # W, H, seed; 4 spp


@pytest.fixture(scope="module")
def ladder(wgt, oracle):
    """The mesh, its scene, and the oracle's frames (computed once, shared by both node forms)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("WGT_SAH_LEAF", "8")  # the leaf cap the clusters are sized for (the builder's default)
    mp.setenv("WGT_DP_LEAF", "0")
    try:
        L, Q, S = wgt.cornell_scene()
        T = ladder_mesh(wgt)
        _, nodes, _ = wgt.bvh_build(T)
    finally:
        mp.undo()
    first, count = leaf_ranges(nodes)
    assert sorted(set(count.tolist())) == list(range(1, 9)), "leaves of every size 1..8"
    assert count[-1] % 2 == 1 and first[-1] + count[-1] == len(T), "the triangle array ends in an odd-sized leaf"
    osc = oracle.OracleScene(L, Q[:5], S, T)
    refs = {(W, H, seed): osc.render(oracle.camera_param(W / H, 4, seed), W, H) for W, H, seed in LADDER_FRAMES}
    return (L, Q[:5], S, T), refs


@pytest.mark.parametrize("env", NODE_FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("W,H,seed", LADDER_FRAMES)
def test_leaves_of_every_size(ctx, wgt, oracle, ladder, W, H, seed, env, monkeypatch):
    """16 x 16: four full waves; 40 x 24: a ragged frame whose waves run sparse."""
    scene, refs = ladder
    monkeypatch.setenv("WGT_SAH_LEAF", "8")
    monkeypatch.setenv("WGT_DP_LEAF", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx.upload_scene(*scene)
    g = ctx.render_tile(wgt.camera_param(W / H, 4, seed), W, H, stats=True)
    compare(g, refs[(W, H, seed)], oracle)
    assert g["stats"]["tri_tests"] > 0


@pytest.fixture(scope="module")
def single_leaf(wgt, oracle):
    L, Q, S = wgt.cornell_scene()
    out = {}
    for n in (1, 2):
        v = np.array([[[100, 0, 100], [450, 0, 100], [278, 400, 500]], [[120, 30, 90], [430, 20, 130], [290, 380, 470]]],
                     np.float32)[:n]
        T = wgt.make_triangles(v)
        out[n] = ((L, Q[:5], S, T), oracle.OracleScene(L, Q[:5], S, T).render(oracle.camera_param(1.0, 4, 8), 32, 32))
    return out


@pytest.mark.parametrize("env", NODE_FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("n", [1, 2])
def test_tree_of_one_leaf(ctx, wgt, oracle, single_leaf, n, env, monkeypatch):
    """The root's only live child is a leaf of n triangles: every traversal is the root step (in the
    service pass) and triangle steps, the second slot dead (n = 1) or live (n = 2)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene, ref = single_leaf[n]
    ctx.upload_scene(*scene)
    info = ctx.scene_info()
    assert info["n_tris"] == n and info["bvh_nodes"] == 1
    compare(ctx.render_tile(wgt.camera_param(1.0, 4, 8), 32, 32, stats=True), ref, oracle)


BUNNY_W, BUNNY_H, BUNNY_SEED = 48, 27, 3  # the frame of tests/golden/bunny2000_48x27_spp1_seed3.npz
# node_visits + tri_tests of the instrumented pass of this frame at 4 spp: the least and the most
# that passes of the parent commit's library counted (test_step_counts_are_the_parents)
BUNNY_STEPS_PARENT = (44978, 44978)


@pytest.fixture(scope="module")
def bunny2000(oracle):
    d = np.load(__file__.rsplit("/", 1)[0] + "/golden/bunny2000_48x27_spp1_seed3.npz")
    scene = (d["lights"], d["quads"], d["spheres"], d["tris"])
    osc = oracle.OracleScene(*scene)
    return scene, osc, osc.render(oracle.camera_param(BUNNY_W / BUNNY_H, 4, BUNNY_SEED), BUNNY_W, BUNNY_H)


@pytest.mark.parametrize("env", NODE_FORMS, ids=FORM_IDS)
def test_small_mesh_many_mode_flips(ctx, wgt, oracle, bunny2000, env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene, _, ref = bunny2000
    ctx.upload_scene(*scene)
    g = ctx.render_tile(wgt.camera_param(BUNNY_W / BUNNY_H, 4, BUNNY_SEED), BUNNY_W, BUNNY_H, stats=True)
    compare(g, ref, oracle)
    # the steps come in both modes, and in runs of more than one
    assert g["stats"]["node_visits"] > g["stats"]["traced_rays"] and g["stats"]["tri_tests"] > g["stats"]["traced_rays"]


def test_sampled_entry_point(ctx, wgt, oracle, bunny2000):
    """wgt_render_tile_sampled (the sampled instantiation of the kernel) at side 2 everywhere: the
    4-spp frame."""
    scene, _, ref = bunny2000
    ctx.upload_scene(*scene)
    smap = np.full((BUNNY_H, BUNNY_W), 2, np.uint8)
    g = ctx.render_tile(wgt.camera_param(BUNNY_W / BUNNY_H, 1, BUNNY_SEED), BUNNY_W, BUNNY_H, stats=True, sample_map=smap)
    compare(g, ref, oracle)


def test_step_counts_are_the_parents(ctx, wgt, bunny2000):
    """The traversal takes the steps it took before the rewrite of trav_resolve: node visits plus
    triangle tests of the instrumented pass stay within what the parent commit's library counts on
    the same input.  Measured on an MI355X with the parent's library, six passes: 31,829 node visits
    and 13,149 triangle tests (44,978) in every one of them, a spread of 0.  The counts vary with
    the schedule where waves refill from the pixel queue; this frame's 24 blocks go to 24 waves
    that take one block each, so every wave's sequence of steps is fixed."""
    scene, _, _ = bunny2000
    ctx.upload_scene(*scene)
    st = ctx.render_tile(wgt.camera_param(BUNNY_W / BUNNY_H, 4, BUNNY_SEED), BUNNY_W, BUNNY_H, stats=True)["stats"]
    steps = st["node_visits"] + st["tri_tests"]
    print(f"node_visits {st['node_visits']} tri_tests {st['tri_tests']} sum {steps}")
    assert BUNNY_STEPS_PARENT[0] <= steps <= BUNNY_STEPS_PARENT[1]
