"""wgt_rebuild_triangles_device at scale and at the limits of the kernel forms.

tests/test_gpu_rebuild.py builds trees of at most 4096 triangles at the default leaf target.  What a
real rebuild meets beyond that (tests/rebuild_cases.py SCALE, each condition proved on the CPU in
tests/test_rebuild_host.py):
  levels 8 to 10, the level cap deciding splits all over the tree, level lists of 10^4 nodes (hundreds
  of blocks, a scan over more than one) and a level of exactly 256 nodes        soup100k, grid4096
  the leaf targets 1 and 8 (8 is the largest count a leaf ref encodes)           every case of CASES
  more than 2^20 keys, which the sort handles by another algorithm, in runs of 8 equal codes whose
  indices lie 2^17 apart                                                        tris_2p20p8
  the kernel form following the tree: 6 waves and 3-byte stack entries below 2^16 nodes and 2^20
  triangles, 5 waves and 4-byte entries from there on, in either direction       nodes_below, nodes_above, tris_2p20p8

Expected values: the host specification (wgt_bvh_build_morton) bit for bit for the trees; the C oracle
(its own BVH and its brute-force scan) bit for bit for rays and frames, since the closest hit does not
depend on the tree.  The two cases of 2^20 + 8 triangles take several seconds each, most of it the
oracle's build and the host specification: both limits of that case sit at 2^20, so it cannot shrink.
"""
import numpy as np
import pytest

import adversarial_meshes as am
import hit_records as hr
import rebuild_cases as cases
import rebuild_restatement as rr
import refit_cases as rc
import test_gpu_refit as host_form  # its scenes and frames, not its tests
import test_gpu_rebuild as small  # its comparisons, not its tests
from test_gpu_adversarial import _set_env
from test_gpu_parity import assert_radiance, check_counters
from test_gpu_refit_device import _dev, _host

pytestmark = pytest.mark.gpu
W, H = am.W, am.H


@pytest.fixture(scope="module")
def fresh(wgt):
    """A second context: the fresh uploads the rebuilt one is compared with."""
    c = wgt.Context(0)
    yield c
    c.close()


def _rebuild_and_compare(ctx, wgt, name, L):
    """upload(nine), rebuild to the case at the leaf target L: the tree and the scene report are the
    specification's, and the input is left as it was.  -> the resident tree."""
    T = cases.case(name, L)
    Ls, Q, S = host_form._tiny_scene(wgt)
    ctx.upload_scene(Ls, Q, S, rc.mesh("nine"))
    d = _dev(T)
    ctx.rebuild_triangles_device(d.data_ptr(), len(T))
    info = ctx.scene_info()
    print(f"{name} L={L}: {len(T)} triangles, {info['bvh_nodes']} nodes, depth {info['bvh_max_depth']}, stack "
          f"{info['bvh_stack']}, max leaf {info['bvh_max_leaf']}, waves {info['ps_waves']}")
    small._assert_is_specification(ctx, wgt, T, f"{name} L={L}", cases.spec(name, L))
    assert info["bvh_max_leaf"] <= L
    assert np.array_equal(_host(d), np.ascontiguousarray(T).view(np.uint8)), "the input was written"
    return ctx.bvh_read()


@pytest.mark.parametrize("L", [1, 8])
@pytest.mark.parametrize("name", cases.CASES)
def test_leaf_targets_1_and_8(ctx, wgt, monkeypatch, name, L):
    """a1. Every case of tests/test_gpu_rebuild.py under WGT_REBUILD_LEAF = 1 and 8: the rebuild reads the
    knob on each call (wgt_rebuild_triangles_device calls RebuildLeafFromEnv), as the specification."""
    monkeypatch.setenv("WGT_REBUILD_LEAF", str(L))
    _rebuild_and_compare(ctx, wgt, name, L)


@pytest.mark.parametrize("name", ["soup100k", "nodes_below", "nodes_above"])
def test_device_tree_at_scale(ctx, wgt, monkeypatch, name):
    """a2. Ten levels, level lists of up to 34,000 nodes, and either side of 2^16 nodes."""
    L = cases.SCALE[name]
    monkeypatch.setenv("WGT_REBUILD_LEAF", str(L))
    _rebuild_and_compare(ctx, wgt, name, L)
    assert ctx.scene_info()["bvh_max_depth"] == 10


def _codes64(T):
    """rebuild_restatement's codes, the bits interleaved in numpy: bit k of x at 3k + 2, of y at 3k + 1,
    of z at 3k."""
    q = rr.cells(T).astype(np.uint64)
    code = np.zeros(len(T), np.uint64)
    for k in range(rr.BITS):
        for a in range(3):
            code |= ((q[:, a] >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k + 2 - a)
    return code


def test_device_tree_past_2p20_keys(ctx, wgt, monkeypatch):
    """a3. 2^20 + 8 keys, beyond the merge sort's limit: the tree is the specification's, and, stated
    without it, the records' codes ascend and within every run of equal codes (each holds the 8 exact
    copies of a cluster, 2^17 indices apart in the input) the original indices ascend: the sort is stable."""
    name, L = "tris_2p20p8", cases.SCALE["tris_2p20p8"]
    monkeypatch.setenv("WGT_REBUILD_LEAF", str(L))
    T = cases.case(name, L)
    assert len(T) == (1 << 20) + 8
    recs = _rebuild_and_compare(ctx, wgt, name, L)[1]
    assert ctx.scene_info()["ps_waves"] == 5
    idx = rc.bits(recs[:, 0, 3]).astype(np.int64)
    assert np.array_equal(np.sort(idx), np.arange(len(T))), "the records hold a permutation"
    code = _codes64(T)[idx]
    assert (code[1:] >= code[:-1]).all(), "codes ascend"
    tie = code[1:] == code[:-1]
    assert tie.sum() >= 7 * cases.CLUSTERS_2P20P8  # every cluster is one run, or part of one
    assert (idx[1:][tie] > idx[:-1][tie]).all(), "original indices ascend within a run of equal codes"
    far = (idx[1:][tie] - idx[:-1][tie]) >= cases.COPY_STRIDE
    print(f"{name}: {int(tie.sum())} neighbours with equal codes, {int(far.sum())} of them at least 2^17 indices apart")
    assert far.sum() >= 7 * cases.COPY_STRIDE


@pytest.mark.parametrize("L", [1, 8])
def test_everything_equals_a_fresh_upload_per_leaf_target(ctx, fresh, wgt, monkeypatch, L):
    """b. tests/test_gpu_rebuild.py's traversal test (frame, sampled frame, G-buffer, hit records,
    occlusion against a fresh upload) through a tree of leaf target 1 and one of 8."""
    monkeypatch.setenv("WGT_REBUILD_LEAF", str(L))
    small.everything_equals_a_fresh_upload(ctx, fresh, wgt, f"L={L}")
    info, want = ctx.scene_info(), cases.spec("bunny2000", L)[0]
    assert (info["bvh_nodes"], info["bvh_max_leaf"], info["bvh_stack"]) == (want["bvh_nodes"], want["bvh_max_leaf"], want["bvh_stack"])
    assert info["bvh_max_leaf"] == (1 if L == 1 else 8)


_ORACLE = {}


def _oracle_scene(oracle, name):
    """(L, Q, S, T), the oracle's scene, the number of lights and quads; one oracle build per case."""
    if name not in _ORACLE:
        L, Q, S = am.scene_parts(name)
        if name == "tris_2p20p8":  # no walls: its last records lie in the box's far corner, most origins outside it
            Q = Q[:0].copy()
        T = cases.case(name)
        _ORACLE[name] = ((L, Q, S, T), oracle.OracleScene(L, Q, S, T), len(L) + len(Q))
    return _ORACLE[name]


def _rays_equal_the_oracle(ctx, oracle, name, more):
    """trace_rays on the limit rays and `more` aimed rays: the oracle's BVH on all, its brute force on 200."""
    (L, Q, S, T), osc, nlq = _oracle_scene(oracle, name)
    o, d = cases.limit_rays(name)
    n_limit = len(o)
    if more:
        ao, ad = am.aimed_rays(T, more, 4)
        o, d = np.concatenate([o, ao]), np.concatenate([d, ad])
    gp, gd = ctx.trace_rays(o, d)
    rp, rd = osc.trace(o, d)
    assert np.array_equal(gp, rp), f"{name}: {int(np.sum(gp != rp))} prims differ; first: ray {np.flatnonzero(gp != rp)[0]}"
    assert np.array_equal(hr.bits(gd), hr.bits(rd))
    k = np.r_[0:100, n_limit - 100:n_limit] if not more else np.r_[0:100, n_limit:n_limit + 100]
    bp, bd = osc.trace(o[k], d[k], brute=True)
    assert np.array_equal(gp[k], bp) and np.array_equal(hr.bits(gd[k]), hr.bits(bd))
    assert np.mean((gp >= nlq) & (gp < nlq + len(T))) > 0.3
    return o, d, gp, k


def _large_step(ctx, oracle, monkeypatch, name, waves):
    """After a rebuild to a node-limit case: the form, rays and one frame from among the limit targets
    under the three kernel forms against the oracle, and the host walk's count of primary rays that push
    a ref the other form's stack entry could not hold (nodes_below: one next to its limit)."""
    (L, Q, S, T), osc, nlq = _oracle_scene(oracle, name)
    info, want = ctx.scene_info(), cases.spec(name)[0]
    for key in ("n_tris", "bvh_nodes", "bvh_stack", "bvh_max_depth", "bvh_max_leaf", "ps_waves", "ps_park", "ps_stack"):
        assert info[key] == want[key], (name, key, info[key], want[key])
    assert info["ps_waves"] == waves and info["ps_stack"] == info["bvh_stack"] + 1
    _rays_equal_the_oracle(ctx, oracle, name, 2000)
    cam = cases.limit_camera(name)
    r = osc.render(cam, W, H)
    for env in ({}, {"WGT_CNODE": "0"}, {"WGT_KERNEL": "1"}):  # the node form and the kernel are the frame's
        _set_env(monkeypatch, env)
        g = ctx.render_tile(cam, W, H, stats=True)
        assert np.array_equal(g["hit"], r["hit"]), f"{name} {env}: {int(np.sum(g['hit'] != r['hit']))} hit ids differ"
        assert_radiance(g["f32"], r["f32"])
        check_counters(g["stats"], r["counters"], oracle)
        assert g["stats"]["stack_overflows"] == 0
    _set_env(monkeypatch, {})
    g = ctx.render_gbuffer(cam, W, H, rays=True)
    assert np.array_equal(g["prim"], r["hit"])
    ro, rd = g["origin"].reshape(-1, 3), g["direction"].reshape(-1, 3)
    walk = am.push_walk(cases.spec_tree(name), ro, rd)
    n = int(cases.over_limit(name, walk).sum())
    on_mesh = float(np.mean((r["hit"] >= nlq) & (r["hit"] < nlq + len(T))))
    print(f"{name}: {info['bvh_nodes']} nodes, {info['ps_waves']} waves; {n} of {len(ro)} primary rays push a node ref >= "
          f"{cases.OVER[name]} (largest {walk['max_node'].max()}); {on_mesh:.2f} of the pixels on the mesh")
    assert n >= 100


def test_form_follows_the_rebuild(ctx, fresh, oracle, wgt, monkeypatch):
    """c. One context: upload nine (6 waves), rebuild to nodes_above (5 waves, 4-byte stack entries), to
    nodes_below (6 waves, 3-byte entries, next to their limit), to nine.  Had the first rebuild kept
    the 3-byte entries, node refs beyond 2^16 would be cut: wrong hits, not a fault."""
    _set_env(monkeypatch, {})
    monkeypatch.setenv("WGT_REBUILD_LEAF", "1")
    nine = rc.mesh("nine")
    L, Q, S = am.scene_parts("nodes_above")
    ctx.upload_scene(L, Q, S, nine)
    assert ctx.scene_info()["ps_waves"] == 6
    for name, waves in (("nodes_above", 5), ("nodes_below", 6)):
        T = cases.case(name)
        d = _dev(T)
        ctx.rebuild_triangles_device(d.data_ptr(), len(T))
        _large_step(ctx, oracle, monkeypatch, name, waves)
    d = _dev(nine)
    ctx.rebuild_triangles_device(d.data_ptr(), len(nine))
    info = ctx.scene_info()
    assert (info["n_tris"], info["ps_waves"], info["bvh_nodes"]) == (9, 6, cases.spec("nine", 1)[0]["bvh_nodes"])
    fresh.upload_scene(L, Q, S, nine)
    cam = host_form._camera_at(wgt, nine, 1.0, 4, 2)
    host_form._same_frame(ctx.render_tile(cam, 32, 32), fresh.render_tile(cam, 32, 32), "back to nine")


def test_rebuild_past_2p20_triangles(ctx, oracle, wgt, monkeypatch):
    """d. upload nine, rebuild to 2^20 + 8 triangles: 5 waves; 1,000 rays at the triangles of the last
    512 leaf-ordered records and 200 at those of the last 8, the only records whose leaf refs
    (<= -2^23) a 3-byte entry cannot hold: trace_rays and trace_hits equal the oracle's BVH on all and
    its brute force on 200, every triangle hit is the lowest index of its cluster, and the host walk
    shows at least 100 rays pushing such a leaf ref.  No frame: the oracle's alone would take seconds."""
    name = "tris_2p20p8"
    _set_env(monkeypatch, {})
    monkeypatch.setenv("WGT_REBUILD_LEAF", str(cases.SCALE[name]))
    (L, Q, S, T), osc, nlq = _oracle_scene(oracle, name)
    ctx.upload_scene(L, Q, S, rc.mesh("nine"))
    assert ctx.scene_info()["ps_waves"] == 6
    d = _dev(T)
    ctx.rebuild_triangles_device(d.data_ptr(), len(T))
    info, want = ctx.scene_info(), cases.spec(name)[0]
    for key in ("n_tris", "bvh_nodes", "bvh_stack", "bvh_max_depth", "bvh_max_leaf", "ps_waves", "ps_park", "ps_stack"):
        assert info[key] == want[key], (key, info[key], want[key])
    assert info["ps_waves"] == 5 and info["n_tris"] == (1 << 20) + 8
    o, d_, gp, k = _rays_equal_the_oracle(ctx, oracle, name, 0)
    want_rec, is_tri = hr.expected_records(osc, L, Q, S, T, o, d_)  # the oracle's BVH on all
    got = ctx.trace_hits(o, d_)
    hr.assert_records_equal(got, want_rec, o, d_, what=name)
    assert np.array_equal(got["prim"][k], osc.trace(o[k], d_[k], brute=True)[0])
    tid = gp[is_tri].astype(np.int64) - nlq
    assert is_tri.sum() >= 600 and np.array_equal(tid, cases.cluster_first(tid)), "the lowest index of a cluster wins"
    walk = am.push_walk(cases.spec_tree(name), o, d_)
    n = int(cases.over_limit(name, walk).sum())
    print(f"{name}: {info['bvh_nodes']} nodes, depth {info['bvh_max_depth']}, stack {info['bvh_stack']}; {int(is_tri.sum())} "
          f"triangle hits; {n} of {len(o)} rays push a leaf ref <= -2^23 (smallest {walk['min_leaf'].min()})")
    assert n >= 100
