"""The meshes of tests/adversarial_meshes.py through a rebuilt tree.

The closest hit does not depend on the tree, but tests/test_gpu_adversarial.py traverses uploaded SAH
trees only.  A rebuilt tree (the LBVH of wgt_rebuild_triangles_device) puts the same exact duplicates,
zero-area triangles, scene-sized triangles and slivers into other leaves, with other overlap and
other empty slots.  These tests run that module's bodies with "upload nine, then rebuild to the mesh"
in the upload's place: the same rays, the same expected values (the oracle's brute force, renders and
counters, float64 geometry with the same shares and tolerances), every stack form.

What depends on the tree comes from the host specification, wgt_bvh_build_morton: the scene report's
tree fields, and, for the parked forms, whether a frame must spill: where the host walk
(adversarial_meshes.push_walk) of the frame's primary rays over the specification's tree reaches a
stack top above the LDS stack, stack_spills must be positive.
"""
import functools

import numpy as np
import pytest

import adversarial_meshes as am
import refit_cases as rc
import test_gpu_adversarial as up  # its bodies, forms and scenes, not its tests
from test_gpu_refit_device import _dev

pytestmark = pytest.mark.gpu
W, H = am.W, am.H
# the specification's fields that do not depend on the other primitives (the compact step follows the
# scene's extent, walls included)
TREE_INFO = ("n_tris", "bvh_nodes", "bvh_leaves", "bvh_max_depth", "bvh_max_leaf", "sah_cost", "bvh_width", "bvh_stack",
             "bvh2_nodes", "bvh2_depth", "ps_waves", "ps_park", "ps_stack")


def rebuilt(ctx, L, Q, S, T):
    """install: upload the scene with nine triangles, then rebuild to T from device memory."""
    ctx.upload_scene(L, Q, S, rc.mesh("nine"))
    d = _dev(T)
    ctx.rebuild_triangles_device(d.data_ptr(), len(T))


@functools.lru_cache(maxsize=None)
def _spec_tree(name):
    """The specification's tree of a mesh (its topology does not depend on the kernel form's knobs)."""
    import test_split_stack as ss
    import webgputracer_amd as wgt

    return ss.Tree(None, built=wgt.bvh_build_morton(am.small_mesh(name))[:3])


_DEEPEST = {}


def _deepest_primary_top(ctx, name):
    """The highest stack top any primary ray of the mesh's frames reaches in the host walk over the
    specification's tree; the rays are the G-buffer pass's, which do not depend on the tree."""
    if name not in _DEEPEST:
        top = 0
        for _, cam in am.cameras(name):
            g = ctx.render_gbuffer(cam, W, H, rays=True)
            walk = am.push_walk(_spec_tree(name), g["origin"].reshape(-1, 3), g["direction"].reshape(-1, 3))
            top = max(top, int(walk["depth"].max()))
        _DEEPEST[name] = top
    return _DEEPEST[name]


def rebuilt_tree(ctx, name, form, info):
    """tree: the scene report states the specification's tree, under the form's knobs."""
    import webgputracer_amd as wgt

    want = wgt.bvh_build_morton(am.small_mesh(name))[0]
    for k in TREE_INFO:
        assert info[k] == want[k], (name, form, k, info[k], want[k])


def rebuilt_spills(ctx, name, form, info, spills):
    """spilled: a parked frame one of whose primary rays needs more than the LDS stack has spilled."""
    if info["ps_park"] and form != "simple":
        top = _deepest_primary_top(ctx, name)
        print(f"{name} {form}: deepest primary stack top {top}, LDS stack {info['ps_stack']}, spills {spills}")
        if top > info["ps_stack"]:
            assert spills > 0


@pytest.mark.parametrize("name", am.GPU)
def test_queries(ctx, oracle, name):
    """test_gpu_adversarial.queries_body through the rebuilt tree; the tie meshes answer the lowest index."""
    up.queries_body(ctx, oracle, name, rebuilt)


@pytest.mark.parametrize("form", list(up.FORMS))
@pytest.mark.parametrize("name", am.GPU)
def test_render(ctx, oracle, name, form, monkeypatch):
    """test_gpu_adversarial.render_body through the rebuilt tree, under every stack form."""
    up.render_body(ctx, oracle, name, form, monkeypatch, rebuilt, rebuilt_tree, rebuilt_spills)


@pytest.mark.parametrize("name", am.GPU)
def test_gbuffer(ctx, oracle, name, monkeypatch):
    """test_gpu_adversarial.gbuffer_body through the rebuilt tree."""
    up.gbuffer_body(ctx, oracle, name, monkeypatch, rebuilt)


def test_cap8_spills_on_some_mesh(ctx, oracle, monkeypatch):
    """The parked-cap8 form tests a spill only if some mesh's primary rays go deeper than 8 entries in
    the rebuilt tree: at least one does, and on it a frame under that form spills."""
    up._set_env(monkeypatch, up.FORMS["parked-cap8"])
    deep = []
    for name in am.GPU:
        (L, Q, S, T), _, _ = up._scene(oracle, name)
        rebuilt(ctx, L, Q, S, T)
        assert ctx.scene_info()["ps_stack"] == 8
        top = _deepest_primary_top(ctx, name)
        print(f"{name}: deepest primary stack top {top}")
        if top > 8:
            deep.append(name)
            spills = sum(ctx.render_tile(cam, W, H, stats=True)["stats"]["stack_spills"] for _, cam in am.cameras(name))
            assert spills > 0, name
    assert deep, "no mesh's primary rays need more than 8 stack entries in a rebuilt tree"
