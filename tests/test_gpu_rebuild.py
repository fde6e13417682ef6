"""wgt_rebuild_triangles and wgt_rebuild_triangles_device: a new triangle BVH made on the device.

The closest hit does not depend on the tree, so after a rebuild every render and query must equal a
fresh upload's bit for bit; and the device tree itself must equal the host specification
(wgt_bvh_build_morton) bit for bit.  Meshes: tests/rebuild_cases.py; scenes, camera and rays:
tests/test_gpu_refit.py; device tensors: tests/test_gpu_refit_device.py.  The largest mesh has 4096
triangles, every case takes milliseconds; larger trees, the other leaf targets and the limits of the
kernel forms are in tests/test_gpu_rebuild_scale.py.
"""
import functools

import numpy as np
import pytest

import hit_records as hr
import rebuild_cases as cases
import refit_cases as rc
import test_gpu_refit as host_form  # its scenes, camera and rays, not its tests
from test_gpu_refit_device import _dev, _host, _refused, _verts32

pytestmark = pytest.mark.gpu
f32 = np.float32

# the fields of wgt_scene_info that the specification's info states; the counts of the other
# primitives, device_bytes, node_form (the camera's) and ps_resident (the device's) are the context's
TREE_INFO = ("n_tris", "bvh_nodes", "bvh_leaves", "bvh_max_depth", "bvh_max_leaf", "sah_cost", "bvh_width", "bvh_stack",
             "bvh2_nodes", "bvh2_depth", "bvh_compact", "bvh_compact_step", "ps_waves", "ps_park", "ps_stack")


@pytest.fixture(scope="module")
def fresh(wgt):
    """A second context: the fresh uploads the rebuilt one is compared with."""
    c = wgt.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _want(name):
    """wgt_bvh_build_morton of a case, computed once."""
    import webgputracer_amd as wgt

    return wgt.bvh_build_morton(cases.case(name))


def _shaded(T, seed):
    """T with a random colour per triangle and every 7th triangle emissive."""
    T = T.copy()
    T["col"] = np.random.default_rng(seed).uniform(0.1, 0.9, (len(T), 3)).astype(f32)
    T["emissive"] = (np.arange(len(T)) % 7 == 3).astype(f32)
    return T


def _pad256(x):
    return (x + 255) // 256 * 256


def _bytes_in_use(info):
    """The scene's lights, quads and spheres, then the five tree parts, each padded to 256 bytes."""
    n, t = info["bvh_nodes"], info["n_tris"]
    return (_pad256((info["n_lights"] + info["n_quads"]) * 96) + _pad256(info["n_spheres"] * 32) +
            sum(_pad256(b) for b in (n * 128, t * 64, t * 32, n * 80, n)))


def _assert_is_specification(ctx, wgt, T, what, want=None):
    info, *tree = want if want is not None else wgt.bvh_build_morton(T)
    rc.assert_trees_equal(ctx.bvh_read(), tree, what=what)
    now = ctx.scene_info()
    for k in TREE_INFO:
        assert now[k] == info[k], (what, k, now[k], info[k])
    assert now["device_bytes"] == _bytes_in_use(now), what


@pytest.mark.parametrize("name", cases.CASES)
def test_device_tree_equals_the_specification(ctx, wgt, name):
    """1. upload(nine), rebuild to the case: wgt_bvh_read equals wgt_bvh_build_morton bit for bit, and the
    scene report its info."""
    T = cases.case(name)
    L, Q, S = host_form._tiny_scene(wgt)
    ctx.upload_scene(L, Q, S, rc.mesh("nine"))
    d = _dev(T)
    ctx.rebuild_triangles_device(d.data_ptr(), len(T))
    info = ctx.scene_info()
    print(f"{name}: {len(T)} triangles, {info['bvh_nodes']} nodes, depth {info['bvh_max_depth']}, stack {info['bvh_stack']}")
    _assert_is_specification(ctx, wgt, T, name, _want(name))
    assert np.array_equal(_host(d), np.ascontiguousarray(T).view(np.uint8)), "the input was written"


def _sample_map(W, H):
    m = np.ones((H, W), np.uint8)
    m[H // 4:H // 2, :] = 2
    m[H // 2:, W // 3:] = 3
    return m


def _everything(c, cam, W, H, o, d, lim):
    frame = c.render_tile(cam, W, H, stats=True)
    sampled = c.render_tile(cam, W, H, sample_map=_sample_map(W, H))
    gbuf = c.render_gbuffer(cam, W, H)
    return frame, sampled, gbuf, c.trace_hits(o, d), c.occluded(o, d, lim)


def _assert_everything_equal(got, want, what):
    host_form._same_frame(got[0], want[0], f"{what}: frame")
    host_form._same_frame(got[1], want[1], f"{what}: sampled frame")
    for k in ("queries", "traced_rays", "samples", "nan_rays"):
        assert got[0]["stats"][k] == want[0]["stats"][k], (what, k)
    assert got[0]["stats"]["stack_overflows"] == 0, what
    for f in hr.FIELDS:
        assert np.array_equal(got[2][f].view(np.uint8), want[2][f].view(np.uint8)), (what, "gbuffer", f)
        assert np.array_equal(got[3][f].view(np.uint8), want[3][f].view(np.uint8)), (what, "hits", f)
    assert np.array_equal(got[4], want[4]), (what, "occlusion")


def everything_equals_a_fresh_upload(ctx, fresh, wgt, form):
    """upload(A) then rebuild(B) against a fresh context's upload(B), B of another count than A: a
    32x32, 4 spp Cornell-plus-mesh frame (f32 words, u8, hit ids), a sampled frame with a non-uniform
    map, the G-buffer, hit records and occlusion answers of 4096 seeded rays, and the stats' ray counts.
    The knobs in force are the caller's; `form` names them in the messages."""
    A, B = rc.mesh("nine"), _shaded(rc.mesh("bunny2000"), 2)
    L, Q, S = host_form._walls(wgt)
    W = H = 32
    cam = host_form._camera_at(wgt, B, 1.0, 4, 11)
    o, d = host_form._query_rays(B, 4096, 3)
    fresh.upload_scene(L, Q, S, B)
    lim = np.nextafter(fresh.trace_hits(o, d)["dist"], f32(np.inf))
    want = _everything(fresh, cam, W, H, o, d, lim)
    assert want[4].sum() > 400
    nlq = len(L) + len(Q)
    assert int(np.sum((want[0]["hit"] >= nlq) & (want[0]["hit"] < nlq + len(B)))) >= 25, "the frame sees the mesh"
    ctx.upload_scene(L, Q, S, A)
    dB = _dev(B)
    ctx.rebuild_triangles_device(dB.data_ptr(), len(B))
    got = _everything(ctx, cam, W, H, o, d, lim)
    _assert_everything_equal(got, want, form)
    print(f"{form}: node visits rebuilt {got[0]['stats']['node_visits']}, uploaded {want[0]['stats']['node_visits']}")


@pytest.mark.parametrize("form", ["default", "WGT_KERNEL=1"])
def test_everything_equals_a_fresh_upload(ctx, fresh, wgt, monkeypatch, form):
    """2. everything_equals_a_fresh_upload under the default kernel and the simple one."""
    if form != "default":
        monkeypatch.setenv(*form.split("="))
    everything_equals_a_fresh_upload(ctx, fresh, wgt, form)


def test_count_goes_down_and_up(ctx, fresh, wgt):
    """3a. 1980 -> 500 -> 3000 triangles: the tree after each step, sphere ids that moved, and a frame
    against a fresh upload at the end.  The third rebuild reuses the first one's allocation."""
    A = rc.mesh("bunny2000")
    steps = (A[:500].copy(), _shaded(wgt.procedural_mesh("bunny", 3000), 5), A)
    L, Q, S = host_form._walls(wgt)
    ctx.upload_scene(L, Q, S, A)
    for T in steps:
        dT = _dev(T)
        ctx.rebuild_triangles_device(dT.data_ptr(), len(T))
        info = ctx.scene_info()
        assert info["n_tris"] == len(T) and ctx.n_prims == len(L) + len(Q) + len(T) + len(S)
        tree = ctx.bvh_read()
        assert np.array_equal(rc.bits(tree[0]), rc.bits(rc.expected_nodes(tree[0], tree[1])))
        assert sorted(rc.bits(tree[1][:, 0, 3]).tolist()) == list(range(len(T)))
        cam = host_form._camera_at(wgt, T, 1.0, 4, 6)
        fresh.upload_scene(L, Q, S, T)
        host_form._same_frame(ctx.render_tile(cam, 32, 32), fresh.render_tile(cam, 32, 32), f"{len(T)} triangles")
        o, d = host_form._query_rays(T, 4096, 4)
        prim, dist = ctx.trace_rays(o, d)
        wprim, wdist = fresh.trace_rays(o, d)
        assert np.array_equal(prim, wprim) and np.array_equal(hr.bits(dist), hr.bits(wdist))


def test_scene_uploaded_without_triangles(ctx, fresh, wgt):
    """3b. A scene uploaded with no triangles is rebuilt to nine."""
    T = rc.mesh("nine")
    L, Q, S = host_form._tiny_scene(wgt)
    ctx.upload_scene(L, Q, S)
    assert ctx.scene_info()["n_tris"] == 0
    ctx.rebuild_triangles(T)
    _assert_is_specification(ctx, wgt, T, "from no triangles")
    L, Q, S = host_form._walls(wgt)
    ctx.upload_scene(L, Q, S)
    ctx.rebuild_triangles(T)
    fresh.upload_scene(L, Q, S, T)
    cam = host_form._camera_at(wgt, T, 1.0, 4, 2)
    host_form._same_frame(ctx.render_tile(cam, 32, 32), fresh.render_tile(cam, 32, 32), "from no triangles")


def test_update_refits_the_rebuilt_tree(ctx, fresh, wgt):
    """3c. rebuild, then wgt_update_vertices_device with a jitter: the rebuilt topology with the boxes of
    the jittered mesh, and frames and hits of a fresh upload of the jittered mesh."""
    A, B = rc.mesh("bunny2000"), rc.moved("bunny2000", "jitter5")
    V = _verts32(B)
    T = wgt.make_triangles(V)
    T["col"], T["emissive"] = A["col"], A["emissive"]  # the vertex form keeps them
    L, Q, S = host_form._walls(wgt)
    ctx.upload_scene(L, Q, S, rc.mesh("nine"))
    dA = _dev(A)
    ctx.rebuild_triangles_device(dA.data_ptr(), len(A))
    rebuilt = ctx.bvh_read()
    dV = _dev(V)
    ctx.update_vertices_device(dV.data_ptr(), 3 * len(A), len(A))
    tree = ctx.bvh_read()
    assert np.array_equal(rc.refs_of(tree[0]), rc.refs_of(rebuilt[0])) and np.array_equal(tree[3], rebuilt[3])
    assert np.array_equal(rc.bits(tree[1][:, 0, 3]), rc.bits(rebuilt[1][:, 0, 3]))
    assert np.array_equal(rc.bits(tree[0]), rc.bits(rc.expected_nodes(tree[0], tree[1])))
    assert not np.array_equal(rc.bits(tree[0]), rc.bits(rebuilt[0]))
    fresh.upload_scene(L, Q, S, T)
    cam = host_form._camera_at(wgt, T, 1.0, 4, 8)
    host_form._same_frame(ctx.render_tile(cam, 32, 32), fresh.render_tile(cam, 32, 32), "rebuilt, then refit")
    o, d = host_form._query_rays(T, 4096, 9)
    hits, want = ctx.trace_hits(o, d), fresh.trace_hits(o, d)
    for f in hr.FIELDS:
        assert np.array_equal(hits[f].view(np.uint8), want[f].view(np.uint8)), f
    # and the host-form update, back to A: the rebuilt tree again
    ctx.update_triangles(A)
    rc.assert_trees_equal(ctx.bvh_read(), rebuilt, what="refit back to A")


def test_host_form_equals_device_form(ctx, wgt):
    """3d. wgt_rebuild_triangles stages the array and runs the same body."""
    T = _shaded(rc.mesh("bunny2000"), 3)
    L, Q, S = host_form._tiny_scene(wgt)
    ctx.upload_scene(L, Q, S, rc.mesh("one"))
    ctx.rebuild_triangles(T)
    _assert_is_specification(ctx, wgt, T, "host form")
    by_host, info = ctx.bvh_read(), ctx.scene_info()
    ctx.upload_scene(L, Q, S, rc.mesh("one"))
    dT = _dev(T)
    ctx.rebuild_triangles_device(dT.data_ptr(), len(T))
    rc.assert_trees_equal(ctx.bvh_read(), by_host, what="device form")
    assert ctx.scene_info() == info
    host_ms, device_ms = ctx.update_timing()
    assert host_ms > 0.0 and device_ms > 0.0


def test_refusals_leave_everything_as_it_was(ctx, wgt):
    """4a. Every refusal's status and words, in the stated order; afterwards the tree's bytes, the scene
    report, a frame and the input's bytes."""
    from webgputracer_amd import _lib

    A = rc.mesh("bunny2000")
    n = len(A)
    L, Q, S = host_form._walls(wgt)
    dA = _dev(A)

    def raw(c, ptr, count, stream=None):
        return lambda lib: lib.wgt_rebuild_triangles_device(c.h, ptr or None, count, stream)

    with wgt.Context(0) as empty:
        _refused(empty, raw(empty, dA.data_ptr(), n), _lib.WGT_E_NOSCENE, "no scene")
        _refused(empty, lambda lib: lib.wgt_rebuild_triangles(empty.h, _lib.ptr(A), n), _lib.WGT_E_NOSCENE, "no scene")
    ctx.upload_scene(L, Q, S, A)
    cam = host_form._camera_at(wgt, A, 1.0, 1, 9)
    tree, info, frame = ctx.bvh_read(), ctx.scene_info(), ctx.render_tile(cam, 32, 32)
    nan, far, both = A.copy(), A.copy(), A.copy()
    nan["e2"][1234, 1] = np.nan
    far["v0"][77, 2] = -(2.0 ** 41)
    both["v0"][17, 0] = np.nan
    both["v0"][1000, 1] = 2.0 ** 41
    padded = np.concatenate([A.view(np.uint8), np.zeros(16, np.uint8)])
    d_nan, d_far, d_both, d_pad = _dev(nan), _dev(far), _dev(both), _dev(padded)
    too_many = 4 * 4 ** 10 + 1
    cases_ = (
        ("null", raw(ctx, None, n), None, ("null",)),
        ("null before the count", raw(ctx, None, 0), None, ("null",)),
        ("count 0", raw(ctx, dA.data_ptr(), 0), dA, ("count 0",)),
        ("too many before the alignment", raw(ctx, d_pad.data_ptr() + 4, too_many), d_pad, ("too many triangles for a rebuild",)),
        ("offset by 4 bytes", raw(ctx, d_pad.data_ptr() + 4, n), d_pad, ("misaligned",)),
        ("a NaN in 1234", raw(ctx, d_nan.data_ptr(), n), d_nan, ("triangle 1234:", "2^40")),
        ("beyond 2^40 in 77", raw(ctx, d_far.data_ptr(), n), d_far, ("triangle 77:", "2^40")),
        ("the lowest-numbered of two", raw(ctx, d_both.data_ptr(), n), d_both, ("triangle 17:", "2^40")),
        ("host form: a NaN in 1234", lambda lib: lib.wgt_rebuild_triangles(ctx.h, _lib.ptr(nan), n), None, ("triangle 1234:",)),
        ("host form: null", lambda lib: lib.wgt_rebuild_triangles(ctx.h, None, n), None, ("null",)),
        ("host form: count 0", lambda lib: lib.wgt_rebuild_triangles(ctx.h, _lib.ptr(A), 0), None, ("count 0",)),
    )
    for what, call, tensor, words in cases_:
        held = _host(tensor) if tensor is not None else None
        _refused(ctx, call, _lib.WGT_E_INVALID, *words)
        rc.assert_trees_equal(ctx.bvh_read(), tree, what=what)
        assert ctx.scene_info() == info, what
        host_form._same_frame(ctx.render_tile(cam, 32, 32), frame, what)
        if tensor is not None:
            assert np.array_equal(_host(tensor), held), f"{what}: the input was written"
    with pytest.raises(wgt.tracer.WgtError):
        ctx.rebuild_triangles_device(d_nan.data_ptr(), n)
    # a refused rebuild left the refit's level lists usable
    ctx.update_triangles(rc.moved("bunny2000", "jitter5"))
    ctx.update_triangles(A)
    rc.assert_trees_equal(ctx.bvh_read(), tree, what="refit after the refusals")


def test_rebuild_drops_the_motion_snapshot(ctx, wgt):
    """4b. wgt_motion_reproject after a rebuild reports that there is no snapshot, as after an upload."""
    A = rc.mesh("bunny2000")
    L, Q, S = host_form._walls(wgt)
    ctx.upload_scene(L, Q, S, A)
    cam = host_form._camera_at(wgt, A, 1.0, 1, 4)
    ctx.motion_snapshot()
    ctx.sync()
    g = ctx.render_gbuffer(cam, 16, 16)
    ctx.motion_reproject(g)  # fine: a snapshot exists
    ctx.rebuild_triangles(A)
    with pytest.raises(wgt.tracer.WgtError, match="no motion snapshot"):
        ctx.motion_reproject(ctx.render_gbuffer(cam, 16, 16))


def test_input_is_read_after_work_queued_on_the_stream(ctx, wgt):
    """4c. On a torch stream: large matmuls, then a copy of B into the tensor that holds A, then the
    rebuild with that stream's handle and no synchronisation: the tree is B's."""
    import torch

    A, B = rc.mesh("bunny2000"), rc.moved("bunny2000", "jitter5")
    L, Q, S = host_form._tiny_scene(wgt)
    ctx.upload_scene(L, Q, S, A)
    d, dB = _dev(A), _dev(B)
    m = torch.ones((2048, 2048), device=d.device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=d.device)
    with torch.cuda.stream(s):
        for _ in range(8):
            m = (m @ m) * (1.0 / 2048.0)
        d.copy_(dB, non_blocking=True)
    ctx.rebuild_triangles_device(d.data_ptr(), len(A), stream=s.cuda_stream)
    _assert_is_specification(ctx, wgt, B, "after the copy")
    torch.cuda.synchronize()
    assert float(m[0, 0]) == 1.0


def test_rebuild_restores_a_scrambled_mesh(ctx, fresh, wgt):
    """5. The point of the feature, as a condition: bunny2000 with its triangles' positions permuted among
    the indices.  A refit to it keeps the upload's topology, whose every node then spans the mesh; a
    rebuild to it gives the same frame bit for bit with fewer node visits."""
    A, P = rc.mesh("bunny2000"), cases.permuted()
    L, Q, S = host_form._walls(wgt)
    cam = host_form._camera_at(wgt, A, 1.0, 4, 13)
    dP = _dev(P)
    ctx.upload_scene(L, Q, S, A)
    ctx.update_triangles_device(dP.data_ptr(), len(P))
    refit = ctx.render_tile(cam, 32, 32, stats=True)
    ctx.rebuild_triangles_device(dP.data_ptr(), len(P))
    rebuilt = ctx.render_tile(cam, 32, 32, stats=True)
    host_form._same_frame(rebuilt, refit, "rebuilt against refit")
    print(f"node visits: refit {refit['stats']['node_visits']}, rebuilt {rebuilt['stats']['node_visits']}; "
          f"triangle tests: refit {refit['stats']['tri_tests']}, rebuilt {rebuilt['stats']['tri_tests']}")
    assert rebuilt["stats"]["node_visits"] < refit["stats"]["node_visits"]
