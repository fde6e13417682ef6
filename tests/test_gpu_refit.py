"""wgt_update_triangles: the resident BVH refit on the device to moved triangles.

The closest hit does not depend on the tree, so after an update every answer must equal a fresh
upload's bit for bit; and the device tree itself must equal the host specification
(wgt_bvh_refit) bit for bit, which catches a non-conservative box or code even where no test ray
passes.  Meshes and motions: tests/refit_cases.py.  The tree tests use a scene whose light and
dummy sphere lie within 1e-3 of the origin, so that the scene's extent (the compact codes' origin
bound) is the triangles' own, as wgt_bvh_refit takes it; the render and query tests use the
Cornell walls.
"""
import numpy as np
import pytest

import hit_records as hr
import refit_cases as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fresh(wgt):
    """A second context: the fresh uploads the updated one is compared with."""
    c = wgt.Context(0)
    yield c
    c.close()


def _tiny_scene(wgt):
    """One light of 1e-3 x 1e-3 at the origin and the dummy sphere: extent 1e-3, below any mesh's."""
    L, _, S = wgt.cornell_scene()
    L = L.copy()
    L["pos"][0, :3] = 0.0
    L["right"][0, :3] = (1e-3, 0.0, 0.0)
    L["up"][0, :3] = (0.0, 0.0, 1e-3)
    L["norm"][0, :3] = (0.0, -1.0, 0.0)
    L["w"][0] = (0.0, -1e6, 0.0)
    L["d"][0] = 0.0
    assert float(np.abs(S["center"]).max()) + float(np.abs(S["radius"]).max()) <= 1e-3
    return L, L[:0].copy(), S


def _walls(wgt):
    L, Q, S = wgt.cornell_scene()
    return L, Q[:5].copy(), S


def _camera_at(wgt, tris, aspect, spp, seed):
    """The reference camera's view, moved to look at the mesh's centre."""
    v = rc.vertices(tris).reshape(-1, 3)
    c = 0.5 * (v.min(0) + v.max(0))
    cam = wgt.camera_param(aspect, spp, seed)
    cam["origin"] = (c + np.array([0.0, 0.0, -1078.0])).astype(np.float32)
    cam["target"] = c.astype(np.float32)
    return cam


def _same_frame(a, b, what):
    assert np.array_equal(a["f32"].view(np.uint32), b["f32"].view(np.uint32)), f"{what}: rgba32f"
    assert np.array_equal(a["u8"], b["u8"]), f"{what}: rgba8"
    assert np.array_equal(a["hit"], b["hit"]), f"{what}: hit ids"


def _refused(wgt, ctx, tris, n, code, word):
    """The raw call returns `code`, the context's error says why, and nothing was raised."""
    from webgputracer_amd import _lib

    rcode = _lib.lib().wgt_update_triangles(ctx.h, _lib.ptr(tris) if tris is not None else None, n)
    msg = (_lib.lib().wgt_last_error(ctx.h) or b"").decode()
    assert rcode == code, (rcode, msg)
    assert word in msg, msg


@pytest.mark.parametrize("motion", rc.MOTIONS)
@pytest.mark.parametrize("name", rc.MESHES)
def test_tree_equals_host_refit(ctx, wgt, name, motion):
    """1. upload(A), update(B): the resident tree is wgt_bvh_refit(A, B) bit for bit."""
    from webgputracer_amd import _lib

    A, B = rc.mesh(name), rc.moved(name, motion)
    L, Q, S = _tiny_scene(wgt)
    ctx.upload_scene(L, Q, S, A)
    info_a = ctx.scene_info()
    if not rc.within_limits(B):  # the motion left the scene limits: refused, the tree stays
        before = ctx.bvh_read()
        _refused(wgt, ctx, B, len(B), _lib.WGT_E_INVALID, "triangle")
        rc.assert_trees_equal(ctx.bvh_read(), before, what=f"{name} {motion} refused")
        return
    ctx.update_triangles(B)
    info, *want = wgt.bvh_refit(A, B)
    got = ctx.bvh_read()
    print(f"{name} {motion}: {len(got[0])} nodes, step {info_a['bvh_compact_step']} -> {got[4]}")
    rc.assert_trees_equal(got, want, what=f"{name} {motion}")
    now = ctx.scene_info()
    assert now["bvh_compact_step"] == want[4] == info["bvh_compact_step"]
    for k in now:  # everything else is the upload's
        if k not in ("bvh_compact_step", "node_form"):
            assert now[k] == info_a[k], k


@pytest.mark.parametrize("name", rc.MESHES)
def test_round_trip(ctx, wgt, name):
    """2. A -> B -> A gives back the uploaded tree, for every motion within the limits."""
    A = rc.mesh(name)
    L, Q, S = _tiny_scene(wgt)
    ctx.upload_scene(L, Q, S, A)
    uploaded = ctx.bvh_read()
    _, nodes, recs = wgt.bvh_build(A)
    cn, cr, step = wgt.bvh_build_compact(A)
    rc.assert_trees_equal(uploaded, (nodes, recs, cn, cr, step), what=f"{name} upload")  # bvh_read itself
    for motion in rc.MOTIONS[1:]:
        B = rc.moved(name, motion)
        if not rc.within_limits(B):
            continue
        ctx.update_triangles(B)
        ctx.update_triangles(A)
        rc.assert_trees_equal(ctx.bvh_read(), uploaded, what=f"{name} {motion} and back")


def _query_rays(B, n, seed):
    """n / 2 rays aimed at interior points of B's triangles from origins around the mesh, n / 2 random."""
    rng = np.random.default_rng(seed)
    v = rc.vertices(B)
    h = n // 2
    t = rng.integers(0, len(v), h)
    u = rng.uniform(0.05, 0.9, h)
    w = rng.uniform(0.05, 0.95, h) * (1.0 - u)
    p = v[t, 0] + u[:, None] * (v[t, 1] - v[t, 0]) + w[:, None] * (v[t, 2] - v[t, 0])
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    d0 = rng.normal(size=(h, 3))
    d0 /= np.linalg.norm(d0, axis=1, keepdims=True)
    o = 0.5 * (lo + hi) + d0 * 0.6 * np.linalg.norm(hi - lo)  # outside the mesh's bounding sphere
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ro, rd = hr.random_rays(n - h, rng)
    return np.concatenate([o.astype(np.float32), ro]), np.concatenate([d.astype(np.float32), rd])


@pytest.mark.parametrize("motion", ["jitter5", "translate1000"])
def test_queries_equal_a_fresh_upload_and_the_oracle(ctx, fresh, wgt, oracle, motion):
    """3. 50,000 rays after an update: hit records, closest hits and occlusion answers; no ray excluded."""
    A, B = rc.mesh("bunny2000"), rc.moved("bunny2000", motion)
    L, Q, S = _walls(wgt)
    ctx.upload_scene(L, Q, S, A)
    ctx.update_triangles(B)
    fresh.upload_scene(L, Q, S, B)
    o, d = _query_rays(B, 50_000, 3)
    got, want = ctx.trace_hits(o, d), fresh.trace_hits(o, d)
    for f in hr.FIELDS:
        assert np.array_equal(got[f].view(np.uint8), want[f].view(np.uint8)), f
    prim, dist = oracle.OracleScene(L, Q, S, B).trace(o, d)
    nlq = len(L) + len(Q)
    tri = (prim >= nlq) & (prim < nlq + len(B))
    print(f"{motion}: triangle hits {tri.sum()}, misses {(prim == hr.NO_HIT).sum()}")
    assert tri.sum() >= 10_000  # of the 25,000 aimed rays some meet a wall first
    assert np.array_equal(got["prim"], prim) and np.array_equal(hr.bits(got["dist"]), hr.bits(dist))
    p2, d2 = ctx.trace_rays(o, d)
    assert np.array_equal(p2, prim) and np.array_equal(hr.bits(d2), hr.bits(dist))
    hit = prim != hr.NO_HIT
    above = np.nextafter(dist, np.float32(np.inf))
    occ_above, occ_at = ctx.occluded(o, d, above), ctx.occluded(o, d, dist)
    assert np.array_equal(occ_above, hit) and not occ_at.any()
    assert np.array_equal(occ_above, fresh.occluded(o, d, above)) and np.array_equal(occ_at, fresh.occluded(o, d, dist))


@pytest.mark.parametrize("motion", ["jitter5", "translate1000"])
@pytest.mark.parametrize("form", ["default", "WGT_CNODE=0", "WGT_KERNEL=1"])
def test_frames_equal_a_fresh_upload(ctx, fresh, wgt, monkeypatch, form, motion):
    """4. A 64x64, 4 spp frame after an update, in the default form, on the 128-B nodes and in the simple
    kernel.  Counters are not compared (a refit tree's node visits differ from a rebuilt one's)."""
    if form != "default":
        monkeypatch.setenv(*form.split("="))
    A, B = rc.mesh("bunny2000"), rc.moved("bunny2000", motion)
    L, Q, S = _walls(wgt)
    ctx.upload_scene(L, Q, S, A)
    ctx.update_triangles(B)
    fresh.upload_scene(L, Q, S, B)
    cam = _camera_at(wgt, B, 1.0, 4, 11)
    a, b = ctx.render_tile(cam, 64, 64, stats=True), fresh.render_tile(cam, 64, 64)
    tri_px = int(np.sum((a["hit"] >= len(L) + len(Q)) & (a["hit"] < len(L) + len(Q) + len(B))))
    print(f"{form} {motion}: {tri_px} pixels see the mesh")
    assert tri_px >= 100
    _same_frame(a, b, f"{form} {motion}")
    assert a["stats"]["stack_overflows"] == 0


def test_sequence_of_updates(ctx, fresh, wgt):
    """5. Eight successive updates, each a further 45 degrees about the vertical axis."""
    A = rc.mesh("bunny2000")
    L, Q, S = _walls(wgt)
    ctx.upload_scene(L, Q, S, A)
    cam = wgt.camera_param(1.0, 1, 5)
    for k in range(1, 9):
        B = rc.rotate_y(A, 45.0 * k)
        ctx.update_triangles(B)
        fresh.upload_scene(L, Q, S, B)
        _same_frame(ctx.render_tile(cam, 32, 32), fresh.render_tile(cam, 32, 32), f"turn {k}")


def test_update_is_ordered_after_queued_frames(ctx, fresh, wgt):
    """6. Two frames queued on pipeline streams 0 and 1, then an update without synchronising, then a third
    frame: the first two show A, the third B."""
    import torch

    from webgputracer_amd._lib import TILE_DTYPE

    A, B = rc.mesh("bunny2000"), rc.moved("bunny2000", "jitter5")
    L, Q, S = _walls(wgt)
    W, H, spp = 64, 64, 64
    dev = torch.device("cuda", 0)
    ctx.upload_scene(L, Q, S, A)
    streams = [ctx.pipeline_stream(0), ctx.pipeline_stream(1), ctx.pipeline_stream(0)]
    outs, tiles = [], []
    for k in range(3):
        t = np.zeros(1, TILE_DTYPE)
        t["seed"] = 20 + k
        tiles.append(torch.from_numpy(t.view(np.uint8).copy()).to(dev))
        outs.append(torch.zeros((H, W, 4), dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    cam = wgt.camera_param(W / H, spp, 0)
    for k in range(2):
        ctx.render_tiles_async(cam, W, H, W, H, tiles[k].data_ptr(), 1, d_f32=outs[k].data_ptr(), stream=streams[k])
    ctx.update_triangles(B)  # no sync: waits for the two frames itself
    ctx.render_tiles_async(cam, W, H, W, H, tiles[2].data_ptr(), 1, d_f32=outs[2].data_ptr(), stream=streams[2])
    ctx.sync()
    torch.cuda.synchronize()
    for k, T in enumerate((A, A, B)):
        fresh.upload_scene(L, Q, S, T)
        ref = fresh.render_tile(wgt.camera_param(W / H, spp, 20 + k), W, H, want=("f32",))["f32"]
        assert np.array_equal(outs[k].cpu().numpy().view(np.uint32), ref.view(np.uint32)), f"frame {k}"


def test_refusals_leave_the_scene_as_it_was(ctx, wgt):
    """7. Every refusal's status and message, and the tree and a frame afterwards."""
    from webgputracer_amd import _lib

    A = rc.mesh("bunny2000")
    L, Q, S = _walls(wgt)
    with wgt.Context(0) as empty:
        _refused(wgt, empty, A, len(A), _lib.WGT_E_NOSCENE, "no scene")
    ctx.upload_scene(L, Q, S)
    _refused(wgt, ctx, A, len(A), _lib.WGT_E_INVALID, "no triangles")
    ctx.upload_scene(L, Q, S, A)
    cam = wgt.camera_param(1.0, 1, 9)
    tree, frame = ctx.bvh_read(), ctx.render_tile(cam, 32, 32)
    nan, far, long_edge = A.copy(), A.copy(), A.copy()
    nan["v0"][17, 0] = np.nan
    far["v0"][1000, 1] = 2.0 ** 41
    long_edge["e1"][1979, 2] = 2.0 ** 31
    for tris, n, word in ((None, len(A), "null"), (A, len(A) - 1, "count"), (A[:10], 10, "count"),
                          (nan, len(A), "triangle 17"), (far, len(A), "triangle 1000"),
                          (long_edge, len(A), "triangle 1979")):
        _refused(wgt, ctx, tris, n, _lib.WGT_E_INVALID, word)
        rc.assert_trees_equal(ctx.bvh_read(), tree, what=word)
        _same_frame(ctx.render_tile(cam, 32, 32), frame, word)
    with pytest.raises(wgt.tracer.WgtError):
        ctx.update_triangles(far)
