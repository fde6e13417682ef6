"""Closest-point queries on the resident BVH (wgt_nearest_points and its forms) against their definition:
every requested field equals wgt_nearest_points_spec (the host brute force over the shared arithmetic of
wgt_nearest.h) on the triangles that are resident, bit for bit.  No tolerance, no excluded point.
"""
import numpy as np
import pytest

import adversarial_meshes as am
import nearest_cases as nc
import refit_cases as rc

pytestmark = pytest.mark.gpu

f32 = np.float32
NO_HIT = np.uint32(0xFFFFFFFF)
INF = f32(np.inf)
FIELDS = ("prim", "dist", "pos", "uv")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what, fields=FIELDS):
    for k in fields:
        g, w = bits(got[k]), bits(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
        assert bad.size == 0, (f"{what}: {k} differs at {bad.size} of {len(g)} points; first {bad[0]}: got {got[k][bad[0]]!r}, "
                               f"the definition gives {want[k][bad[0]]!r}")


def resident(ctx):
    """The resident triangles in original order (v0, e1, e2 of wgt_bvh_read's records)."""
    import webgputracer_amd as wgt

    recs = ctx.bvh_read()[1]
    T = np.zeros(len(recs), wgt.tracer.TRI_DTYPE)
    idx = bits(recs[:, 0, 3]).astype(np.int64)
    assert np.array_equal(np.sort(idx), np.arange(len(recs)))
    for k, row in (("v0", 0), ("e1", 1), ("e2", 2)):
        T[k][idx, :3] = recs[:, row, :3]
    return T


def first_prim(ctx):
    info = ctx.scene_info()
    return info["n_lights"] + info["n_quads"]


def check(ctx, wgt, P, what, max_dist=None, tris=None):
    """The query on P against the definition on the resident triangles; -> the definition's answers."""
    T = resident(ctx) if tris is None else tris
    want = wgt.nearest_points_spec(T, P, max_dist=max_dist, first_prim=first_prim(ctx))
    assert_same(ctx.nearest_points(P, max_dist=max_dist), want, what)
    return want


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.uint8)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(a.copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _dev_outputs(n, fill=0x5A):
    """Device buffers of the four fields, every byte `fill`."""
    import torch

    dev = torch.device("cuda", 0)
    shape = {"prim": (n,), "dist": (n,), "pos": (3, n), "uv": (2, n)}
    return {k: torch.full(tuple(4 * x if i == len(s) - 1 else x for i, x in enumerate(s)), fill, dtype=torch.uint8, device=dev)
            for k, s in shape.items()}


def _host_outputs(d):
    out = {}
    for k, t in d.items():
        a = t.cpu().numpy().copy()
        a = a.view(np.uint32) if k == "prim" else a.view(f32)
        out[k] = np.ascontiguousarray(a.T) if k in ("pos", "uv") else a
    return out


@pytest.fixture(scope="module")
def bunny_ctx(ctx):
    L, Q, S, T = nc.bunny_scene()
    ctx.upload_scene(L, Q, S, T)
    return ctx, T, len(L) + len(Q)


@pytest.fixture(scope="module")
def main_answers(wgt):
    """The definition on the two main point sets, computed once."""
    T = nc.bunny()
    L, Q, _, _ = nc.bunny_scene()
    fp = len(L) + len(Q)
    return {"box": wgt.nearest_points_spec(T, nc.box_points(), first_prim=fp),
            "surface": wgt.nearest_points_spec(T, nc.surface_points(), first_prim=fp)}


def test_both_point_sets(ctx, wgt, main_answers):
    """1. The Cornell walls plus bunny2000, uniform points in the box and points within 2 units of the
    surface: all four outputs, then each output alone."""
    L, Q, S, T = nc.bunny_scene()
    ctx.upload_scene(L, Q, S, T)
    assert np.array_equal(bits(resident(ctx)["e1"][:, :3]), bits(T["e1"][:, :3]))  # an upload keeps the caller's bits
    for name, P in (("box", nc.box_points()), ("surface", nc.surface_points())):
        want = main_answers[name]
        assert (want["prim"] >= len(L) + len(Q)).all() and (want["prim"] < len(L) + len(Q) + len(T)).all()
        assert_same(ctx.nearest_points(P), want, name)
        for k in FIELDS:
            one = ctx.nearest_points(P, want=(k,))
            assert list(one) == [k]
            assert_same(one, want, f"{name}, {k} alone", fields=(k,))


def test_radius(ctx, wgt, main_answers):
    """2. max_dist = 0.5 D, D, the float above D, 2 D, +inf, 0, -1, NaN per point; NULL = +inf."""
    L, Q, S, T = nc.bunny_scene()
    ctx.upload_scene(L, Q, S, T)
    for name, P in (("box", nc.box_points()[:1500]), ("surface", nc.surface_points()[:1500])):
        D = main_answers[name]["dist"][:1500]
        hits = []
        for lim in nc.radius_sets(D):
            want = check(ctx, wgt, P, f"{name} radius", max_dist=lim, tris=T)
            hits.append(want["prim"] != NO_HIT)
        assert [h.all() for h in hits] == [False, False, True, True, True, False, False, False]
        assert [h.any() for h in hits] == [False, False, True, True, True, False, False, False]
        assert_same(ctx.nearest_points(P, max_dist=np.inf), ctx.nearest_points(P), "NULL radius = +inf")


@pytest.mark.parametrize("back", nc.FAR)
def test_far_points(ctx, wgt, back):
    """3. Points about `back` units from random centroids, without a radius and with max_dist one float
    below, at and above the distance: where a cull that ignores what the arithmetic loses far from the
    mesh goes wrong."""
    L, Q, S, T = nc.bunny_scene()
    ctx.upload_scene(L, Q, S, T)
    P = nc.far_points(back)
    want = check(ctx, wgt, P, f"far {back:g}", tris=T)
    assert (want["prim"] != NO_HIT).all()
    for lim, hit in zip(nc.around(want["dist"]), (False, False, True)):
        w = check(ctx, wgt, P, f"far {back:g} radius", max_dist=lim, tris=T)
        assert ((w["prim"] != NO_HIT) == hit).all()


@pytest.mark.parametrize("scale", nc.SCALES)
def test_scale(ctx, wgt, scale):
    """4. The mesh and the points scaled by a power of two."""
    L, Q, S, T = nc.bunny_scene()
    Ts = nc.scaled(T, scale)
    ctx.upload_scene(L, Q[:0], S, Ts)
    for name, P in (("box", nc.box_points()[:1500]), ("surface", nc.surface_points()[:1500])):
        want = check(ctx, wgt, P * f32(scale), f"{name} x {scale:g}", tris=Ts)
        assert (want["prim"] != NO_HIT).all()


def test_ties_and_degenerates(ctx, wgt):
    """5. 64 exact copies give the lowest id; zero-area triangles never win with a NaN; a mesh of nothing
    but such triangles gives what the definition gives; NaN and infinite points give the miss record."""
    L, Q, S, T = nc.bunny_scene()
    P = nc.small_points()
    ctx.upload_scene(L, Q, S, nc.copies64())
    want = check(ctx, wgt, P, "64 copies")
    assert (want["prim"] == len(L) + len(Q)).all()
    for name, mesh in (("degenerate among ordinary", nc.degenerate_mix()), ("degenerate only", nc.degenerate_only())):
        ctx.upload_scene(L, Q, S, mesh)
        want = check(ctx, wgt, P, name)
        assert not np.isnan(want["dist"]).any()
    ctx.upload_scene(L, Q, S, T)
    want = check(ctx, wgt, nc.bad_points(), "NaN and infinite points", tris=T)
    odd = ~np.isfinite(nc.bad_points()).all(1)
    assert (want["prim"][odd] == NO_HIT).all() and np.isposinf(want["dist"][odd]).all()
    assert (want["prim"][~odd] != NO_HIT).all()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_point_counts(bunny_ctx, wgt, main_answers, n):
    """6a. Around the workgroup size."""
    ctx, T, fp = bunny_ctx
    want = {k: v[:n] for k, v in main_answers["box"].items()}
    assert_same(ctx.nearest_points(nc.box_points()[:n]), want, f"n = {n}")


def test_scenes_at_the_limits(ctx, wgt):
    """6b. No triangles: all misses.  One triangle: the root with a single leaf."""
    L, Q, S, T = nc.bunny_scene()
    P = nc.small_points()
    ctx.upload_scene(L, Q, S)
    got = ctx.nearest_points(P)
    assert (got["prim"] == NO_HIT).all() and np.isposinf(got["dist"]).all() and not got["pos"].any() and not got["uv"].any()
    ctx.upload_scene(L, Q, S, T[7:8])
    assert ctx.scene_info()["bvh_nodes"] == 1
    want = check(ctx, wgt, P, "one triangle")
    assert (want["prim"] == len(L) + len(Q)).all()


@pytest.mark.parametrize("name", am.GPU)
def test_hard_meshes(ctx, wgt, name):
    """6c. The meshes that reach the builder's depth limit and the stack bound: the nearest-first order
    pushes differently from a ray's, and the bound has to hold all the same."""
    L, Q, S = am.scene_parts(name)
    T = am.small_mesh(name)
    ctx.upload_scene(L, Q, S, T)
    rng = np.random.default_rng(11)
    idx = rng.integers(0, len(T), 1000)
    c = nc.centroids(T, idx)
    near = (c + rng.normal(size=c.shape) * (0.05 * np.linalg.norm(c, axis=1, keepdims=True) + 5.0)).astype(f32)
    P = np.concatenate([near, nc.small_points(1000, 4)])
    check(ctx, wgt, P, name)


def test_the_mesh_moves(ctx, wgt):
    """7. One context through update_triangles, update_vertices_device with an index buffer, a rebuild to
    a smaller count and to a larger one, and a refit of the rebuilt tree: after each the answers equal
    the definition on the triangles wgt_bvh_read returns."""
    L, Q, S, _ = nc.bunny_scene()
    A = rc.mesh("bunny2000")
    P = np.concatenate([nc.box_points()[:1000], nc.surface_points()[:1000]])
    ctx.upload_scene(L, Q, S, A)
    check(ctx, wgt, P, "upload")
    ctx.update_triangles(rc.moved("bunny2000", "jitter5"))
    check(ctx, wgt, P, "update_triangles")
    V = rc.vertices(rc.moved("bunny2000", "translate1000")).astype(f32)
    rows = rc.bits(V.reshape(-1, 3))
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    verts, index = np.ascontiguousarray(uniq).view(f32), np.asarray(inv).reshape(-1, 3).astype(np.uint32)
    dv, di = _dev(verts), _dev(index)
    ctx.update_vertices_device(dv.data_ptr(), len(verts), len(A), d_index=di.data_ptr())
    want = check(ctx, wgt, P, "update_vertices_device, indexed")
    assert np.array_equal(bits(resident(ctx)["v0"][:, :3]), bits(V[:, 0]))
    assert (want["prim"] != NO_HIT).all()
    ctx.rebuild_triangles(A[::4])
    assert ctx.scene_info()["n_tris"] == len(A[::4])
    check(ctx, wgt, P, "rebuild, smaller")
    big = wgt.procedural_mesh("bunny", 5000)
    ctx.rebuild_triangles(big)
    check(ctx, wgt, P, "rebuild, larger")
    moved = big.copy()
    moved["v0"][:, :3] += np.random.default_rng(5).normal(0.0, 3.0, (len(big), 3)).astype(f32)
    ctx.update_triangles(moved)
    check(ctx, wgt, P, "refit of the rebuilt tree")


def test_async_behind_a_device_update(ctx, wgt):
    """8. The async call on torch device tensors on wgt_pipeline_stream(1), behind a device update on the
    same stream: the answers see the new triangles."""
    import torch

    L, Q, S, _ = nc.bunny_scene()
    A, B = rc.mesh("bunny2000"), rc.moved("bunny2000", "jitter5")
    ctx.upload_scene(L, Q, S, A)
    P = nc.surface_points()[:2000]
    n = len(P)
    s = ctx.pipeline_stream(1)
    dP, dB, out = _dev(np.ascontiguousarray(P.T)), _dev(B), _dev_outputs(n)
    ctx.update_triangles_device(dB.data_ptr(), len(B), stream=s)
    ctx.nearest_points_async(dP.data_ptr(), n, stream=s, **{k: t.data_ptr() for k, t in out.items()})
    torch.cuda.synchronize()
    T = resident(ctx)
    assert np.array_equal(bits(T["v0"][:, :3]), bits(B["v0"][:, :3]))
    want = wgt.nearest_points_spec(T, P, first_prim=len(L) + len(Q))
    assert_same(_host_outputs(out), want, "async after the update")
    before = wgt.nearest_points_spec(A, P, first_prim=len(L) + len(Q))
    assert (bits(before["dist"]) != bits(want["dist"])).mean() > 0.5  # the update matters
    # a field that is not asked for is not written
    out2 = _dev_outputs(n)
    ctx.nearest_points_async(dP.data_ptr(), n, stream=s, dist=out2["dist"].data_ptr())
    torch.cuda.synchronize()
    assert_same(_host_outputs({"dist": out2["dist"]}), want, "dist alone", fields=("dist",))
    for k in ("prim", "pos", "uv"):
        assert bool((out2[k] == 0x5A).all()), k


def test_the_tree_is_used(ctx, wgt, main_answers):
    """9. On bunny2000 with the near-surface set the counting kernel reports fewer than n_tris / 4 triangle
    tests per point (a brute-force scan reports n_tris), and its answers equal the plain call's."""
    L, Q, S, T = nc.bunny_scene()
    ctx.upload_scene(L, Q, S, T)
    P = nc.surface_points()
    n = len(P)
    dP, out = _dev(np.ascontiguousarray(P.T)), _dev_outputs(n)
    nodes, tests = ctx.nearest_points_stats(dP.data_ptr(), n, **{k: t.data_ptr() for k, t in out.items()})
    print(f"near-surface set: {nodes / n:.1f} node visits and {tests / n:.1f} triangle tests per point of {len(T)} triangles")
    assert 0 < tests / n < len(T) / 4 and nodes >= n
    got = _host_outputs(out)
    assert_same(got, ctx.nearest_points(P), "counting against plain")
    assert_same(got, main_answers["surface"], "counting against the definition")
