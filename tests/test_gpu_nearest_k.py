"""k-nearest and within-radius closest-point queries on the resident BVH (wgt_nearest_k_points and its forms)
against their definition: every requested field equals wgt_nearest_k_points_spec (the host brute force over
the shared arithmetic of wgt_nearest.h and wgt_nearest_k.h) on the triangles that are resident, bit for bit,
in the count form (count asked for: every triangle within the radius is visited) and in the cull form (no
count: the bound shrinks to the k-th distance).  No tolerance, no excluded point.
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
LISTS = ("prim", "dist", "pos", "uv")
FIELDS = ("count",) + LISTS
N = 512  # points per set


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


def check(ctx, wgt, P, k, what, max_dist=None, tris=None):
    """Both forms of the query on P against the definition on the resident triangles; -> the definition's."""
    T = resident(ctx) if tris is None else tris
    want = wgt.nearest_k_points_spec(T, P, k, max_dist=max_dist, first_prim=first_prim(ctx))
    assert_same(ctx.nearest_k_points(P, k, max_dist=max_dist), want, f"{what}, k = {k}, count form")
    assert_same(ctx.nearest_k_points(P, k, max_dist=max_dist, want=LISTS), want, f"{what}, k = {k}, cull form", fields=LISTS)
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


PLANES = {"count": 1, "prim": 1, "dist": 1, "pos": 3, "uv": 2}


def _dev_outputs(n, k, fill=0x5A):
    """Device buffers of the five fields, every byte `fill`."""
    import torch

    dev = torch.device("cuda", 0)
    return {f: torch.full(((1 if f == "count" else k) * p, 4 * n), fill, dtype=torch.uint8, device=dev) for f, p in PLANES.items()}


def _host_outputs(d, n, k):
    out = {}
    for f, t in d.items():
        a = t.cpu().numpy().copy()
        a = a.view(np.uint32) if f in ("count", "prim") else a.view(f32)
        if f == "count":
            out[f] = a.reshape(n)
        elif f in ("prim", "dist"):
            out[f] = np.ascontiguousarray(a.T)
        else:
            out[f] = np.ascontiguousarray(a.reshape(k, PLANES[f], n).transpose(2, 0, 1))
    return out


def main_sets():
    return (("box", nc.box_points()[:N]), ("surface", nc.surface_points()[:N]))


def upload_bunny(ctx):
    L, Q, S, T = nc.bunny_scene()
    ctx.upload_scene(L, Q, S, T)
    return T


@pytest.fixture(scope="module")
def main_answers(wgt):
    """The definition at k = 32 on the two main point sets without a radius, computed once."""
    T = nc.bunny()
    L, Q, _, _ = nc.bunny_scene()
    return {name: wgt.nearest_k_points_spec(T, P, 32, first_prim=len(L) + len(Q)) for name, P in main_sets()}


@pytest.mark.parametrize("k", [1, 2, 8, 32])
def test_both_point_sets(ctx, wgt, main_answers, k):
    """1. The Cornell walls plus bunny2000, uniform points in the box and points within 2 units of the
    surface: all fields in both forms, each field alone, and entry 0 against the single-triangle query."""
    L, Q, S, T = nc.bunny_scene()
    ctx.upload_scene(L, Q, S, T)
    for name, P in main_sets():
        want = check(ctx, wgt, P, k, name, tris=T)
        assert (want["count"] > 1800).all() and (want["count"] <= len(T)).all()  # all but the zero-area poles' NaNs
        for f in LISTS:  # the list for k is a prefix of the list for 32
            assert np.array_equal(bits(want[f]), bits(main_answers[name][f][:, :k])), (name, f)
        assert (want["prim"] >= len(L) + len(Q)).all() and (want["prim"] < len(L) + len(Q) + len(T)).all()
        for f in FIELDS:
            one = ctx.nearest_k_points(P, k, want=(f,))
            assert list(one) == [f]
            assert_same(one, want, f"{name}, k = {k}, {f} alone", fields=(f,))
        single = ctx.nearest_points(P)
        for f in LISTS:
            assert np.array_equal(bits(want[f][:, 0]), bits(single[f])), (name, f)


def test_radius(ctx, wgt, main_answers):
    """2. max_dist = 0.5 D, D, the float above D, 2 D, +inf, 0, -1, NaN and one float below, at and above D,
    for D the 1st and the k-th distance; NULL = +inf; the count alone with a radius that holds about ten
    triangles."""
    L, Q, S, T = nc.bunny_scene()
    ctx.upload_scene(L, Q, S, T)
    for name, P in main_sets():
        P = P[:256]
        free = {f: a[:256] for f, a in main_answers[name].items()}
        for k in (1, 8):
            for j in sorted({0, k - 1}):
                D = free["dist"][:, j]
                for lim in nc.radius_sets(D) + nc.around(D):
                    want = check(ctx, wgt, P, k, f"{name} radius", max_dist=lim, tris=T)
                    single = ctx.nearest_points(P, max_dist=lim)
                    for f in LISTS:
                        assert np.array_equal(bits(want[f][:, 0]), bits(single[f])), (name, f)
                # below and at the (j+1)-th distance j triangles at least, above it j + 1 at least
                c = [wgt.nearest_k_points_spec(T, P, k, max_dist=m, want=("count",))["count"] for m in nc.around(D)]
                assert (c[0] <= c[1]).all() and (c[1] <= c[2]).all() and (c[2] >= j + 1).all() and (c[1] <= c[2] - 1).all()
        assert_same(ctx.nearest_k_points(P, 8, max_dist=np.inf), ctx.nearest_k_points(P, 8), "NULL radius = +inf")
        # the count alone (k is ignored), at the float above each point's 10th distance
        lim = np.nextafter(free["dist"][:, 9], INF)
        want = wgt.nearest_k_points_spec(T, P, 0, max_dist=lim, want=("count",))
        assert (want["count"] >= 10).all() and np.median(want["count"]) < 16
        for k in (0, 5, 99):
            assert_same(ctx.nearest_k_points(P, k, max_dist=lim, want=("count",)), want, "count alone", fields=("count",))


def test_ties_and_degenerates(ctx, wgt):
    """3. Ties at the k-th bound.  64 exact copies: k = 1 and 32 keep the lowest ids (a later triangle with
    d2 == D and a lower id still enters), k = 31 likewise with a list one entry shorter; 300
    copies and the doubled coplanar mesh likewise; zero-area triangles never enter with a NaN; NaN and
    infinite points give empty records."""
    L, Q, S, T = nc.bunny_scene()
    P = nc.small_points()
    fp = len(L) + len(Q)
    ctx.upload_scene(L, Q, S, nc.copies64())
    for k in (1, 32, 31):
        want = check(ctx, wgt, P, k, "64 copies")
        assert (want["count"] == 64).all() and (want["prim"] == fp + np.arange(k, dtype=np.uint32)[None, :]).all()
    for name in ("copies300", "coplanar_x2"):
        Lm, Qm, Sm = am.scene_parts(name)
        ctx.upload_scene(Lm, Qm, Sm, am.small_mesh(name))
        for k in (1, 8, 32):
            check(ctx, wgt, P, k, name)
    for name, mesh in (("degenerate among ordinary", nc.degenerate_mix()), ("degenerate only", nc.degenerate_only())):
        ctx.upload_scene(L, Q, S, mesh)
        for k in (1, 8, 32):
            want = check(ctx, wgt, P, k, name)
            assert not np.isnan(want["dist"]).any()
    ctx.upload_scene(L, Q, S, T)
    want = check(ctx, wgt, nc.bad_points(), 8, "NaN and infinite points", tris=T)
    odd = ~np.isfinite(nc.bad_points()).all(1)
    assert (want["count"][odd] == 0).all() and (want["prim"][odd] == NO_HIT).all() and np.isposinf(want["dist"][odd]).all()
    assert (want["count"][~odd] > 8).all() and (want["prim"][~odd] != NO_HIT).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_point_counts(ctx, wgt, n):
    """4. Around the wave and the workgroup size."""
    T = upload_bunny(ctx)
    check(ctx, wgt, nc.box_points()[:n], 8, f"n = {n}", tris=T)
    assert ctx.nearest_k_points(np.zeros((0, 3), f32), 8)["prim"].shape == (0, 8)


def test_scenes_at_the_limits(ctx, wgt):
    """5. No triangles: empty records.  One triangle at k = 32 and five at k = 8: the lists are padded."""
    L, Q, S, T = nc.bunny_scene()
    P = nc.small_points()
    ctx.upload_scene(L, Q, S)
    for want in (FIELDS, LISTS):
        got = ctx.nearest_k_points(P, 4, want=want)
        assert (got["prim"] == NO_HIT).all() and np.isposinf(got["dist"]).all() and not got["pos"].any() and not got["uv"].any()
    assert not ctx.nearest_k_points(P, 4)["count"].any()
    ctx.upload_scene(L, Q, S, T[7:8])
    assert ctx.scene_info()["bvh_nodes"] == 1
    want = check(ctx, wgt, P, 32, "one triangle")
    assert (want["count"] == 1).all() and (want["prim"][:, 0] == len(L) + len(Q)).all() and (want["prim"][:, 1:] == NO_HIT).all()
    area = np.linalg.norm(np.cross(T["e1"][:, :3].astype(np.float64), T["e2"][:, :3].astype(np.float64)), axis=1)
    ctx.upload_scene(L, Q, S, T[np.flatnonzero(area > 0.0)[100:105]])
    want = check(ctx, wgt, P, 8, "five triangles")
    assert (want["count"] == 5).all() and (want["prim"][:, 5:] == NO_HIT).all() and (want["prim"][:, :5] != NO_HIT).all()


def test_points_beyond_the_cull_range(ctx, wgt):
    """6. |px| + |py| + |pz| above 2^40: nothing is culled, every record is scanned, the definition verbatim."""
    T = upload_bunny(ctx)
    rng = np.random.default_rng(6)
    P = (rng.uniform(0.5, 1.0, (256, 3)) * 2.0 ** 41 * rng.choice([-1.0, 1.0], (256, 3))).astype(f32)
    P[::4] = (rng.uniform(0.34, 0.4, (64, 3)) * 2.0 ** 40 * rng.choice([-1.0, 1.0], (64, 3))).astype(f32)  # just above
    assert (np.abs(P.astype(np.float64)).sum(1) > 2.0 ** 40).all()
    for k in (1, 8, 32):
        want = check(ctx, wgt, P, k, "beyond 2^40", tris=T)
    assert (want["count"] > 1800).all()
    D = want["dist"][:, 7]
    for lim in nc.around(D):
        check(ctx, wgt, P, 8, "beyond 2^40, radius", max_dist=lim, tris=T)


def test_far_and_scaled(ctx, wgt):
    """7. Points about 1e5 units from the mesh, with radii around the k-th distance; the mesh and the points
    scaled by 2^-12 and 2^20."""
    L, Q, S, T = nc.bunny_scene()
    ctx.upload_scene(L, Q, S, T)
    P = nc.far_points(1e5)[:N]
    for k in (1, 8, 32):
        want = check(ctx, wgt, P, k, "far 1e5", tris=T)
        assert (want["prim"] != NO_HIT).all()
    for lim in nc.around(want["dist"][:, 7]):
        check(ctx, wgt, P, 8, "far 1e5 radius", max_dist=lim, tris=T)
    for scale in nc.SCALES:
        Ts = nc.scaled(T, scale)
        ctx.upload_scene(L, Q[:0], S, Ts)
        for name, P in main_sets():
            for k in (1, 8, 32):
                want = check(ctx, wgt, P * f32(scale), k, f"{name} x {scale:g}", tris=Ts)
                assert (want["prim"] != NO_HIT).all()


@pytest.mark.parametrize("name", am.GPU)
def test_hard_meshes(ctx, wgt, name):
    """8. The meshes that reach the builder's depth limit and the stack bound, at k = 8 in both forms."""
    L, Q, S = am.scene_parts(name)
    T = am.small_mesh(name)
    ctx.upload_scene(L, Q, S, T)
    rng = np.random.default_rng(11)
    idx = rng.integers(0, len(T), N)
    c = nc.centroids(T, idx)
    near = (c + rng.normal(size=c.shape) * (0.05 * np.linalg.norm(c, axis=1, keepdims=True) + 5.0)).astype(f32)
    P = np.concatenate([near, nc.small_points(N, 4)])
    want = check(ctx, wgt, P, 8, name)
    check(ctx, wgt, P, 8, name + ", radius", max_dist=np.nextafter(want["dist"][:, 3], INF))


def test_the_mesh_moves(ctx, wgt):
    """9. One context through update_triangles, update_vertices_device with an index buffer, a rebuild to a
    different count and a refit of the rebuilt tree: after each the answers equal the definition on the
    triangles wgt_bvh_read returns."""
    L, Q, S, _ = nc.bunny_scene()
    A = rc.mesh("bunny2000")
    P = np.concatenate([nc.box_points()[:N], nc.surface_points()[:N]])
    ctx.upload_scene(L, Q, S, A)
    check(ctx, wgt, P, 8, "upload")
    ctx.update_triangles(rc.moved("bunny2000", "jitter5"))
    check(ctx, wgt, P, 8, "update_triangles")
    V = rc.vertices(rc.moved("bunny2000", "translate1000")).astype(f32)
    rows = rc.bits(V.reshape(-1, 3))
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    verts, index = np.ascontiguousarray(uniq).view(f32), np.asarray(inv).reshape(-1, 3).astype(np.uint32)
    dv, di = _dev(verts), _dev(index)
    ctx.update_vertices_device(dv.data_ptr(), len(verts), len(A), d_index=di.data_ptr())
    want = check(ctx, wgt, P, 8, "update_vertices_device, indexed")
    assert np.array_equal(bits(resident(ctx)["v0"][:, :3]), bits(V[:, 0]))
    assert (want["prim"] != NO_HIT).all()
    ctx.rebuild_triangles(A[::4])
    assert ctx.scene_info()["n_tris"] == len(A[::4])
    check(ctx, wgt, P, 8, "rebuild to a different count")
    check(ctx, wgt, P, 32, "rebuild to a different count")
    moved = A[::4].copy()
    moved["v0"][:, :3] += np.random.default_rng(5).normal(0.0, 3.0, (len(moved), 3)).astype(f32)
    ctx.update_triangles(moved)
    check(ctx, wgt, P, 8, "refit of the rebuilt tree")


def test_async_behind_a_device_update(ctx, wgt):
    """10. The async call on torch device tensors on wgt_pipeline_stream(1), behind a device update on the
    same stream: the answers see the new triangles; a field that is not asked for is not written."""
    import torch

    L, Q, S, _ = nc.bunny_scene()
    A, B = rc.mesh("bunny2000"), rc.moved("bunny2000", "jitter5")
    ctx.upload_scene(L, Q, S, A)
    P = nc.surface_points()[:N]
    n, k = len(P), 8
    s = ctx.pipeline_stream(1)
    dP, dB, out = _dev(np.ascontiguousarray(P.T)), _dev(B), _dev_outputs(n, k)
    ctx.update_triangles_device(dB.data_ptr(), len(B), stream=s)
    ctx.nearest_k_points_async(dP.data_ptr(), n, k, stream=s, **{f: t.data_ptr() for f, t in out.items()})
    torch.cuda.synchronize()
    T = resident(ctx)
    assert np.array_equal(bits(T["v0"][:, :3]), bits(B["v0"][:, :3]))
    lim = np.full(n, 6.0, f32)
    want = wgt.nearest_k_points_spec(T, P, k, first_prim=len(L) + len(Q))
    assert_same(_host_outputs(out, n, k), want, "async after the update")
    before = wgt.nearest_k_points_spec(A, P, k, first_prim=len(L) + len(Q))
    assert (bits(before["dist"]) != bits(want["dist"])).mean() > 0.5  # the update matters
    want = wgt.nearest_k_points_spec(T, P, k, max_dist=lim, first_prim=len(L) + len(Q))
    dL = _dev(lim)
    for asked in (("dist",), ("count",), ("uv", "prim"), ("count", "pos")):
        out2 = _dev_outputs(n, k)
        ctx.nearest_k_points_async(dP.data_ptr(), n, k, d_max_dist=dL.data_ptr(), stream=s, **{f: out2[f].data_ptr() for f in asked})
        torch.cuda.synchronize()
        assert_same(_host_outputs({f: out2[f] for f in asked}, n, k), want, f"{asked} alone", fields=asked)
        for f in FIELDS:
            if f not in asked:
                assert bool((out2[f] == 0x5A).all()), (asked, f)


def test_the_tree_is_used(ctx, wgt):
    """11. The counting kernel on bunny2000's near-surface set.  The cull form's triangle tests per point at
    k = 32 stay below the scan's 1,980; at k = 1 without a radius the traversal is wgt_nearest_points' own
    (the same bound after the same insertions, the same descent order), so both counts are equal; the
    counting kernel's answers equal the plain call's in both forms."""
    L, Q, S, T = nc.bunny_scene()
    ctx.upload_scene(L, Q, S, T)
    P = nc.surface_points()[:N]
    n = len(P)
    dP = _dev(np.ascontiguousarray(P.T))
    per_point = {}
    for k in (1, 8, 32):
        out = _dev_outputs(n, k)
        nodes, tests = ctx.nearest_k_points_stats(dP.data_ptr(), n, k, **{f: out[f].data_ptr() for f in LISTS})
        per_point[k] = (nodes / n, tests / n)
        print(f"cull form, k = {k}: {nodes / n:.1f} node visits and {tests / n:.1f} triangle tests per point of {len(T)} triangles")
        assert_same(_host_outputs({f: out[f] for f in LISTS}, n, k), ctx.nearest_k_points(P, k, want=LISTS), "counting against plain", fields=LISTS)
        assert nodes >= n
        if k == 1:
            single = {f: t for f, t in _dev_outputs(n, 1).items() if f != "count"}
            assert (nodes, tests) == ctx.nearest_points_stats(dP.data_ptr(), n, **{f: t.data_ptr() for f, t in single.items()})
    assert 0 < per_point[32][1] < len(T)
    lim = _dev(np.full(n, 4.0, f32))
    out = _dev_outputs(n, 8)
    nodes, tests = ctx.nearest_k_points_stats(dP.data_ptr(), n, 8, d_max_dist=lim.data_ptr(), **{f: t.data_ptr() for f, t in out.items()})
    print(f"count form, radius 4, k = 8: {nodes / n:.1f} node visits and {tests / n:.1f} triangle tests per point")
    assert_same(_host_outputs(out, n, 8), wgt.nearest_k_points_spec(T, P, 8, max_dist=4.0, first_prim=len(L) + len(Q)), "count form, counting")
    assert 0 < tests / n < len(T)
