"""Multi-hit queries, wgt_trace_multi_hits, against their specification (tests/multihit_spec.py: every
primitive tested alone by the untouched CPU oracle, the limit rule, the order (dist, primitive id)).  The
definition is exact, so every comparison here is equality: no tolerance, no excluded rays.

"count mode" asks for count, prim and dist (every hit is visited); "cull mode" for prim and dist only
(the search stops looking beyond the k-th distance).  Both must give the specification's prim and dist.
"""
import ctypes

import numpy as np
import pytest

import multihit_spec as ms

pytestmark = pytest.mark.gpu

NO_HIT = ms.NO_HIT
INF = ms.INF
BOTH = ("count", "cull")


def _query(ctx, o, d, k, mode, max_dist=None, tris_only=False):
    want = ("count", "prim", "dist") if mode == "count" else ("prim", "dist")
    return ctx.trace_multi_hits(o, d, k, max_dist=max_dist, tris_only=tris_only, want=want)


def _check(ctx, spec, o, d, k, max_dist=None, tris_only=False, modes=BOTH, what=""):
    """Both modes against the specification; -> the specification's answer."""
    want = spec.answer(k, max_dist, tris_only)
    for mode in modes:
        ms.assert_equal(_query(ctx, o, d, k, mode, max_dist, tris_only), want, f"{what} k={k} {mode} mode")
    return want


# ------------------------------------------------------------------ scenes and their specifications, computed once
@pytest.fixture(scope="module")
def spheres(wgt, oracle):
    """The Cornell box plus three concentric UV spheres (504 triangles), 4,000 random rays."""
    scene = ms.concentric_scene(wgt)
    o, d = ms.random_rays(4000, np.random.default_rng(0))
    return scene, o, d, ms.MultiHitSpec(oracle, *scene, o, d)


@pytest.fixture(scope="module")
def bunny(wgt):
    """The Cornell walls and a 2,000-triangle bunny stand-in (tests/test_gpu_occlusion.py's scene)."""
    return wgt.mesh_scene("bunny", 2000)


@pytest.fixture(scope="module")
def bunny_box(bunny, oracle):
    o, d = ms.random_rays(4000, np.random.default_rng(0))
    return o, d, ms.MultiHitSpec(oracle, *bunny, o, d)


# ------------------------------------------------------------------ 1
@pytest.mark.parametrize("k", [1, 2, 4, 8, 32])
def test_concentric_spheres(ctx, spheres, k):
    """1. Counts below, equal to and above k; both modes; n = 4,000 and the tail-lane sizes 1, 63, 65."""
    scene, o, d, spec = spheres
    ctx.upload_scene(*scene)
    want = _check(ctx, spec, o, d, k, what="spheres")
    c = want["count"]
    print(f"k={k}: counts {c.min()}..{c.max()}, below {np.count_nonzero(c < k)}, equal {np.count_nonzero(c == k)}, "
          f"above {np.count_nonzero(c > k)}")
    if k in (2, 4, 8):
        assert (c < k).any() and (c == k).any() and (c > k).any()
    for n in (1, 63, 65):
        for mode in BOTH:
            got = _query(ctx, o[:n], d[:n], k, mode)
            ms.assert_equal(got, {f: want[f][:n] for f in got}, f"n={n} k={k} {mode} mode")


# ------------------------------------------------------------------ 2
@pytest.fixture(scope="module")
def stack_of_squares(wgt, oracle):
    """40 squares of side 200 in the planes z = 100 + 5 j, two triangles each, the whole set twice (the
    duplicates at the higher ids); 2,000 rays from z = 20 along (N(0, .05), N(0, .05), 1), the first 200
    exactly axis-parallel."""
    z = 100.0 + 5.0 * np.arange(40)
    a = np.stack([np.full(40, 100.0), np.full(40, 100.0), z], 1)
    b, c, e = a + (200.0, 0, 0), a + (200.0, 200.0, 0), a + (0, 200.0, 0)
    one = np.stack([np.stack([a, b, c], 1), np.stack([a, c, e], 1)], 1).reshape(-1, 3, 3)
    T = wgt.make_triangles(np.concatenate([one, one]).astype(np.float32))
    L, Q, S = wgt.cornell_scene()
    rng = np.random.default_rng(11)
    n = 2000
    o = np.stack([rng.uniform(110, 290, n), rng.uniform(110, 290, n), np.full(n, 20.0)], 1).astype(np.float32)
    d = np.stack([rng.normal(0, 0.05, n), rng.normal(0, 0.05, n), np.ones(n)], 1).astype(np.float32)
    d[:200, :2] = 0.0
    return (L, Q, S, T), o, d, ms.MultiHitSpec(oracle, L, Q, S, T, o, d)


@pytest.mark.parametrize("k", [32, 31])
def test_more_hits_than_the_list_holds(ctx, stack_of_squares, k):
    """2. Most rays cross 80 triangles, in 40 tied pairs: the list overflows, and k = 31 cuts inside a pair."""
    scene, o, d, spec = stack_of_squares
    assert len(scene[3]) == 160
    ctx.upload_scene(*scene)
    want = _check(ctx, spec, o, d, k, tris_only=True, what="squares")
    c = want["count"]
    print(f"counts: median {np.median(c)}, max {c.max()}, share >= 66: {np.mean(c >= 66):.3f}, > 32: {np.mean(c > 32):.3f}")
    assert np.median(c) == 80 and c.max() == 80 and (c[:200] == 80).all()
    assert np.mean(c > 32) >= 0.9
    full = spec.answer(34, tris_only=True)["dist"][:200]
    assert (full[:, 30] == full[:, 31]).all() and (full[:, 32] == full[:, 33]).all()
    if k == 31:  # the last kept entry is the lower id of its tied pair
        pair = spec.answer(32, tris_only=True)["prim"][:200, 30:32]
        assert (want["prim"][:200, 30] == pair.min(1)).all()


# ------------------------------------------------------------------ 3
def test_limits_around_the_second_distance(ctx, spheres):
    """3a. max_dist = 0.5 D2, D2, the float above D2 and +inf per ray, D2 the specification's second distance."""
    scene, o, d, spec = spheres
    ctx.upload_scene(*scene)
    D2 = spec.answer(2)["dist"][:, 1]
    assert np.count_nonzero(np.isfinite(D2)) >= 1000
    for name, lim in (("0.5 D2", np.float32(0.5) * D2), ("D2", D2), ("above D2", np.nextafter(D2, INF)),
                      ("+inf", np.full_like(D2, INF))):
        want = _check(ctx, spec, o, d, 4, max_dist=lim, what=f"limit {name}")
        if name == "D2":  # the second hit itself is not below its own distance
            assert (want["count"][np.isfinite(D2)] <= 1).all()
        if name == "above D2":
            assert (want["count"][np.isfinite(D2)] >= 2).all()


def test_nan_and_degenerate(ctx, bunny, oracle):
    """3b. The five rays of test_gpu_occlusion.test_nan_and_degenerate x max_dist in {NaN, -1, 0, 1e-3, 1e3, +inf}."""
    ctx.upload_scene(*bunny)
    o = np.array([[278, 278, -800], [np.nan, 1, 1], [278, 100, 278], [278, 100, 278], [0, 0, 0]], np.float32)
    d = np.array([[0, 0, 1], [0, 0, 1], [np.nan, 0, 0], [0, 0, 0], [1e-38, 1e-38, 1]], np.float32)
    lims = np.repeat(np.array([np.nan, -1.0, 0.0, 1e-3, 1e3, np.inf], np.float32), 5)
    oo, dd = np.tile(o, (6, 1)), np.tile(d, (6, 1))
    spec = ms.MultiHitSpec(oracle, *bunny, oo, dd)
    want = _check(ctx, spec, oo, dd, 4, max_dist=lims, what="nan/degenerate")
    c = want["count"].reshape(6, 5)
    assert not c[:3].any() and not c[:, 1:3].any() and c[5, 0] >= 1
    # no limit at all is the +inf row
    ms.assert_equal(_query(ctx, o, d, 4, "count"), {f: a[25:] for f, a in want.items()}, "NULL max_dist")


# ------------------------------------------------------------------ 4
@pytest.mark.parametrize("back", [1e3, 1e5, 1e7])
def test_far_origins(ctx, bunny, oracle, back):
    """4a. test_gpu_occlusion.test_far_origins' rays (aimed at triangle centroids from `back` units away,
    t ~ 1): the rounding of o + t d loses about ulp(back), which a bound D_k / |d| on t would ignore."""
    L, Q, S, T = bunny
    ctx.upload_scene(L, Q, S, T)
    rng = np.random.default_rng(1)
    n = 1000
    idx = rng.integers(0, len(T), n)
    c = (T["v0"][idx, :3] + (T["e1"][idx, :3] + T["e2"][idx, :3]) / 3.0).astype(np.float64)
    o0 = rng.uniform(5, 550, size=(n, 3))
    u = c - o0
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (c - back * u).astype(np.float32)
    d = (c - o.astype(np.float64)).astype(np.float32)
    spec = ms.MultiHitSpec(oracle, L, Q, S, T, o, d)
    want = _check(ctx, spec, o, d, 4, modes=("cull",), what=f"back {back:g}")
    assert np.count_nonzero(want["count"] >= 1) >= 950
    print(f"back {back:g}: counts {want['count'].min()}..{want['count'].max()}, "
          f"ties inside the list {np.count_nonzero(want['dist'][:, :3] == want['dist'][:, 1:])}")
    # the limit one float above and at the second distance, with the k-th distance's bound on top
    D2 = want["dist"][:, 1]
    for lim in (D2, np.nextafter(D2, INF)):
        _check(ctx, spec, o, d, 1, max_dist=lim, modes=("cull",), what=f"back {back:g} limited")
        _check(ctx, spec, o, d, 2, max_dist=lim, what=f"back {back:g} limited")


@pytest.mark.parametrize("scale", [2.0 ** -20, 2.0 ** 20])
def test_direction_scale(ctx, bunny, oracle, scale):
    """4b. Distances are Euclidean: d scaled by 2^-20 and 2^20.  (At 2^20 every hit within 1,048 units has
    t < 0.001 and is rejected, as in the closest-hit query: the box holds none, and the answer is that.)"""
    ctx.upload_scene(*bunny)
    o, d1 = ms.random_rays(1000, np.random.default_rng(0))
    d = (d1 * np.float32(scale)).astype(np.float32)
    spec = ms.MultiHitSpec(oracle, *bunny, o, d)
    want = _check(ctx, spec, o, d, 4, what=f"scale {scale:g}")
    _check(ctx, spec, o, d, 4, max_dist=150.0, what=f"scale {scale:g} limited")
    print(f"scale {scale:g}: rays with a hit {np.count_nonzero(want['count'])}, counts up to {want['count'].max()}")
    if scale < 1.0:
        assert np.count_nonzero(want["count"]) >= 100


# ------------------------------------------------------------------ 5
def test_relations_to_the_other_queries(ctx, bunny, bunny_box):
    """5. count > 0 is the occlusion query; the first entry is the closest-hit query's."""
    ctx.upload_scene(*bunny)
    o, d, spec = bunny_box
    for lim in (np.float32(np.inf), np.float32(150.0)):
        want = _check(ctx, spec, o, d, 2, max_dist=lim, what="bunny")
        assert np.array_equal(want["count"] > 0, ctx.occluded(o, d, lim))
    got = _query(ctx, o, d, 2, "cull")
    prim, dist = ctx.trace_rays(o, d)
    hit = (prim != NO_HIT) & ~np.isnan(dist)
    assert np.count_nonzero(hit) >= 3000
    assert np.array_equal(got["dist"][hit, 0].view(np.uint32), dist[hit].view(np.uint32))
    assert (got["prim"][~hit, 0] == NO_HIT).all()
    full = spec.answer(2)
    distinct = hit & (full["dist"][:, 0] != full["dist"][:, 1])
    assert np.count_nonzero(distinct) >= 0.9 * np.count_nonzero(hit)
    assert np.array_equal(got["prim"][distinct, 0], prim[distinct])


# ------------------------------------------------------------------ 6
def test_cornell_without_triangles(ctx, wgt, oracle):
    """6a. The plain Cornell box: quads and the dummy sphere only; tris-only answers with empty records."""
    L, Q, S = wgt.cornell_scene()
    ctx.upload_scene(L, Q, S)
    o, d = ms.random_rays(2000, np.random.default_rng(2))
    spec = ms.MultiHitSpec(oracle, L, Q, S, None, o, d)
    want = _check(ctx, spec, o, d, 4, what="cornell")
    assert want["count"].max() >= 2
    empty = _check(ctx, spec, o, d, 4, tris_only=True, what="cornell tris-only")
    assert not empty["count"].any() and (empty["prim"] == NO_HIT).all() and np.isinf(empty["dist"]).all()


def test_sphere_beside_the_mesh(ctx, bunny, oracle):
    """6b. A real sphere (radius 60) beside the mesh, as test_gpu_occlusion.test_sphere_occluder: rays at it
    from outside and from inside; the full query lists it, tris-only equals the specification's triangles."""
    L, Q, S, T = bunny
    S2 = np.concatenate([S, S])
    S2[1]["center"] = (420.0, 100.0, 150.0)
    S2[1]["radius"] = 60.0
    ctx.upload_scene(L, Q, S2, T)
    rng = np.random.default_rng(3)
    n = 500
    center = np.array([420.0, 100.0, 150.0])
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    target = center + v * rng.uniform(0, 59, size=(n, 1))
    o = np.concatenate([rng.uniform(5, 550, size=(n, 3)), center + v[::-1] * rng.uniform(0, 59, size=(n, 1))]).astype(np.float32)
    d = (np.concatenate([target, target]) - o).astype(np.float32)
    spec = ms.MultiHitSpec(oracle, L, Q, S2, T, o, d)
    sphere_id = len(L) + len(Q) + len(T) + 1
    full = _check(ctx, spec, o, d, 8, what="sphere")
    assert np.count_nonzero((full["prim"] == sphere_id).any(1)) >= 800
    tris = _check(ctx, spec, o, d, 8, tris_only=True, what="sphere tris-only")
    listed = tris["prim"][tris["prim"] != NO_HIT]
    assert listed.size >= 200 and (listed >= len(L) + len(Q)).all() and (listed < len(L) + len(Q) + len(T)).all()


# ------------------------------------------------------------------ 7
def test_after_update_and_rebuild(ctx, wgt, oracle, spheres):
    """7a. The answers follow the resident records: a refit (the spheres translated by (30, 0, -20)), then a
    rebuild to another triangle count (two of the three spheres; the sphere ids move)."""
    (L, Q, S, T), o, d, _ = spheres
    o, d = o[:2000], d[:2000]
    ctx.upload_scene(L, Q, S, T)
    moved = wgt.make_triangles(ms.concentric_verts(), translation=(30.0, 0.0, -20.0))
    ctx.update_triangles(moved)
    _check(ctx, ms.MultiHitSpec(oracle, L, Q, S, moved, o, d), o, d, 8, what="refit")
    two = wgt.make_triangles(ms.concentric_verts((150.0, 50.0)))
    assert len(two) == 336
    ctx.rebuild_triangles(two)
    want = _check(ctx, ms.MultiHitSpec(oracle, L, Q, S, two, o, d), o, d, 8, what="rebuild")
    assert want["count"].max() >= 6


def test_the_deepest_stack(ctx, oracle):
    """7b. geometric_up of tests/adversarial_meshes.py needs the builder's 31 stack entries: the lists behind
    the stack must not meet it, at the longest list too."""
    import adversarial_meshes as am

    T = am.small_mesh("geometric_up")
    L, Q, S = am.scene_parts("geometric_up")
    ctx.upload_scene(L, Q, S, T)
    assert ctx.scene_info()["bvh_stack"] == 31
    o, d = am.aimed_rays(T, 1000, 5)
    spec = ms.MultiHitSpec(oracle, L, Q, S, T, o, d)
    for k in (1, 8, 32):
        want = _check(ctx, spec, o, d, k, what="geometric_up")
    assert np.count_nonzero(want["count"]) >= 900


# ------------------------------------------------------------------ 8
def _device_rays(o, d, lim=None):
    import torch

    dev = torch.device("cuda", 0)
    soa = np.ascontiguousarray(np.concatenate([o.T, d.T], axis=0), np.float32)
    return torch.from_numpy(soa).to(dev), (None if lim is None else torch.from_numpy(np.ascontiguousarray(lim, np.float32)).to(dev))


def _device_run(ctx, form, d_rays, d_lim, n, k, mode, stream=0):
    """One device-pointer call; -> (the answer as the synchronous form returns it, what the call returned)."""
    import torch

    dev = d_rays.device
    count = torch.full((n,), 7, dtype=torch.int32, device=dev) if mode == "count" else None
    prim = torch.full((k, n), 7, dtype=torch.int32, device=dev)
    dist = torch.full((k, n), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    kw = dict(d_max_dist=d_lim.data_ptr() if d_lim is not None else 0, count=count.data_ptr() if count is not None else 0,
              prim=prim.data_ptr(), dist=dist.data_ptr())
    if form == "stats":
        ret = ctx.trace_multi_hits_stats(d_rays.data_ptr(), n, k, **kw)
    else:
        ret = ctx.trace_multi_hits_async(d_rays.data_ptr(), n, k, stream=stream, **kw)
        torch.cuda.synchronize()
    out = {"prim": np.ascontiguousarray(prim.cpu().numpy().view(np.uint32).T), "dist": np.ascontiguousarray(dist.cpu().numpy().T)}
    if count is not None:
        out["count"] = count.cpu().numpy().view(np.uint32)
    return out, ret


def test_stats_and_async_forms(ctx, spheres):
    """8. The device-pointer forms return the plain form's answers; the counters show that the k-th distance
    and the limit cull: k = 1 in cull mode visits fewer nodes than count mode, and so does a limit of 50."""
    import torch

    scene, o, d, spec = spheres
    ctx.upload_scene(*scene)
    n = len(o)
    d_rays, d_50 = _device_rays(o, d, np.full(n, 50.0, np.float32))
    stream = torch.cuda.Stream(device=d_rays.device)
    for k, mode in ((1, "cull"), (1, "count"), (8, "cull")):
        want = spec.answer(k)
        got, _ = _device_run(ctx, "async", d_rays, None, n, k, mode, stream=stream.cuda_stream)
        ms.assert_equal(got, want, f"async k={k} {mode}")
    got, cull1 = _device_run(ctx, "stats", d_rays, None, n, 1, "cull")
    ms.assert_equal(got, spec.answer(1), "stats k=1 cull")
    got, count_inf = _device_run(ctx, "stats", d_rays, None, n, 1, "count")
    ms.assert_equal(got, spec.answer(1), "stats k=1 count")
    got, count_50 = _device_run(ctx, "stats", d_rays, d_50, n, 1, "count")
    ms.assert_equal(got, spec.answer(1, max_dist=50.0), "stats k=1 count, limit 50")
    print(f"(node visits, triangle tests): cull k=1 {cull1}, count +inf {count_inf}, count 50 {count_50}")
    assert 0 < cull1[0] < count_inf[0] and 0 < count_50[0] < count_inf[0]
    assert cull1[1] <= count_inf[1] and count_50[1] < count_inf[1]


def test_refusals_on_a_context(ctx, spheres):
    """The entry points' own checks behind the scene check, in order; nothing is written."""
    from webgputracer_amd import _lib

    scene, o, d, _ = spheres
    ctx.upload_scene(*scene)
    L = _lib.lib()
    rays = np.ascontiguousarray(np.concatenate([o[:2].T, d[:2].T]), np.float32)
    prim = np.full(2 * 40, 123, np.uint32)
    count = np.full(2, 123, np.uint32)
    lists, only_count, none = (_lib.WgtMultiHitBuffers(prim=prim.ctypes.data), _lib.WgtMultiHitBuffers(count=count.ctypes.data),
                               _lib.WgtMultiHitBuffers())
    p = _lib.ptr
    assert L.wgt_trace_multi_hits(ctx.h, None, None, 0, 99, 99, None) == _lib.WGT_OK  # n == 0
    for args, text in (((None, None, 2, 99, 99, None), b"null rays"),
                       ((p(rays), None, 2, 99, 99, None), b"null output buffers"),
                       ((p(rays), None, 2, 99, 99, ctypes.byref(none)), b"no multi-hit field"),
                       ((p(rays), None, 2, 99, 2, ctypes.byref(lists)), b"unknown multi-hit flags"),
                       ((p(rays), None, 2, 0, 0, ctypes.byref(lists)), b"k out of range"),
                       ((p(rays), None, 2, 33, 1, ctypes.byref(lists)), b"k out of range")):
        assert L.wgt_trace_multi_hits(ctx.h, *args) == _lib.WGT_E_INVALID
        assert text in L.wgt_last_error(ctx.h), L.wgt_last_error(ctx.h)
        assert (prim == 123).all()
    assert L.wgt_trace_multi_hits_stats(ctx.h, p(rays), None, 2, 1, 0, ctypes.byref(lists), None) == _lib.WGT_E_INVALID
    assert b"null counts" in L.wgt_last_error(ctx.h)
    assert L.wgt_trace_multi_hits(ctx.h, p(rays), None, 2, 99, 1, ctypes.byref(only_count)) == _lib.WGT_OK  # k ignored
    assert (count != 123).all()
    with pytest.raises(ValueError):
        ctx.trace_multi_hits(o[:2], d[:2], 1, want=("pos",))


# ------------------------------------------------------------------ 9
def _cube(lo, hi):
    """12 triangles of the axis-aligned cube [lo, hi]^3 and its 18 edges (12 sides, 6 face diagonals)."""
    c = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.float64)
    faces = ((0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3))
    tris = [[c[f[0]], c[f[1]], c[f[2]]] for f in faces] + [[c[f[0]], c[f[2]], c[f[3]]] for f in faces]
    edges = {tuple(sorted(e)) for f in faces for e in ((f[0], f[1]), (f[1], f[2]), (f[2], f[3]), (f[3], f[0]), (f[0], f[2]))}
    return np.asarray(tris), np.asarray([[c[a], c[b]] for a, b in sorted(edges)])


def test_points_inside(ctx, wgt):
    """9. A cube of side 200 with a cube-shaped cavity of side 80: inside means in the shell, by the analytic
    test in float64.  Points are drawn at least 1 unit from every face and with rays at least 1e-3 from every
    edge's line (face diagonals included); a point that fails either is replaced by another draw."""
    lo, hi, clo, chi = 178.0, 378.0, 238.0, 318.0
    (t_out, e_out), (t_in, e_in) = _cube(lo, hi), _cube(clo, chi)
    T = wgt.make_triangles(np.concatenate([t_out, t_in]).astype(np.float32))
    assert len(T) == 24
    L, Q, S = wgt.cornell_scene()
    ctx.upload_scene(L, Q, S, T)
    directions = ((0.5377, 0.3183, 0.7807), (-0.3, 0.9, 0.1))  # the default, and another
    edges = np.concatenate([e_out, e_in])
    rng = np.random.default_rng(9)
    cand = rng.uniform(lo - 30.0, hi + 30.0, size=(6000, 3)).astype(np.float32)
    c64 = cand.astype(np.float64)
    ok = np.abs(c64[:, :, None] - np.array([lo, hi, clo, chi])).min(2).min(1) >= 1.0  # from every face's plane
    e = edges[:, 1] - edges[:, 0]
    for direction in directions:
        nrm = np.cross(np.asarray(direction, np.float64), e)  # (E, 3): neither direction is parallel to an edge
        assert (np.linalg.norm(nrm, axis=1) > 1.0).all()
        line_gap = np.abs(np.einsum("pej,ej->pe", edges[None, :, 0] - c64[:, None], nrm)) / np.linalg.norm(nrm, axis=1)
        ok &= line_gap.min(1) >= 1e-3
    pts = cand[ok][:2000]
    assert len(pts) == 2000
    p64 = pts.astype(np.float64)
    in_outer = ((p64 > lo) & (p64 < hi)).all(1)
    in_cavity = ((p64 > clo) & (p64 < chi)).all(1)
    want = in_outer & ~in_cavity
    assert want.sum() >= 500 and in_cavity.sum() >= 20 and (~in_outer).sum() >= 500
    got = ctx.points_inside(pts)
    assert got.dtype == np.bool_ and np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert np.array_equal(ctx.points_inside(pts, direction=directions[1]), want)  # parity, whatever the direction


# ------------------------------------------------------------------ 10
def test_hit_count_cli(ctx, wgt, tmp_path):
    """10. `frames --hit-count` at 32 x 32 writes NNN_hits.png = min(count, 255) of the query on the G-buffer's
    exported rays."""
    from PIL import Image

    from webgputracer_amd import frames

    obj = tmp_path / "mesh.obj"
    wgt.write_obj(str(obj), wgt.procedural_mesh("bunny", 2000))
    frames.main(["--frame", "2", "2", "--width", "32", "--height", "32", "--spp", "4", "--scene", f"obj:{obj}",
                 "--hit-count", "--out", str(tmp_path)])
    assert sorted(p.name for p in tmp_path.glob("*.png")) == ["001_hits.png"]
    img = np.asarray(Image.open(tmp_path / "001_hits.png").convert("RGBA"))
    ctx.upload_scene(*wgt.mesh_scene("bunny", obj_path=str(obj)))
    g = ctx.render_gbuffer(wgt.camera_param(1.0, 4, 1), 32, 32, want=("prim",), rays=True)
    count = ctx.trace_multi_hits(g["origin"].reshape(-1, 3), g["direction"].reshape(-1, 3), 0, want=("count",))["count"]
    assert img.shape == (32, 32, 4) and (img[..., 3] == 255).all()
    want = np.minimum(count, 255).astype(np.uint8).reshape(32, 32)
    for ch in range(3):
        assert np.array_equal(img[..., ch], want)
    assert len(np.unique(want)) >= 3 and np.array_equal(count > 0, g["prim"].ravel() != NO_HIT)
