"""Occlusion (any-hit) queries, wgt_occluded_rays, against their definition:

    occluded[i] = (prim != 0xffffffff) & (dist < max_dist[i])      (IEEE float32)

with (prim, dist) the CPU oracle's closest hit of ray i.  The definition is exact, so every
comparison here is equality: no tolerance, no excluded rays.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NO_HIT = np.uint32(0xFFFFFFFF)
INF = np.float32(np.inf)


def _random_rays(n, rng):
    # as tests/test_gpu_parity.py draws them
    o = rng.uniform(5, 550, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def _expected(prim, dist, max_dist):
    with np.errstate(invalid="ignore"):
        return (prim != NO_HIT) & (dist.astype(np.float32) < np.asarray(max_dist, np.float32))


def _five_limits(D):
    """0.5 D, D, the float above D, 2 D, +inf per ray (D: the closest distance)."""
    D = D.astype(np.float32)
    return [np.float32(0.5) * D, D, np.nextafter(D, INF), np.float32(2.0) * D, np.full_like(D, INF)]


def _check_limits(ctx, o, d, prim, dist, limits):
    """One query over the rays repeated once per limit array; -> the expected values."""
    k = len(limits)
    oo, dd, lim = np.tile(o, (k, 1)), np.tile(d, (k, 1)), np.concatenate(limits).astype(np.float32)
    want = _expected(np.tile(prim, k), np.tile(dist, k), lim)
    got = ctx.occluded(oo, dd, lim)
    assert got.dtype == np.bool_ and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{bad.size} of {want.size} differ; first: ray {bad[0] % len(o)} limit set {bad[0] // len(o)} "
                           f"o={oo[bad[0]]} d={dd[bad[0]]} max_dist={lim[bad[0]]!r} dist={np.tile(dist, k)[bad[0]]!r} "
                           f"got {got[bad[0]]}")
    return want


@pytest.fixture(scope="module")
def small_bunny(wgt, oracle):
    """The Cornell walls and a 2,000-triangle bunny stand-in, with its oracle scene."""
    L, Q, S, T = wgt.mesh_scene("bunny", 2000)
    return (L, Q, S, T), oracle.OracleScene(L, Q, S, T)


@pytest.fixture(scope="module")
def box_rays(small_bunny):
    """The 20,000 random rays of tests 1 and 3 with the oracle's closest hits, computed once."""
    _, osc = small_bunny
    o, d = _random_rays(20_000, np.random.default_rng(0))
    prim, dist = osc.trace(o, d)
    return o, d, prim, dist


def test_limits_around_the_closest_distance(ctx, small_bunny, box_rays):
    """1. Each ray with max_dist = 0.5 D, D, nextafter(D), 2 D and +inf: a hit gives 0, 0, 1, 1, 1."""
    (L, Q, S, T), _ = small_bunny
    ctx.upload_scene(L, Q, S, T)
    o, d, prim, dist = box_rays
    want = _check_limits(ctx, o, d, prim, dist, _five_limits(dist))
    assert want.mean() >= 0.25 and (~want).mean() >= 0.25
    nlq = len(L) + len(Q)
    assert np.count_nonzero((prim >= nlq) & (prim < nlq + len(T))) >= 2000  # the closest hits that are triangles


@pytest.mark.parametrize("back", [1e3, 1e5, 1e7])
def test_far_origins(ctx, small_bunny, back):
    """2. Rays aimed at triangle centroids from about `back` units away, d = the unnormalised
    difference (t ~ 1), max_dist one float below, at and above the closest distance: the rounding
    of o + t d loses about ulp(back), which a bound max_dist / |d| on t ignores."""
    (L, Q, S, T), osc = small_bunny
    ctx.upload_scene(L, Q, S, T)
    rng = np.random.default_rng(1)
    idx = rng.integers(0, len(T), 3000)
    c = (T["v0"][idx, :3] + (T["e1"][idx, :3] + T["e2"][idx, :3]) / 3.0).astype(np.float64)
    o0 = rng.uniform(5, 550, size=(3000, 3))
    u = c - o0
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = (c - back * u).astype(np.float32)
    d = (c - o.astype(np.float64)).astype(np.float32)
    prim, D = osc.trace(o, d)
    assert np.count_nonzero(prim != NO_HIT) >= 2900
    _check_limits(ctx, o, d, prim, D, [np.nextafter(D, -INF), D, np.nextafter(D, INF)])


@pytest.mark.parametrize("scale", [2.0 ** -20, 1.0, 2.0 ** 20])
def test_direction_scale(ctx, small_bunny, box_rays, scale):
    """3. The limit is Euclidean: d scaled by 2^-20, 1, 2^20, with D (and so max_dist) from the
    oracle on the scaled rays."""
    (L, Q, S, T), osc = small_bunny
    ctx.upload_scene(L, Q, S, T)
    o, d1, prim1, dist1 = box_rays
    d = (d1 * np.float32(scale)).astype(np.float32)
    prim, dist = (prim1, dist1) if scale == 1.0 else osc.trace(o, d)
    # (at 2^-20 the walls drop out: |dot(normal, d)| < 0.001 rejects a quad, so most rays hit
    # nothing or a triangle; the shares of test 1 are not asserted here)
    _check_limits(ctx, o, d, prim, dist, _five_limits(dist))


def test_nan_and_degenerate(ctx, small_bunny):
    """4. The five rays of test_trace_rays_nan_and_degenerate x max_dist in {NaN, -1, 0, 1e-3, 1e3, +inf}."""
    (L, Q, S, T), osc = small_bunny
    ctx.upload_scene(L, Q, S, T)
    o = np.array([[278, 278, -800], [np.nan, 1, 1], [278, 100, 278], [278, 100, 278], [0, 0, 0]], np.float32)
    d = np.array([[0, 0, 1], [0, 0, 1], [np.nan, 0, 0], [0, 0, 0], [1e-38, 1e-38, 1]], np.float32)
    prim, dist = osc.trace(o, d)
    assert np.isnan(dist[1]) and np.isnan(dist[2])  # a NaN ray's hit has a NaN distance: never occluded
    lims = [np.full(5, v, np.float32) for v in (np.nan, -1.0, 0.0, 1e-3, 1e3, np.inf)]
    want = _check_limits(ctx, o, d, prim, dist, lims)
    assert not want[:15].any() and not want.reshape(6, 5)[:, 1:3].any()
    assert want.reshape(6, 5)[5, 0]  # the plain ray is occluded under +inf


def test_cornell_without_triangles(ctx, wgt, oracle):
    """5a. The plain Cornell box: quads and the dummy sphere only (the TRIS = false kernel)."""
    L, Q, S = wgt.cornell_scene()
    ctx.upload_scene(L, Q, S)
    o, d = _random_rays(5000, np.random.default_rng(2))
    prim, dist = oracle.OracleScene(L, Q, S).trace(o, d)
    want = _check_limits(ctx, o, d, prim, dist, _five_limits(dist))
    assert want.mean() >= 0.25 and (~want).mean() >= 0.25


def test_sphere_occluder(ctx, small_bunny, oracle):
    """5b. A real sphere (radius 60) beside the mesh: rays aimed at it from outside (the near
    root) and from inside it (the far root), where it is often the only occluder in range."""
    (L, Q, S, T), _ = small_bunny
    S2 = np.concatenate([S, S])
    S2[1]["center"] = (420.0, 100.0, 150.0)
    S2[1]["radius"] = 60.0
    ctx.upload_scene(L, Q, S2, T)
    osc = oracle.OracleScene(L, Q, S2, T)
    rng = np.random.default_rng(3)
    n = 3000
    center = np.array([420.0, 100.0, 150.0])
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    target = center + v * rng.uniform(0, 59, size=(n, 1))
    o_out = rng.uniform(5, 550, size=(n, 3))
    o_in = center + v[::-1] * rng.uniform(0, 59, size=(n, 1))
    o = np.concatenate([o_out, o_in]).astype(np.float32)
    d = (np.concatenate([target, target]) - o).astype(np.float32)
    prim, dist = osc.trace(o, d)
    sphere_id = len(L) + len(Q) + len(T) + 1
    assert np.count_nonzero(prim[:n] == sphere_id) >= 1000 and np.count_nonzero(prim[n:] == sphere_id) >= 2000
    _check_limits(ctx, o, d, prim, dist, _five_limits(dist))


def test_refill_and_grid_edges(ctx, small_bunny):
    """6. Grid edges: n = 1, 63, 64, 65 and 3 x 64 x ps_resident + 17 rays (a ragged last wave, and
    several times more waves than the device holds at once, so wave slots are reused within the
    launch), max_dist uniform in [0, 600], against trace_rays on the same rays (itself pinned to
    the oracle)."""
    (L, Q, S, T), _ = small_bunny
    ctx.upload_scene(L, Q, S, T)
    R = ctx.scene_info()["ps_resident"]
    assert R > 0
    big = 64 * R * 3 + 17
    rng = np.random.default_rng(4)
    o, d = _random_rays(big, rng)
    lim = rng.uniform(0, 600, size=big).astype(np.float32)
    for n in (1, 63, 64, 65, big):
        prim, dist = ctx.trace_rays(o[:n], d[:n])
        want = _expected(prim, dist, lim[:n])
        got = ctx.occluded(o[:n], d[:n], lim[:n])
        assert np.array_equal(got, want), (n, int(np.count_nonzero(got != want)))
    assert 0.2 < want.mean() < 0.8


def test_async_on_a_torch_stream(ctx, small_bunny):
    """7. Two consecutive device-pointer calls on a non-default stream, different limits into
    different outputs: both equal the synchronous results."""
    import torch

    (L, Q, S, T), _ = small_bunny
    ctx.upload_scene(L, Q, S, T)
    n = 50_000
    o, d = _random_rays(n, np.random.default_rng(5))
    lim_a = np.full(n, 150.0, np.float32)
    lim_b = np.random.default_rng(6).uniform(0, 600, size=n).astype(np.float32)
    want_a, want_b = ctx.occluded(o, d, lim_a), ctx.occluded(o, d, lim_b)
    dev = torch.device("cuda", 0)
    soa = np.ascontiguousarray(np.concatenate([o.T, d.T], axis=0), np.float32)
    d_rays = torch.from_numpy(soa).to(dev)
    d_a, d_b = torch.from_numpy(lim_a).to(dev), torch.from_numpy(lim_b).to(dev)
    out_a = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    out_b = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=dev)
    ctx.occluded_async(d_rays.data_ptr(), d_a.data_ptr(), n, out_a.data_ptr(), stream=stream.cuda_stream)
    ctx.occluded_async(d_rays.data_ptr(), d_b.data_ptr(), n, out_b.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(out_a.cpu().numpy(), want_a.astype(np.uint8))
    assert np.array_equal(out_b.cpu().numpy(), want_b.astype(np.uint8))
    assert want_a.any() and not want_a.all() and np.any(want_a != want_b)


def test_existing_kernels_unchanged_after_an_occlusion_call(ctx, wgt, oracle, small_bunny):
    """8. The context's shared state survives an occlusion call: a Cornell render and a
    closest-hit query on the same context still equal the oracle."""
    (L, Q, S, T), osc = small_bunny
    ctx.upload_scene(L, Q, S, T)
    o, d = _random_rays(100_000, np.random.default_rng(7))
    assert ctx.occluded(o, d, 200.0).any()  # a scalar limit broadcasts
    gp, gd = ctx.trace_rays(o[:20_000], d[:20_000])
    rp, rd = osc.trace(o[:20_000], d[:20_000])
    assert np.array_equal(gp, rp) and np.array_equal(gd.view(np.uint32), rd.view(np.uint32))
    Lc, Qc, Sc = wgt.cornell_scene()
    ctx.upload_scene(Lc, Qc, Sc)
    osc_c = oracle.OracleScene(Lc, Qc, Sc)
    cp, cd = osc_c.trace(o[:1000], d[:1000])
    assert np.array_equal(ctx.occluded(o[:1000], d[:1000], np.inf), _expected(cp, cd, INF))
    g = ctx.render_tile(wgt.camera_param(1.0, 4, 7), 32, 32)
    r = osc_c.render(oracle.camera_param(1.0, 4, 7), 32, 32)
    assert np.array_equal(g["f32"].view(np.uint32), r["f32"].view(np.uint32))
    assert np.array_equal(g["hit"], r["hit"])
