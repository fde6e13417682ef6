"""The ray-query kernels and the renders against float64 geometry (tests/f64_truth.py), directly
and not through the oracle: the input sets of tests/test_truth_f64.py, the same decided rays,
the same bounds.  Every other GPU test demands the oracle's bits, so a rule that the oracle, the
restatements and the kernels all state wrongly passes them together; these do not.

The ray queries (k_trace_hits, k_occluded) read the 128-B nodes whatever WGT_CNODE says;
the node forms and both kernel families are covered by the renders at the end.  Each test
uploads its scene once and prints its share of decided rays and the largest error / E_t.
"""
import numpy as np
import pytest

import f64_truth as ft
from hit_records import NO_HIT

pytestmark = pytest.mark.gpu


def _queries_vs_truth(ctx, name, o, d, truth, cap):
    """trace_rays, trace_hits and occluded on the uploaded scene."""
    share = ft.check_share(name, truth, cap)
    prim, dist = ctx.trace_rays(o, d)
    worst = ft.check_closest(f"{name}: trace_rays", truth, prim, dist32=dist)
    rec = ctx.trace_hits(o, d)
    assert np.array_equal(rec["prim"], prim) and np.array_equal(rec["dist"].view(np.uint32), dist.view(np.uint32))
    pos_r, norm_ulp = ft.check_records(f"{name}: trace_hits", truth, rec)
    # occlusion: limits at 0.5 x and 2 x the float64 distance are answered exactly on decided rays
    # (a decided miss is not occluded at any limit); the two limits next to the hit are counted
    dec, hit = truth["decided"], (truth["prim"] >= 0) & (truth["nan_prim"] < 0)  # a NaN distance is below no limit
    d64 = np.where(hit, truth["dist"], 1e9)
    near = {}
    for f in (0.5, 0.999, 1.001, 2.0):
        occ = ctx.occluded(o, d, (f * d64).astype(np.float32))
        want = hit & (f > 1.0)
        if f in (0.5, 2.0):
            bad = np.flatnonzero(dec & (occ != want))
            assert bad.size == 0, (f"{name}: occluded at {f} x the float64 distance is wrong on {bad.size} decided rays; "
                                   f"first: ray {bad[0]} got {occ[bad[0]]} dist64 {truth['dist'][bad[0]]!r}")
        else:
            near[f] = int(np.sum(dec & (occ != want)))
    print(f"{name}: {len(o)} rays, decided {share:.3f}, max error / E_t {worst:.3f}, pos {pos_r:.3f}, norm {norm_ulp:.2f} ulp, "
          f"occluded off at 0.999 x / 1.001 x: {near[0.999]} / {near[1.001]}")


@pytest.mark.parametrize("size,offset,flat", ft.LATTICE_SCENES)
def test_lattice_queries_vs_float64(ctx, size, offset, flat):
    tris, _ = ft.lattice_tris(size, offset, flat)
    o, d, _ = ft.lattice_rays(size, offset, flat)
    L, S = ft.tri_scene(far_sphere=True)
    ctx.upload_scene(L, L[:0], S, tris)
    name = f"lattice size {size:g} near {offset:g} {'flat' if flat else 'general'}"
    _queries_vs_truth(ctx, name, o, d, ft.lattice_truth(size, offset, flat), ft.CAP_LATTICE)


@pytest.mark.parametrize("kind", ft.SOUP_KINDS)
@pytest.mark.parametrize("log2_scale,offset", ft.SOUP_CASES_GPU)
def test_scaled_soup_queries_vs_float64(ctx, log2_scale, offset, kind):
    """The uploadable soups of tests/test_truth_f64.py::test_scaled_soup_vs_float64 (up to
    coordinates of 2^39.6) through the three queries: exactly axis-parallel rays, d = target - o
    and unit directions."""
    tris, o, d, truth = ft.scaled_soup_set(log2_scale, offset, kind)
    L, S = ft.soup_scene(log2_scale, offset)
    ctx.upload_scene(L, L[:0], S, tris)
    _queries_vs_truth(ctx, f"soup 2^{log2_scale} offset {offset:g} {kind}", o, d, truth, ft.CAP_LATTICE)


def test_bunny_queries_vs_float64(ctx):
    tris, o, d, truth = ft.bunny_set()
    L, S = ft.tri_scene()
    ctx.upload_scene(L, L[:0], S, tris)
    _queries_vs_truth(ctx, "bunny-2000", o, d, truth, ft.CAP_MESH)


def test_sponza_queries_vs_float64(ctx):
    tris, o, d, truth = ft.sponza_set()
    L, S = ft.tri_scene()
    ctx.upload_scene(L, L[:0], S, tris)
    _queries_vs_truth(ctx, "sponza-20000", o, d, truth, ft.CAP_MESH)


def test_cornell_and_sphere_queries_vs_float64(ctx):
    L, Q, S, o, d, truth = ft.cornell_set()
    ctx.upload_scene(L, Q, S)
    _queries_vs_truth(ctx, "cornell", o, d, truth, ft.CAP_MESH)


def test_gbuffer_primary_rays_vs_float64(ctx, wgt):
    """One G-buffer of bunny-2000 in the Cornell walls at 48x27: each pixel's returned primary
    ray, traced in float64, gives the returned primitive, distance and record on decided rays."""
    L, Q, S, T = wgt.mesh_scene("bunny", target_tris=2000)
    ctx.upload_scene(L, Q, S, T)
    g = ctx.render_gbuffer(wgt.camera_param(16 / 9, 1, 3), 48, 27, rays=True)
    o, d = g["origin"].reshape(-1, 3), g["direction"].reshape(-1, 3)
    truth = ft.scan(o, d, L, Q, S, T)
    share = ft.check_share("gbuffer", truth, ft.CAP_MESH)
    rec = {k: g[k].reshape((-1,) + g[k].shape[2:]) for k in ("prim", "dist", "pos", "norm", "flags")}
    worst = ft.check_closest("gbuffer", truth, rec["prim"], dist32=rec["dist"])
    pos_r, norm_ulp = ft.check_records("gbuffer", truth, rec)
    nlq = len(L) + len(Q)
    on_mesh = np.mean((truth["prim"] >= nlq) & (truth["prim"] < nlq + len(T)) & truth["decided"])
    assert on_mesh > 0.05  # the frame does look at the mesh
    print(f"gbuffer: decided {share:.3f}, on the mesh {on_mesh:.3f}, max error / E_t {worst:.3f}, pos {pos_r:.3f}, "
          f"norm {norm_ulp:.2f} ulp")


@pytest.mark.parametrize("env", [{}, {"WGT_CNODE": "0"}, {"WGT_KERNEL": "1"}], ids=["ps-compact", "ps-128B", "simple"])
def test_flat_box_renders_solid(ctx, wgt, env, monkeypatch):
    """The user-visible form of the dropped hits: an axis-aligned box [0, 3]^3 of 192 flat
    triangles near the origin, seen from 100 away across three of its faces.  Every centre
    pixel's hit id names a triangle of the box, not the wall far behind it or nothing, through
    k_render_ps on both node forms and through the simple kernel.  (Under the rule that
    demanded t inside the triangle's own slab interval 16 of these 196 pixels saw through.)"""
    for k in ("WGT_CNODE", "WGT_KERNEL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L, Q, S = wgt.cornell_scene()
    T = ft.flat_box_mesh()
    ctx.upload_scene(L, Q[4:5], S, T)  # the back wall (z = 555) alone: the camera stands outside the Cornell box
    cam = wgt.camera_param(1.0, 4, 11, fovy=4.0)
    cam["origin"] = (1.5 - 40.0, 1.5 + 50.0, 1.5 - 80.0)
    cam["target"] = (1.5, 1.5, 1.5)
    W = 48
    # a cube's silhouette holds the disc of radius side / 2 about its centre: 1.5 / (102.5 tan(2 deg)) of the
    # half frame, 10 pixels; the centre 14 x 14 pixels (half diagonal 9.9) lie inside it
    g = ctx.render_tile(cam, W, W, want=("hit",))
    centre = g["hit"][W // 2 - 7:W // 2 + 7, W // 2 - 7:W // 2 + 7]
    nlq = len(L) + 1
    on_box = (centre >= nlq) & (centre < nlq + len(T))
    assert on_box.all(), f"{int((~on_box).sum())} of {on_box.size} centre pixels see through the box: {centre[~on_box][:8]}"
    assert np.any(g["hit"] == NO_HIT)  # and the frame is wider than the box
