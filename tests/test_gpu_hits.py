"""Whole hit records of caller rays, wgt_trace_hits, against their definition: record i is the
reference's HitInfo after sample_hit on ray i (prim, dist, pos, norm, col, emissive and
front-face flags).

Expected values (tests/hit_records.py): the C oracle's closest hit for (prim, dist),
numpy_restatement.sample_hit for every field of quad and sphere hits, and a restatement of the
oracle's intersect_tris for triangle hits.  Every comparison is bit equality (floats as
uint32); the one exception is a record whose ray has a NaN component, whose floats compare
with NaN equal to NaN (hit_records.assert_records_equal).
"""
import ctypes

import numpy as np
import pytest

import hit_records as hr

pytestmark = pytest.mark.gpu

NO_HIT = hr.NO_HIT


@pytest.fixture(scope="module")
def small_bunny(wgt, oracle):
    """The Cornell walls and a 2,000-triangle bunny stand-in, with its oracle scene."""
    L, Q, S, T = wgt.mesh_scene("bunny", 2000)
    return (L, Q, S, T), oracle.OracleScene(L, Q, S, T)


@pytest.fixture(scope="module")
def box_rays():
    """The 20,000 rays of test_gpu_occlusion._random_rays(20_000, default_rng(0))."""
    return hr.random_rays(20_000, np.random.default_rng(0))


@pytest.fixture(scope="module")
def bunny_expected(small_bunny, box_rays):
    """Every field of those rays' closest hits on the mesh scene, computed once."""
    (L, Q, S, T), osc = small_bunny
    return hr.expected_records(osc, L, Q, S, T, *box_rays)


def _sphere_scene(wgt, emissive):
    """Cornell plus a sphere at (190, 90, 190) with radius 90, after the dummy."""
    L, Q, S = wgt.cornell_scene()
    S2 = np.concatenate([S, S])
    S2[1]["center"] = (190.0, 90.0, 190.0)
    S2[1]["radius"] = 90.0
    S2[1]["col"] = (0.2, 0.5, 0.9)
    S2[1]["emissive"] = 1.0 if emissive else 0.0
    return L, Q, S2


def test_mesh_scene_every_field(ctx, small_bunny, box_rays, bunny_expected):
    """1. 20,000 random rays in the box with the 2,000-triangle bunny: triangle hits (front and
    back faces), quad hits and misses, every field; prim and dist also equal trace_rays."""
    (L, Q, S, T), _ = small_bunny
    ctx.upload_scene(L, Q, S, T)
    o, d = box_rays
    want, is_tri = bunny_expected
    back = is_tri & ((want["flags"] & hr.FRONT_FACE) == 0)
    miss = want["prim"] == NO_HIT
    print(f"triangle hits {is_tri.sum()}, back-facing {back.sum()}, misses {miss.sum()}")
    assert is_tri.sum() >= 2000 and back.sum() >= 500 and miss.sum() >= 2000
    got = ctx.trace_hits(o, d)
    assert set(got) == set(hr.FIELDS)
    hr.assert_records_equal(got, want, what="bunny")
    init = hr.miss_record(int(miss.sum()))
    for f in hr.FIELDS:  # a miss is hit_init's record
        assert np.array_equal(got[f][miss].view(np.uint8), init[f].view(np.uint8)), f
    prim, dist = ctx.trace_rays(o, d)
    assert np.array_equal(got["prim"], prim) and np.array_equal(hr.bits(got["dist"]), hr.bits(dist))


def test_quad_back_faces_from_outside_the_box(ctx, small_bunny):
    """2. Rays from outside the box towards points inside: the walls are hit from behind."""
    (L, Q, S, T), osc = small_bunny
    ctx.upload_scene(L, Q, S, T)
    rng = np.random.default_rng(7)
    p = rng.uniform(5, 550, size=(4000, 3))
    q = rng.uniform(5, 550, size=(4000, 3))
    c = np.array([278.0, 278.0, 278.0])
    o64 = c + 3.0 * (p - c)
    d64 = q - o64
    d64 /= np.linalg.norm(d64, axis=1, keepdims=True)
    o, d = o64.astype(np.float32), d64.astype(np.float32)
    want, _ = hr.expected_records(osc, L, Q, S, T, o, d)
    nlq = len(L) + len(Q)
    back_quads = (want["prim"] < nlq) & ((want["flags"] & hr.FRONT_FACE) == 0)
    print(f"back-facing quad hits {back_quads.sum()}")
    assert back_quads.sum() >= 2500
    hr.assert_records_equal(ctx.trace_hits(o, d), want, what="outside")


@pytest.mark.parametrize("emissive", [False, True])
def test_spheres(ctx, wgt, oracle, box_rays, emissive):
    """3. A real sphere in the Cornell box, hit from outside (front) and from inside (back);
    emissive too, for the flag."""
    L, Q, S2 = _sphere_scene(wgt, emissive)
    ctx.upload_scene(L, Q, S2)
    o, d = box_rays
    want = hr.quad_sphere_records(o, d, L, Q, S2)
    prim, dist = oracle.OracleScene(L, Q, S2).trace(o, d)
    assert np.array_equal(want["prim"], prim) and np.array_equal(hr.bits(want["dist"]), hr.bits(dist))
    sph = want["prim"] == len(L) + len(Q) + 1
    front = sph & ((want["flags"] & hr.FRONT_FACE) != 0)
    print(f"sphere hits {sph.sum()}, front {front.sum()}, back {(sph & ~front).sum()}")
    assert sph.sum() >= 400 and front.sum() >= 150 and (sph & ~front).sum() >= 150
    assert np.all(((want["flags"][sph] & hr.EMISSIVE) != 0) == emissive)
    hr.assert_records_equal(ctx.trace_hits(o, d), want, what=f"sphere emissive={emissive}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_shapes_and_optional_fields(ctx, wgt, small_bunny, box_rays, bunny_expected, n):
    """4. Ragged launches, each field alone and prim with dist only; through the async form the
    buffers of the fields not asked for keep a sentinel; no field at all is an error."""
    import torch

    from webgputracer_amd import _lib

    (L, Q, S, T), _ = small_bunny
    ctx.upload_scene(L, Q, S, T)
    o, d = box_rays[0][:n], box_rays[1][:n]
    want = {k: v[:n] for k, v in bunny_expected[0].items()}
    for fields in [(f,) for f in hr.FIELDS] + [("prim", "dist")]:
        got = ctx.trace_hits(o, d, want=fields)
        assert set(got) == set(fields)
        for f in fields:
            assert got[f].shape == ((n, 3) if f in hr.VEC else (n,))
        hr.assert_records_equal(got, want, fields=fields, what=f"n={n} {fields}")
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([o.T, d.T], axis=0), np.float32)).to(dev)
    dt = {"prim": torch.int32, "flags": torch.uint8}
    for fields in [(f,) for f in hr.FIELDS] + [("prim", "dist"), hr.FIELDS]:
        buf = {f: torch.full(((3, n) if f in hr.VEC else (n,)), 0x5A, dtype=dt.get(f, torch.float32), device=dev)
               for f in hr.FIELDS}
        torch.cuda.synchronize()
        ctx.trace_hits_async(d_rays.data_ptr(), n, **{f: buf[f].data_ptr() for f in fields})
        ctx.sync()
        host = {f: b.cpu().numpy() for f, b in buf.items()}
        got = {f: (host[f].T if f in hr.VEC else host[f]) for f in fields}
        if "prim" in got:
            got["prim"] = got["prim"].view(np.uint32)
        hr.assert_records_equal(got, want, fields=fields, what=f"async n={n} {fields}")
        for f in set(hr.FIELDS) - set(fields):
            assert np.all(host[f] == 0x5A), (fields, f)  # not asked for: untouched
    none = _lib.WgtHitBuffers()
    soa = np.ascontiguousarray(np.concatenate([o.T, d.T], axis=0), np.float32)
    L_ = _lib.lib()
    assert L_.wgt_trace_hits(ctx.h, _lib.ptr(soa), n, ctypes.byref(none)) == _lib.WGT_E_INVALID
    assert L_.wgt_trace_hits_async(ctx.h, ctypes.c_void_p(d_rays.data_ptr()), n, ctypes.byref(none), None) == _lib.WGT_E_INVALID
    assert L_.wgt_trace_hits(ctx.h, _lib.ptr(soa), n, None) == _lib.WGT_E_INVALID
    assert L_.wgt_trace_hits(ctx.h, _lib.ptr(soa), 0, ctypes.byref(none)) == _lib.WGT_OK  # n == 0: nothing to do


def test_degenerate_rays(ctx, wgt, oracle):
    """5. A NaN origin component, a NaN direction, a zero direction and an infinite origin on
    the sphere scene of test 3, after a plain ray.  A NaN ray's hit is the last sphere with NaN
    fields (nan_hit)."""
    L, Q, S2 = _sphere_scene(wgt, False)
    ctx.upload_scene(L, Q, S2)
    o = np.array([[278, 278, -800], [np.nan, 1, 1], [278, 100, 278], [278, 100, 278], [np.inf, 100, 278]], np.float32)
    d = np.array([[0, 0, 1], [0, 0, 1], [np.nan, 0, 0], [0, 0, 0], [0, 0, 1]], np.float32)
    want = hr.quad_sphere_records(o, d, L, Q, S2)
    got = ctx.trace_hits(o, d)
    for f in hr.FIELDS:
        print(f, "got", got[f].tolist(), "bits", (hr.bits(got[f]) if got[f].dtype == np.float32 else got[f]).tolist())
        print(f, "want", want[f].tolist(), "bits", (hr.bits(want[f]) if want[f].dtype == np.float32 else want[f]).tolist())
    last = len(L) + len(Q) + len(S2) - 1
    assert want["prim"][1] == last and want["prim"][2] == last and np.isnan(want["dist"][1:3]).all()
    hr.assert_records_equal(got, want, o, d, what="degenerate")
    prim, dist = ctx.trace_rays(o, d)
    assert np.array_equal(got["prim"], prim) and np.array_equal(hr.bits(got["dist"]), hr.bits(dist))


def test_scene_without_triangles(ctx, wgt, oracle, box_rays):
    """6. The plain Cornell box (the TRIS = false instantiation)."""
    L, Q, S = wgt.cornell_scene()
    ctx.upload_scene(L, Q, S)
    o, d = box_rays
    want, is_tri = hr.expected_records(oracle.OracleScene(L, Q, S), L, Q, S, None, o, d)
    assert not is_tri.any() and (want["prim"] != NO_HIT).sum() >= 10_000
    got = ctx.trace_hits(o, d)
    hr.assert_records_equal(got, want, what="cornell")
    prim, dist = ctx.trace_rays(o, d)
    assert np.array_equal(got["prim"], prim) and np.array_equal(hr.bits(got["dist"]), hr.bits(dist))
