"""CPU expectations of whole hit records (wgt_trace_hits, wgt_render_gbuffer), shared by
tests/test_gpu_hits.py and tests/test_gpu_gbuffer.py.  TEST INFRASTRUCTURE ONLY.

Three sources, as the tests' docstrings say: the C oracle's closest hit (prim, dist) on any
scene; numpy_restatement.sample_hit for every field of quad and sphere hits; and, for a
triangle hit, the restatement below of the oracle's intersect_tris (oracle/wgt_oracle.c) from
OracleScene.trace_tris' (tid, t), written with numpy_restatement's float32 vector helpers.
"""
import numpy as np

import numpy_restatement as nr
from numpy_restatement import add, dot, length, neg, scl, sel, sub

NO_HIT = np.uint32(0xFFFFFFFF)
EMISSIVE, FRONT_FACE = 1, 2  # WGT_HIT_EMISSIVE, WGT_HIT_FRONT_FACE
VEC = ("pos", "norm", "col")
FIELDS = ("prim", "dist", "pos", "norm", "col", "flags")


def random_rays(n, rng):
    # as tests/test_gpu_occlusion.py (and tests/test_gpu_parity.py) draw them
    o = rng.uniform(5, 550, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


def _cols(a):
    return tuple(np.ascontiguousarray(a[:, k], np.float32) for k in range(3))


def _rows(v):
    return np.stack(v, axis=1).astype(np.float32)


def miss_record(n):
    """hit_init's state: prim = 0xffffffff, dist = kRayMax, zero vectors, flags = 0."""
    z = np.zeros((n, 3), np.float32)
    return {"prim": np.full(n, NO_HIT, np.uint32), "dist": np.full(n, nr.kRayMax, np.float32), "pos": z.copy(),
            "norm": z.copy(), "col": z.copy(), "flags": np.zeros(n, np.uint8)}


def quad_sphere_records(o, d, lights, quads, spheres):
    """numpy_restatement.sample_hit on the lights, quads and spheres, as records."""
    with np.errstate(all="ignore"):
        h = nr.sample_hit(_cols(o), _cols(d), lights, quads, spheres)
    flags = (h["emissive"].astype(np.uint8) * EMISSIVE) | (h["ff"].astype(np.uint8) * FRONT_FACE)
    return {"prim": h["prim"].astype(np.uint32), "dist": h["dist"].astype(np.float32), "pos": _rows(h["pos"]),
            "norm": _rows(h["norm"]), "col": _rows(h["col"]), "flags": flags.astype(np.uint8)}


def triangle_records(o, d, tris, tid, t, nlq):
    """The oracle's intersect_tris for rays whose closest triangle is (tid, t): pos = o + t d,
    ff = dot(d, fn) < 0, norm = ff ? fn : -fn, col and emissive from the record."""
    with np.errstate(all="ignore"):
        ov, dv = _cols(o), _cols(d)
        pos = add(ov, scl(t.astype(np.float32), dv))
        dist = length(sub(pos, ov))
        fn = _cols(tris["face_norm"][tid][:, :3])
        ff = dot(dv, fn) < 0
        norm = sel(ff, fn, neg(fn))
    flags = ((tris["emissive"][tid] > 0).astype(np.uint8) * EMISSIVE) | (ff.astype(np.uint8) * FRONT_FACE)
    return {"prim": (np.uint32(nlq) + tid).astype(np.uint32), "dist": dist.astype(np.float32), "pos": _rows(pos),
            "norm": _rows(norm), "col": np.ascontiguousarray(tris["col"][tid], np.float32), "flags": flags.astype(np.uint8)}


def expected_records(osc, lights, quads, spheres, tris, o, d):
    """Every field of the closest hit of rays (o, d) on the scene, and the mask of triangle hits.
    A ray whose closest hit (the oracle's) is a triangle takes the triangle restatement; any
    other ray's closest hit is a quad, a sphere or nothing, which the quad-and-sphere scan
    alone finds.  The assembled (prim, dist) must equal the oracle's, bit for bit."""
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    want = quad_sphere_records(o, d, lights, quads, spheres)
    nlq, nt = len(lights) + len(quads), 0 if tris is None else len(tris)
    is_tri = np.zeros(len(o), bool)
    prim, dist = osc.trace(o, d)
    if nt:
        # sphere ids follow the triangles'
        want["prim"] = np.where((want["prim"] != NO_HIT) & (want["prim"] >= nlq), want["prim"] + np.uint32(nt),
                                want["prim"]).astype(np.uint32)
        is_tri = (prim >= nlq) & (prim < nlq + nt)
        k = np.flatnonzero(is_tri)
        tid, t = osc.trace_tris(o[k], d[k])
        assert np.array_equal(tid, prim[k] - np.uint32(nlq))
        rec = triangle_records(o[k], d[k], tris, tid, t, nlq)
        for f in FIELDS:
            want[f][k] = rec[f]
    nan_ray = np.isnan(o).any(axis=1) | np.isnan(d).any(axis=1)
    assert np.array_equal(want["prim"], prim)
    assert np.array_equal(want["dist"][~nan_ray].view(np.uint32), dist[~nan_ray].view(np.uint32))
    return want, is_tri


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_records_equal(got, want, o=None, d=None, fields=FIELDS, what=""):
    """Bit equality of every field (floats as uint32).  The one exception: a record whose ray
    (o, d) has a NaN component compares its floats with NaN equal to NaN, because the payload
    bits of a NaN are not specified; its prim and flags are still compared exactly."""
    n = len(want["prim"])
    nan_ray = np.zeros(n, bool)
    if o is not None:
        nan_ray = np.isnan(np.asarray(o).reshape(n, 3)).any(axis=1) | np.isnan(np.asarray(d).reshape(n, 3)).any(axis=1)
    for f in fields:
        g, w = np.asarray(got[f]).reshape((n,) + ((3,) if f in VEC else ())), want[f]
        assert g.shape == w.shape and g.dtype == w.dtype, (what, f, g.shape, w.shape, g.dtype, w.dtype)
        if f in ("prim", "flags"):
            same = g == w
        else:
            same = bits(g) == bits(w)
            loose = np.isnan(g) & np.isnan(w)
            same = same | (loose & (nan_ray[:, None] if f in VEC else nan_ray))
        bad = np.flatnonzero(~(same.all(axis=1) if same.ndim == 2 else same))
        assert bad.size == 0, (f"{what}: field {f}: {bad.size} of {n} records differ; first: record {bad[0]} "
                               f"got {g[bad[0]]!r} want {w[bad[0]]!r} (prim got {np.asarray(got['prim']).ravel()[bad[0]] if 'prim' in got else '-'}"
                               f" want {want['prim'][bad[0]]})")
