"""Bit parity of the ray queries (wgt_trace_rays, wgt_trace_hits, wgt_occluded_rays) with the
oracle over the caller-ray domain: scaled scenes, far origins, huge and tiny directions.

Caller rays are not validated, and the query kernels carry guards written for rays outside the
render limits: quad_scan_fast<true>'s `qt D < 2^62` (2^64 until this file) and `prev D >= 2^-49`, occ_t_hi's covered
box (l1, m <= 2^40, 2^-40 <= nd <= 2^40), sqrt_rn's small-operand branch, the IEEE (EXACT)
divisions, k_occluded's NaN fallbacks.  The other query tests stay at Cornell scale with direction
scales within 2^+-20 and origins within 1e7, where none of these guards is crossed.

The oracle is the definition, so every comparison is equality: prim exact, dist and the record
fields by their bits; a NaN compares equal to a NaN (the payload of a NaN is not specified), as in
the degenerate-ray tests.  Each test builds its rays and the expected values on the CPU (the
`_case_*` functions, which also assert that the rays reach what they are for) and uploads once.
"""
import numpy as np
import pytest

import hit_records as hr
from numpy_restatement import length
from test_gpu_numerics import scale_quads
from test_gpu_occlusion import _check_limits, _five_limits
from test_quad_scan import double_back_wall, edge_rays, far_sphere, quad_scan_fast, v3

pytestmark = pytest.mark.gpu

f32 = np.float32
NO_HIT = hr.NO_HIT
INF = f32(np.inf)


def _same(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def _expected_records(osc, scene, o, d):
    """hit_records.expected_records, which demands the oracle's bits of its own restatements."""
    with np.errstate(all="ignore"):
        return hr.expected_records(osc, *scene, o, d)[0]


def _check_queries(ctx, o, d, prim, dist, want=None, limits=None, what=""):
    """trace_rays and trace_hits against the oracle's (prim, dist) and the expected records,
    occluded against its definition at `limits`."""
    gp, gd = ctx.trace_rays(o, d)
    bad = np.flatnonzero((gp != prim) | ~_same(gd, dist))
    assert bad.size == 0, (f"{what}: trace_rays differs on {bad.size} of {len(o)} rays; first: ray {bad[0]} o={o[bad[0]]} "
                           f"d={d[bad[0]]} got ({gp[bad[0]]}, {gd[bad[0]]!r}) want ({prim[bad[0]]}, {dist[bad[0]]!r})")
    got = ctx.trace_hits(o, d)
    assert np.array_equal(got["prim"], prim) and _same(got["dist"], dist).all(), what
    if want is not None:
        for f in hr.FIELDS:
            same = (got[f] == want[f]) if f in ("prim", "flags") else _same(got[f], want[f])
            bad = np.flatnonzero(~(same.all(axis=1) if same.ndim == 2 else same))
            assert bad.size == 0, (f"{what}: trace_hits field {f} differs on {bad.size} records; first: ray {bad[0]} "
                                   f"got {got[f][bad[0]]!r} want {want[f][bad[0]]!r} prim {prim[bad[0]]}")
    if limits is not None:
        _check_limits(ctx, o, d, prim, dist, limits)


# ------------------------------------------------------------------------------- scaled scenes
def _scaled_scene(wgt, s):
    """double_back_wall(Q) + bunny-2000 + a real sphere of radius 50, all scaled by s."""
    L, Q, S = wgt.cornell_scene()
    T = wgt.procedural_mesh("bunny", 2000).copy()
    S = np.concatenate([S, S])
    S[1]["center"], S[1]["radius"] = (420.0, 100.0, 150.0), 50.0
    L, Q = scale_quads(L, s), scale_quads(double_back_wall(Q), s)
    S["center"] *= f32(s)
    S["radius"] *= f32(s)
    for f in ("v0", "e1", "e2"):
        T[f][:, :3] *= f32(s)
    return L, Q, S, T


def _case_scaled(wgt, oracle, k):
    s = 2.0 ** k
    L0, Q0, _ = wgt.cornell_scene()
    walls = double_back_wall(Q0)
    rng = np.random.default_rng(40)
    n = 700
    tgt = np.stack([rng.uniform(0, 555, n), rng.uniform(0, 555, n), np.full(n, 555.0)], 1).astype(f32)
    o1 = rng.uniform(5, 550, (n, 3)).astype(f32)
    o1[: n // 4] = (278, 278, -800)
    o2, d2 = edge_rays(np.concatenate([L0, walls]), 700, rng)
    # and some at the mesh and at the sphere, which the wall rays reach only by chance
    T0 = wgt.procedural_mesh("bunny", 2000)
    i = rng.integers(0, len(T0), 200)
    c = T0["v0"][i, :3] + (T0["e1"][i, :3] + T0["e2"][i, :3]) / f32(3)
    c = np.concatenate([c, np.array([420.0, 100.0, 150.0]) + rng.uniform(-30, 30, (100, 3))]).astype(f32)
    o3 = rng.uniform(5, 550, (300, 3)).astype(f32)
    o = np.concatenate([o1, o2, o3])
    d = np.concatenate([(tgt - o1).astype(f32), d2, (c - o3).astype(f32)])
    # origins times 2^k; directions times 2^k, and again times 2^-30 and 2^30 (all exact)
    o = np.tile(o * f32(s), (3, 1))
    d = np.concatenate([d * f32(s), d * f32(s) * f32(2.0 ** -30), d * f32(s) * f32(2.0 ** 30)])
    scene = _scaled_scene(wgt, s)
    osc = oracle.OracleScene(*scene)
    prim, dist = osc.trace(o, d)
    want = _expected_records(osc, scene, o, d)
    osc.close()
    L, Q, S, T = scene
    nlq = len(L) + len(Q)
    back = len(L) + int(np.argmax(Q["pos"][:5, 2] * (np.abs(Q["norm"][:5, 2]) == 1)))
    counts = {"earlier wall": int(np.sum(prim == back)), "nearer copy": int(np.sum(prim == nlq - 1)),
              "triangles": int(np.sum((prim >= nlq) & (prim < nlq + len(T)))), "sphere": int(np.sum(prim == nlq + len(T) + 1)),
              "NaN": int(np.sum(np.isnan(dist)))}
    return scene, o, d, prim, dist, want, counts


@pytest.mark.parametrize("k", [-60, -8, 20])
def test_scaled_scenes(ctx, wgt, oracle, k):
    """Walls with the doubled back wall, bunny-2000 and a sphere of radius 50, scaled by 2^k, with
    the tie-making rays of tests/test_quad_scan.py: origins times 2^k, directions times 2^k, 2^(k-30)
    and 2^(k+30) (at 2^-60 direction components down to 2^-81 and below the slab's clamp; at 2^20
    up to 2^59, where the spheres' discriminants overflow)."""
    scene, o, d, prim, dist, want, counts = _case_scaled(wgt, oracle, k)
    print(f"scaled 2^{k}: {len(o)} rays, winners {counts}")
    if k != -60:  # the set bites: ties go both ways, and every primitive class wins somewhere
        assert min(counts["earlier wall"], counts["nearer copy"], counts["triangles"], counts["sphere"]) >= 20, counts
    ctx.upload_scene(*scene)
    _check_queries(ctx, o, d, prim, dist, want, _five_limits(dist), what=f"scaled 2^{k}")


# ------------------------------------------------------- far origins and quad_scan_fast's guards
def _case_far_origins(wgt, oracle):
    """Rays at the unscaled walls from |o| = 2^41, 2^62, 2^64 and 2^100, along the back walls' normal
    (from -z) and across it (from +-x, along the side walls' normal), at several direction scales.

    quad_scan_fast lets its smallest-t quad stand when qt D < 2^62 (the distance is then finite
    and below kRayMax) and, with an earlier candidate at prev, when the two are no almost-tie and
    prev D >= 2^-49.  qt D is the distance travelled along the dominant axis whatever the
    direction's scale, so it is near 2^62 for the origins 2^62 away: the origins there step through
    the floats on both sides of 2^62 and the roundings of t and of qt D put rays on either side of
    the guard.  From 2^62 (2^64) a wall is reached within kRayMax only at direction scales of
    2^-4.4 (2^-2.4) and more, and from scale 4 (1) on the far sphere's discriminant overflows and
    the answer is that sphere with a NaN distance: the smaller scales leave the quad answer the
    query's answer, 2^8 does not.  From 2^100 every wall is beyond kRayMax at any scale.

    The guard was qt D < 2^64, which forgot the sum of the squares in the distance: the diagonal
    rays below, from (-M, -M, -M) with M from 2^61.5 to 2^63.9 along (1, 1, 1) at the box's corner
    (0, 0, 0), reach it at a true distance sqrt(3) M < kRayMax, but from M = 2^63.2 on 3 M^2
    overflows, the reference's distance is infinite and it rejects the quad.  With 2^64 the
    restatement let 43 of these 240 rays stand that the oracle misses (asserted below: where the test
    lets a quad stand the oracle returns that quad, and where the oracle misses it has none).

    prev D < 2^-49 cannot occur under the upload limits, and the set asserts so: an accepted quad
    has |n . d| >= kRayMin with normal components within 2, so D >= kRayMin / 6, and prev >= kRayMin,
    so prev D >= 1.6e-7 > 2^-49 = 1.8e-15.  Rays that start a few floats in front of the
    doubled back wall with |n . d| just above kRayMin come as close as this scene allows: the
    two walls are one ulp of 555 apart, prev D about 1.2e-4."""
    L, Q, S = wgt.cornell_scene()
    walls = double_back_wall(Q)
    S = far_sphere(S)
    rng = np.random.default_rng(41)
    O, D = [], []
    for mag, scales in ((2.0 ** 41, (2.0 ** -20, 1.0, 2.0 ** 20)), (2.0 ** 62, (2.0 ** -4, 2.0 ** -1, 2.0 ** 1)),
                        (2.0 ** 64, (2.0 ** -2, 2.0 ** -1, 2.0 ** 8)),
                        (2.0 ** 100, (2.0 ** -40, 2.0 ** 36))):
        for axis, sign in ((2, -1.0), (0, -1.0), (0, 1.0)):
            for sc in scales:
                n = 150
                # aimed in float64 at a point of the wall the axis meets (the back walls from -z, a side wall
                # from +-x: the ray crosses the other side wall 555 earlier or later, an almost-tie from there)
                tgt = rng.uniform(5, 550, (n, 3))
                tgt[:, axis] = 555.0 if axis == 2 else rng.choice([0.0, 555.0], n)
                o = rng.uniform(5, 550, (n, 3))
                # the floats around mag: steps of -8 .. 8 ulp
                far = (np.full(n, mag, f32).view(np.int32) + rng.integers(-8, 9, n).astype(np.int32)).view(f32)
                o[:, axis] = sign * far
                o = o.astype(f32)
                d = (tgt - o.astype(np.float64)) / mag  # the dominant component is about 1
                O.append(o)
                D.append((d * sc).astype(f32))
    # diagonals at the corner (0, 0, 0): o_i + t d_i cancels exactly, so the aim survives fp32 from any distance
    n = 240
    M = (2.0 ** rng.uniform(61.5, 63.9, n)).astype(f32)
    O.append(-np.stack([M, M, M], 1))
    D.append(np.repeat(rng.choice([0.25, 0.5], n).astype(f32)[:, None], 3, axis=1))
    # just in front of the two back walls with |n . d| just above kRayMin (the smallest D an accepted quad allows)
    n = 300
    o = rng.uniform(5, 550, (n, 3))
    o[:, 2] = 555.0 - rng.integers(2, 7, n) * float(np.spacing(f32(554.0)))  # 2 to 6 floats in front of the walls
    d = rng.normal(0.0, 3e-4, (n, 3))
    d[:, 2] = rng.uniform(1.001e-3, 1.1e-3, n)
    O.append(o.astype(f32))
    D.append(d.astype(f32))
    o, d = np.concatenate(O), np.concatenate(D)
    allq = np.concatenate([L, walls])
    qp, qt, exact, (prev, Dm, Lm) = quad_scan_fast(v3(o), v3(d), allq, details=True)
    hit = qp != NO_HIT
    with np.errstate(all="ignore"):
        below64 = hit & (qt * Dm < f32(2.0 ** 62))
        above64 = hit & ~(qt * Dm < f32(2.0 ** 62))
        two = hit & (prev != INF)
        pd = np.where(two, prev * Dm, np.inf)
    near64 = hit & (Lm > 2.0 ** 61.9) & (Lm < 2.0 ** 62.1)
    counts = {"qt D < 2^62": int(below64.sum()), "qt D >= 2^62": int(above64.sum()),
              "both near 2^62": (int((below64 & near64).sum()), int((above64 & near64).sum())),
              "with prev": int(two.sum()), "smallest prev D": float(pd.min()), "fallback": int((~exact).sum())}
    # both sides of the first guard occur, among the rays 2^62 away too (a few floats apart there)
    assert min(counts["both near 2^62"]) >= 20, counts
    # the second guard has one side only (the docstring says why)
    assert two.sum() >= 100 and np.all(pd >= 2.0 ** -49) and pd.min() < 1e-3, counts
    scene = (L, walls, S)
    osc = oracle.OracleScene(*scene)
    prim, dist = osc.trace(o, d)
    osc.close()
    # the restatement's own check, as tests/test_quad_scan.py: where the test lets the quad stand it is the oracle's
    quad_won = prim < len(allq)
    assert np.array_equal(qp[exact & quad_won], prim[exact & quad_won])
    assert np.all(qp[exact & (prim == NO_HIT)] == NO_HIT)
    diag = (o[:, 0] == o[:, 1]) & (o[:, 1] == o[:, 2]) & (Lm > 2.0 ** 61)
    counts["diagonals: quad, missed by overflow"] = (int(np.sum(diag & quad_won)), int(np.sum(diag & hit & (prim == NO_HIT))))
    assert min(counts["diagonals: quad, missed by overflow"]) >= 20, counts
    won = [int(np.sum(quad_won & ~diag & (Lm > lo) & (Lm < 4 * lo))) for lo in (2.0 ** 40, 2.0 ** 61, 2.0 ** 63, 2.0 ** 99)]
    counts["quad winners at 2^41, 2^62, 2^64, 2^100"] = won
    assert min(won[:3]) >= 100, counts
    return scene, o, d, prim, dist, counts


def test_far_origins_and_quad_scan_guards(ctx, wgt, oracle):
    scene, o, d, prim, dist, counts = _case_far_origins(wgt, oracle)
    print(f"far origins: {len(o)} rays, {counts}")
    ctx.upload_scene(*scene)
    _check_queries(ctx, o, d, prim, dist, None, _five_limits(dist), what="far origins")


# ----------------------------------------------------------------------- occ_t_hi's covered box
def _length32(d):
    return length(tuple(np.ascontiguousarray(d[:, k], f32) for k in range(3))).astype(f32)


def _case_covered_box(wgt, oracle):
    """Rays that hit triangles of bunny-2000 (no walls: from this far a wall would tie with every
    triangle) with each operand of occ_t_hi's `covered` one float inside and one float outside
    its bound.  l1 = |o_x| + |o_y| + |o_z| and m (a limit next to the hit's distance) reach 2^40
    only from 2^40 away, and nd = 2^40 needs a hit at least kRayMin 2^40 away: from that far only
    an exactly axis-parallel ray can be aimed at a triangle, so these rays run along +z and +x.
    nd = 2^-40: unit directions whose fp32 length is exactly 1 or the float below, times 2^-40."""
    L, _, S = wgt.cornell_scene()
    S = S.copy()
    # the dummy sphere (radius 0) where no ray's fp32 discriminant is 0 or NaN: 2^31 beside the lines of the
    # rays along z, and at the origins of the rays along x (whose |d| = 2^40 squares everything else away)
    S["center"][0] = (-2.0 ** 31, 0.0, 0.0)
    T = wgt.procedural_mesh("bunny", 2000)
    rng = np.random.default_rng(42)
    two40, up40, dn40 = f32(2.0 ** 40), np.nextafter(f32(2.0 ** 40), INF), np.nextafter(f32(2.0 ** 40), f32(0))
    O, D, tag = [], [], []

    def along(axis, n, back, step, name):
        i = rng.integers(0, len(T), n)
        c = (T["v0"][i, :3] + (T["e1"][i, :3] + T["e2"][i, :3]) / f32(3)).astype(f32)
        o = c.copy()
        o[:, axis] = -back
        d = np.zeros((n, 3), f32)
        d[:, axis] = step
        O.append(o), D.append(d), tag.extend([name] * n)

    along(2, 300, two40, f32(1.0), "l1 = 2^40")             # dist = 2^40: the limit above it is m's first float outside
    along(2, 300, up40, f32(1.0), "l1 > 2^40")              # dist = the float above 2^40: the limit below it is m = 2^40
    along(2, 300, dn40, f32(1.0), "l1 < 2^40")
    along(0, 300, f32(2.0 ** 31), two40, "nd = 2^40")       # t = 2^-9 >= kRayMin
    along(0, 300, f32(2.0 ** 31), up40, "nd > 2^40")
    # nd around 2^-40 from inside the box
    n = 4000
    o = rng.uniform(5, 550, (n, 3)).astype(f32)
    i = rng.integers(0, len(T), n)
    c = T["v0"][i, :3] + (T["e1"][i, :3] + T["e2"][i, :3]) / f32(3)
    u = (c - o).astype(np.float64)
    u = (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(f32)
    ln = _length32(u)
    for want, name in ((f32(1.0), "nd = 2^-40"), (np.nextafter(f32(1.0), f32(0)), "nd < 2^-40")):
        k = np.flatnonzero(ln == want)[:400]
        O.append(o[k]), D.append(u[k] * f32(2.0 ** -40)), tag.extend([name] * len(k))
    o, d, tag = np.concatenate(O), np.concatenate(D), np.array(tag)
    scene = (L, L[:0], S, T)
    osc = oracle.OracleScene(*scene)
    prim, dist = osc.trace(o, d)
    osc.close()
    tri = (prim >= len(L)) & (prim < len(L) + len(T))
    l1 = (np.abs(o[:, 0]) + np.abs(o[:, 1])) + np.abs(o[:, 2])
    nd = _length32(d)
    below, above = np.nextafter(dist, -INF), np.nextafter(dist, INF)
    # the operands, as the kernel computes them, on rays whose closest hit is a triangle
    sets = {"l1 = 2^40": l1 == two40, "l1 > 2^40": l1 == up40, "nd = 2^40": nd == two40, "nd > 2^40": nd == up40,
            "nd = 2^-40": nd == f32(2.0 ** -40), "nd < 2^-40": nd == np.nextafter(f32(2.0 ** -40), f32(0)),
            "m = 2^40 (at, l1 in)": (dist == two40) & (l1 == two40), "m > 2^40 (above, l1 in)": (above == up40) & (l1 == two40),
            "m = 2^40 (below, l1 out)": (below == two40) & (l1 == up40)}
    counts = {name: int(np.sum(k & tri)) for name, k in sets.items()}
    assert min(counts.values()) >= 50, counts
    limits = [below, dist, above]
    # nd = 2^-40 (and the float below) with m = 2^40 and the float above it: every hit is occluded
    k = np.flatnonzero(np.char.startswith(tag, "nd ") & (nd < 1.0))
    extra = (o[k], d[k], prim[k], dist[k], [np.full(len(k), two40, f32), np.full(len(k), up40, f32)])
    return scene, o, d, prim, dist, limits, extra, counts


def test_occlusion_bound_covered_box(ctx, wgt, oracle):
    scene, o, d, prim, dist, limits, extra, counts = _case_covered_box(wgt, oracle)
    print(f"covered box: {len(o)} rays, triangle hits with {counts}")
    ctx.upload_scene(*scene)
    _check_queries(ctx, o, d, prim, dist, None, limits, what="covered box")
    want = _check_limits(ctx, *extra)
    assert want.mean() > 0.9


# ------------------------------------------------------------------------------ overflow paths
def _case_overflow(wgt, oracle):
    """Finite rays whose intermediates overflow.  (a) |d| = 2^59 from inside the box, with a
    sphere 1e6 away: h^2 and a c are both infinite, the discriminant is NaN, the reference
    accepts the sphere with a NaN distance and k_occluded must answer from closest_hit.  (b) one
    huge direction component beside ordinary ones (2^100 to 2^126): t d overflows, o + t d is
    infinite, the quad coordinates are NaN, the distance infinite (inside the scans: with a
    direction this long the far sphere's discriminant is NaN too, and it is the answer).  (c) |d| = 2^70 to 2^120:
    |d|^2 overflows (k_occluded's first fallback test).  (d) origins near FLT_MAX: l1 overflows."""
    L, Q, S, T = wgt.mesh_scene("bunny", 2000)
    S = np.concatenate([S, far_sphere(S)])
    scene = (L, Q, S, T)
    rng = np.random.default_rng(43)
    o, u = hr.random_rays(1200, rng)
    O, D = [], []
    O.append(o[:300]), D.append(u[:300] * f32(2.0 ** 59))
    d = u[300:600].copy()
    a = rng.integers(0, 3, 300)
    d[np.arange(300), a] *= (2.0 ** rng.integers(100, 127, 300)).astype(f32)
    O.append(o[300:600]), D.append(d)
    O.append(o[600:900]), D.append(u[600:900] * (2.0 ** rng.integers(70, 121, 300)).astype(f32)[:, None])
    big = rng.uniform(300, 550, (300, 3)).astype(f32) * f32(2.0 ** 118)  # finite components whose sum overflows
    O.append(big), D.append((-big * f32(2.0 ** -20)).astype(f32))  # back towards the box
    o, d = np.concatenate(O), np.concatenate(D)
    assert np.isfinite(o).all() and np.isfinite(d).all()
    osc = oracle.OracleScene(*scene)
    prim, dist = osc.trace(o, d)
    want = _expected_records(osc, scene, o, d)
    osc.close()
    with np.errstate(all="ignore"):
        l1 = (np.abs(o[:, 0]) + np.abs(o[:, 1])) + np.abs(o[:, 2])
        nd = _length32(d)
    far = len(L) + len(Q) + len(T) + 1
    counts = {"NaN sphere": int(np.sum((prim == far) & np.isnan(dist))), "|d| overflows": int(np.sum(np.isinf(nd))),
              "l1 overflows": int(np.sum(np.isinf(l1))), "misses": int(np.sum(prim == NO_HIT))}
    assert counts["NaN sphere"] >= 250 and counts["|d| overflows"] >= 500 and counts["l1 overflows"] >= 200, counts
    return scene, o, d, prim, dist, want, counts


def test_overflow_paths(ctx, wgt, oracle):
    scene, o, d, prim, dist, want, counts = _case_overflow(wgt, oracle)
    print(f"overflow: {len(o)} rays, {counts}")
    ctx.upload_scene(*scene)
    lims = _five_limits(dist) + [np.full(len(o), 1e3, f32), np.full(len(o), 1e19, f32)]
    _check_queries(ctx, o, d, prim, dist, want, lims, what="overflow")
