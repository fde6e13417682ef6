"""The oracle and the restatements against float64 geometry (tests/f64_truth.py).

Every GPU test compares a kernel with the C oracle bit for bit; these tests pin the oracle
itself, and with it the triangle rule of DESIGN.md §3.4, to geometry: on every decided ray (the
helper's docstring says which those are) the oracle's BVH and its brute-force scan must return
the float64 primitive, or the float64 miss, with t within 4 E_t.  The triangle rule before this
file existed demanded that t lie inside the slab interval of the triangle's own padded box; for
a triangle that is flat along an axis that interval is narrower than Moller-Trumbore's own
cancellation error in t, and on the flat lattice cases below 1,286 of the 5,000 decided rays
failed (1,252 dropped the hit, 34 returned what lay behind it; none of the 4,978 decided rays
of the general cases, of the bunny or of the sponza stand-in).  The rule now clamps t to the
interval.

Each test prints its share of decided rays and the largest observed error / E_t.
"""
import numpy as np
import pytest

import f64_truth as ft
import hit_records as hr
from hit_records import NO_HIT


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


def _triangle_scene_vs_truth(oracle, name, L, S, tris, o, d, truth, cap, norms=True):
    share = ft.check_share(name, truth, cap)
    nlq, nt = len(L), len(tris)
    osc = oracle.OracleScene(L, L[:0], S, tris)
    tview = ft.tri_view(truth, nlq, nt)
    worst, res = 0.0, {}
    for brute in (True, False):
        tid, t = res["tris", brute] = osc.trace_tris(o, d, brute=brute)
        worst = max(worst, ft.check_closest(f"{name}: trace_tris(brute={brute})", tview, tid, t32=t))
        prim, dist = res["all", brute] = osc.trace(o, d, brute=brute)
        worst = max(worst, ft.check_closest(f"{name}: trace(brute={brute})", truth, prim, dist32=dist))
    assert _same_bits(res["tris", True], res["tris", False]) and _same_bits(res["all", True], res["all", False])
    # the record fields of tests/hit_records.py's triangle restatement
    k = np.flatnonzero(tview["decided"] & (tview["prim"] >= 0))
    tid, t = res["tris", False]
    rec = hr.triangle_records(o[k], d[k], tris, tid[k], t[k], nlq)
    pos_r, norm_ulp = ft.check_records(f"{name}: triangle_records", ft.take(truth, k), rec, norms=norms)
    assert np.array_equal(rec["prim"], truth["prim"][k])
    print(f"{name}: {len(o)} rays, decided {share:.3f}, hits {len(k)}, max error / E_t {worst:.3f}, "
          f"pos {pos_r:.3f}, norm {norm_ulp:.2f} ulp")


@pytest.mark.parametrize("size,offset,flat", ft.LATTICE_SCENES)
def test_lattice_vs_float64(oracle, size, offset, flat):
    """Triangles of one size on a lattice, hit at interior points (margin >= 0.1) from 100 to 1e5
    away (length / size <= 1e5), flat along an axis with the ray along it, or general."""
    tris, _ = ft.lattice_tris(size, offset, flat)
    o, d, _ = ft.lattice_rays(size, offset, flat)
    L, S = ft.tri_scene(far_sphere=True)
    name = f"lattice size {size:g} near {offset:g} {'flat' if flat else 'general'}"
    _triangle_scene_vs_truth(oracle, name, L, S, tris, o, d, ft.lattice_truth(size, offset, flat), ft.CAP_LATTICE)


def test_bunny_vs_float64(oracle):
    tris, o, d, truth = ft.bunny_set()
    _triangle_scene_vs_truth(oracle, "bunny-2000", *ft.tri_scene(), tris, o, d, truth, ft.CAP_MESH)


def test_sponza_vs_float64(oracle):
    tris, o, d, truth = ft.sponza_set()
    _triangle_scene_vs_truth(oracle, "sponza-20000", *ft.tri_scene(), tris, o, d, truth, ft.CAP_MESH)


@pytest.mark.parametrize("kind", ft.SOUP_KINDS)
@pytest.mark.parametrize("log2_scale,offset", ft.SOUP_CASES_CPU)
def test_scaled_soup_vs_float64(oracle, log2_scale, offset, kind):
    """A 300-triangle soup scaled by 2^-12 to 2^31 (coordinates up to 2^40.2; (22, 2e5): 2^39.6
    with edges an upload accepts), hit by rays exactly parallel to an axis from 800 scale away, by
    d = target - o from inside the soup's cube and by unit directions.  An axis-parallel ray has
    two zero direction components, where the slab rule's 1/d is the clamp's:
    with the clamp at 1e-30 the slab offset overflowed from coordinates of 3.4e8 and the oracle
    dropped 1,762 of the 3,000 decided axis hits at 2^20, 2,942 at 2^22, 3,000 at (22, 2e5), 2^30
    and 2^31, and none at 2^-12 and 2^0 (the aimed and unit rays lost none at any scale).
    At 2^30 and 2^31 the aimed rays' full-scene answer is the dummy sphere with a NaN distance
    (f64_truth.sphere_terms; the triangle query is checked as everywhere), and the triangles'
    stored normals are not unit vectors (f64_truth.soup_has_normals)."""
    tris, o, d, truth = ft.scaled_soup_set(log2_scale, offset, kind)
    L, S = ft.soup_scene(log2_scale, offset)
    name = f"soup 2^{log2_scale} offset {offset:g} {kind}"
    _triangle_scene_vs_truth(oracle, name, L, S, tris, o, d, truth, ft.CAP_LATTICE, norms=ft.soup_has_normals(log2_scale))
    nan = int(np.sum(truth["nan_prim"] >= 0))
    if nan:
        print(f"{name}: {nan} rays return the dummy sphere with a NaN distance (its fp32 discriminant is inf - inf)")


def test_cornell_and_sphere_vs_float64(oracle):
    """The Cornell light and quads and a sphere of radius 50, built in float64 from pos, right, up
    and center, radius: the oracle's packed constructors (norm, w, d) and its scan, and the numpy
    restatement's sample_hit with every record field."""
    L, Q, S, o, d, truth = ft.cornell_set()
    share = ft.check_share("cornell", truth, ft.CAP_MESH)
    osc = oracle.OracleScene(L, Q, S)
    worst = 0.0
    for brute in (True, False):
        prim, dist = osc.trace(o, d, brute=brute)
        worst = max(worst, ft.check_closest(f"cornell: trace(brute={brute})", truth, prim, dist32=dist))
    rec = hr.quad_sphere_records(o, d, L, Q, S)
    worst = max(worst, ft.check_closest("cornell: numpy sample_hit", truth, rec["prim"], dist32=rec["dist"]))
    pos_r, norm_ulp = ft.check_records("cornell: numpy sample_hit", truth, rec)
    k = truth["decided"] & (truth["prim"] >= 0)
    hit = np.unique(truth["prim"][k])
    # the set reaches the light, walls, both boxes and the sphere, from both sides
    assert len(hit) >= 15 and hit[-1] == len(L) + len(Q) + 1 and truth["front"][k].any() and not truth["front"][k].all()
    print(f"cornell: {len(o)} rays, decided {share:.3f}, max error / E_t {worst:.3f}, pos {pos_r:.3f}, "
          f"norm {norm_ulp:.2f} ulp, primitives hit {len(hit)}")


def test_flat_box_is_solid(oracle):
    """The user-visible form of the defect: an axis-aligned box of 192 flat unit-scale triangles
    near the origin has no pinholes.  Rays from 100 and 1000 away at points of its faces, along
    the face normal and up to 0.3 rad off it, unit directions and d = target - o."""
    tris = ft.flat_box_mesh()
    L, S = ft.tri_scene(far_sphere=True)
    rng = np.random.default_rng(5)
    O, D = [], []
    for a in range(3):
        for side in (0.0, 3.0):
            n = 300
            p = rng.uniform(0.05, 2.95, (n, 3))
            p[:, a] = side
            tilt, phi = rng.choice([0.0, 0.02, 0.3], n), rng.uniform(0, 2 * np.pi, n)
            dirs = np.zeros((n, 3))
            dirs[:, a] = np.cos(tilt) * (1.0 if side == 0.0 else -1.0)  # from outside
            dirs[:, (a + 1) % 3], dirs[:, (a + 2) % 3] = np.sin(tilt) * np.cos(phi), np.sin(tilt) * np.sin(phi)
            o = (p - rng.choice([100.0, 1000.0], (n, 1)) * dirs).astype(np.float32)
            d = p - o.astype(np.float64)
            d[::2] = ft._unit(d[::2])
            O.append(o)
            D.append(d.astype(np.float32))
    o, d = np.concatenate(O), np.concatenate(D)
    truth = ft.scan(o, d, L, None, S, tris)
    share = ft.check_share("flat box", truth, ft.CAP_LATTICE)
    assert np.all(truth["prim"][truth["decided"]] >= len(L))
    osc = oracle.OracleScene(L, L[:0], S, tris)
    for brute in (True, False):
        prim, dist = osc.trace(o, d, brute=brute)
        assert not np.any(prim[truth["decided"]] == NO_HIT)
        ft.check_closest(f"flat box: trace(brute={brute})", truth, prim, dist32=dist)
    print(f"flat box: decided {share:.3f}")


# ------------------------------------------------------------- the helper against closed forms
def test_truth_closed_forms():
    """scan on cases with known answers: a triangle in the plane z = 100 hit at t = 900 (as
    tests/test_oracle_kats.py), a ray through its edge (undecided), one beside it (a decided
    miss), a sphere from outside and from inside, a quad's back face."""
    import webgputracer_amd as w

    tri = w.make_triangles(np.float32([[[0, 0, 100], [600, 0, 100], [0, 600, 100]]]))
    o = np.float32([[50, 50, -800], [300, 300, -800], [400, 400, -800], [50, 50, 1000]])
    d = np.float32([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, -2]])
    r = ft.scan_tris(o, d, tri)
    assert list(r["prim"]) == [0, 0, -1, 0] and list(r["decided"]) == [True, False, True, True]
    assert r["t"][0] == 900.0 and r["t"][3] == 450.0 and r["dist"][3] == 900.0
    assert np.allclose(r["margin"][0], 50 / 600) and abs(r["margin"][1]) < 1e-12
    assert list(r["front"]) == [False, False, False, True]  # e1 x e2 = +z: seen from -z is the back
    assert np.array_equal(r["norm"][0], [0, 0, -1]) and np.array_equal(r["norm"][3], [0, 0, 1])
    assert 0 < r["E_t"][0] < 1e-3 and 0 < r["E_m"][0] < 1e-5
    L, Q, S = w.cornell_scene()
    S = S.copy()
    S["center"][0], S["radius"][0] = (400, 400, 278), 50
    r = ft.scan(np.float32([[400, 400, -800], [400, 400, 278], [278, 800, 278]]),
                np.float32([[0, 0, 1], [0, 0, 1], [0, -1, 0]]), L, Q[:5], S)
    assert list(r["decided"]) == [True, True, True]
    assert r["prim"][0] == 6 and r["t"][0] == 1028.0 and r["front"][0]      # sphere: 1078 - 50
    assert r["prim"][1] == 6 and r["t"][1] == 50.0 and not r["front"][1]    # from inside: the far root
    assert np.array_equal(r["norm"][1], [0, 0, -1])
    # the ceiling (y = 555) from above: the normal is turned against the ray
    assert r["prim"][2] == 3 and np.isclose(r["t"][2], 800 - 555) and np.allclose(r["norm"][2], [0, 1, 0])
