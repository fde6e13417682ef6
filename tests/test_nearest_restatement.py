"""The closest-point query's host definition (wgt_nearest_points_spec, webgputracer_amd/csrc/wgt_nearest.h)
against its numpy restatement (tests/nearest_restatement.py) on every case of tests/nearest_cases.py: equality
of bits in every field, no tolerance, no excluded point.  CPU only."""
import numpy as np
import pytest

import nearest_cases as nc
import nearest_restatement as nr

f32 = np.float32


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what):
    for k in ("prim", "dist", "pos", "uv"):
        g, w = bits(got[k]), bits(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
        assert bad.size == 0, f"{what}: {k} differs at {bad.size} of {len(g)} points; first {bad[0]}: {got[k][bad[0]]!r} != {want[k][bad[0]]!r}"


@pytest.fixture(scope="module")
def restated():
    """name -> the numpy statement's answers without a radius, computed once."""
    return {name: nr.nearest_points(T, P, first_prim=7) for name, (T, P, _) in nc.cpu_cases().items()}


@pytest.mark.parametrize("name", list(nc.cpu_cases()))
def test_spec_equals_the_numpy_statement(wgt, restated, name):
    T, P, _ = nc.cpu_cases()[name]
    got = wgt.nearest_points_spec(T, P, first_prim=7)
    assert_same(got, restated[name], name)
    # each field asked for alone gives the same
    for k in ("prim", "dist", "pos", "uv"):
        one = wgt.nearest_points_spec(T, P, first_prim=7, want=(k,))
        assert list(one) == [k] and np.array_equal(bits(one[k]), bits(got[k]))


def test_known_answers_one_point_per_region(wgt):
    T = nc.kat_tris()
    P = np.array([k[0] for k in nc.KAT], f32)
    for name, r in (("spec", wgt.nearest_points_spec(T, P)), ("numpy", nr.nearest_points(T, P))):
        for i, (p, (v, w), d2) in enumerate(nc.KAT):
            assert r["prim"][i] == 0, (name, i)
            assert (r["uv"][i] == f32([v, w])).all(), (name, i, r["uv"][i])
            assert r["dist"][i] == np.sqrt(f32(d2)), (name, i, r["dist"][i])
            assert (r["pos"][i] == f32([v, w, 0.0])).all(), (name, i, r["pos"][i])
    assert list(nr.nearest_points(T, P)["region"]) == nc.KAT_REGION


def test_the_main_sets_mix_the_regions(restated):
    """Uniform points in the box are answered by vertices, edges and faces, at least 5 % each; points
    within 2 units of the surface all land on faces."""
    reg = restated["box"]["region"]
    share = [np.mean(reg == k) for k in (nr.VERTEX, nr.EDGE, nr.FACE)]
    print("box set: vertex %.3f edge %.3f face %.3f" % tuple(share))
    assert min(share) >= 0.05, share
    assert (restated["surface"]["region"] == nr.FACE).all()


def test_radius_decides_the_report(wgt, restated):
    T, P = nc.bunny(), nc.box_points()[:500]
    D = restated["box"]["dist"][:500]
    sets = nc.radius_sets(D)
    want_hit = [False, False, True, True, True, False, False, False]
    for lim, hit in zip(sets, want_hit):
        got = wgt.nearest_points_spec(T, P, max_dist=lim, first_prim=7)
        assert_same(got, nr.nearest_points(T, P, max_dist=lim, first_prim=7), "radius")
        assert ((got["prim"] != nr.NO_HIT) == hit).all()
        if not hit:
            assert np.isposinf(got["dist"]).all() and not got["pos"].any() and not got["uv"].any()
    inf = wgt.nearest_points_spec(T, P, max_dist=np.inf, first_prim=7)
    assert_same(wgt.nearest_points_spec(T, P, first_prim=7), inf, "NULL radius = +inf")


def test_ties_and_degenerates(wgt, restated):
    assert (restated["copies64"]["prim"] == 7).all()  # the lowest id of 64 copies
    assert not np.isnan(restated["degenerate_mix"]["dist"]).any()
    only = restated["degenerate_only"]
    assert not np.isnan(only["dist"]).any()
    bad = restated["bad_points"]
    P = nc.bad_points()
    odd = ~np.isfinite(P).all(1)
    assert odd.sum() >= 24 and (bad["prim"][odd] == nr.NO_HIT).all() and (bad["prim"][~odd] != nr.NO_HIT).all()
    assert (restated["no_triangles"]["prim"] == nr.NO_HIT).all()
