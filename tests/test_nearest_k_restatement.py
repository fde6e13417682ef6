"""The k-nearest closest-point query's host definition (wgt_nearest_k_points_spec, webgputracer_amd/csrc/
wgt_nearest_k.h) against its numpy restatement (tests/nearest_k_restatement.py) on every case of
tests/nearest_cases.py at k = 1, 2, 8 and 32, with and without radii: equality of bits in every field, no
tolerance, no excluded point; and the consequences the header states.  CPU only."""
import functools

import numpy as np
import pytest

import nearest_cases as nc
import nearest_k_restatement as nk

f32 = np.float32
INF = f32(np.inf)
FIELDS = ("count", "prim", "dist", "pos", "uv")
KS = (1, 2, 8, 32)
FP = 7  # first_prim
N_RADIUS = 600  # points of a case the radius runs use


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(got, want, what, fields=FIELDS):
    for k in fields:
        g, w = bits(got[k]), bits(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
        assert bad.size == 0, f"{what}: {k} differs at {bad.size} of {len(g)} points; first {bad[0]}: {got[k][bad[0]]!r} != {want[k][bad[0]]!r}"


@functools.lru_cache(maxsize=None)
def ranked(name, n=None):
    T, P, _ = nc.cpu_cases()[name]
    return nk.Ranked(T, P[:n])


@pytest.mark.parametrize("name", list(nc.cpu_cases()))
def test_spec_equals_the_numpy_statement(wgt, name):
    T, P, _ = nc.cpu_cases()[name]
    rk = ranked(name)
    prev = None
    for k in KS:
        got = wgt.nearest_k_points_spec(T, P, k, first_prim=FP)
        assert_same(got, nk.nearest_k_points(rk, k, first_prim=FP), f"{name}, k = {k}")
        # entry 0 is wgt_nearest_points' record, in all four fields
        one = wgt.nearest_points_spec(T, P, first_prim=FP)
        for f in ("prim", "dist", "pos", "uv"):
            assert np.array_equal(bits(got[f][:, 0]), bits(one[f])), (name, k, f)
        # the list for k is a prefix of the list for a larger k; the count does not depend on k
        if prev is not None:
            pk = prev["prim"].shape[1]
            for f in ("prim", "dist", "pos", "uv"):
                assert np.array_equal(bits(got[f][:, :pk]), bits(prev[f])), (name, k, f)
            assert np.array_equal(got["count"], prev["count"])
        prev = got
        # entries beyond min(count, k) are the miss entry, those before it are not
        j = np.arange(k)[None, :]
        miss = j >= np.minimum(got["count"], k)[:, None]
        assert np.array_equal(got["prim"] == nk.NO_HIT, miss)
        assert np.isposinf(got["dist"][miss]).all() and not got["pos"][miss].any() and not got["uv"][miss].any()
        # ascending by dist (by d2, hence by its monotone root)
        d = np.where(miss, INF, got["dist"])
        assert (d[:, 1:] >= d[:, :-1]).all()
    # each field asked for alone gives the same; count alone ignores k
    for f in FIELDS:
        alone = wgt.nearest_k_points_spec(T, P, 8 if f != "count" else 99, first_prim=FP, want=(f,))
        want = prev[f] if f == "count" else prev[f][:, :8]
        assert list(alone) == [f] and np.array_equal(bits(alone[f]), bits(want)), (name, f)


@pytest.mark.parametrize("name", list(nc.cpu_cases()))
def test_radii(wgt, name):
    """radius_sets of the entry-0 distance (0.5 D, D, the float above, 2 D, +inf, 0, -1, NaN), and one float
    below, at and above each point's 5th distance: the count is the number of triangles whose dist < m."""
    T, P, _ = nc.cpu_cases()[name]
    P = P[:N_RADIUS]
    rk = ranked(name, N_RADIUS)
    free = wgt.nearest_k_points_spec(T, P, 8, first_prim=FP)
    D0 = free["dist"][:, 0]
    some = (free["prim"][:, 0] != nk.NO_HIT)
    want_any = [False, False, True, True, True, False, False, False]
    for lim, hit in zip(nc.radius_sets(D0), want_any):
        for k in (1, 8):
            got = wgt.nearest_k_points_spec(T, P, k, max_dist=lim, first_prim=FP)
            assert_same(got, nk.nearest_k_points(rk, k, max_dist=lim, first_prim=FP), f"{name} radius, k = {k}")
            assert np.array_equal(got["count"] > 0, some & hit)
            one = wgt.nearest_points_spec(T, P, max_dist=lim, first_prim=FP)
            for f in ("prim", "dist", "pos", "uv"):
                assert np.array_equal(bits(got[f][:, 0]), bits(one[f])), (name, k, f)
            with np.errstate(invalid="ignore"):
                assert np.array_equal(got["count"], (rk.all_dist < np.asarray(lim, f32)[:, None]).sum(1))
    if len(T) < 5:
        return
    D5 = free["dist"][:, 4]  # +inf where fewer than five triangles have a finite d2
    for lim in nc.around(D5):
        for k in (2, 8, 32):
            got = wgt.nearest_k_points_spec(T, P, k, max_dist=lim, first_prim=FP)
            assert_same(got, nk.nearest_k_points(rk, k, max_dist=lim, first_prim=FP), f"{name} 5th-distance radius, k = {k}")
            # within the radius is a prefix of the free list
            cut = np.arange(min(k, 8))[None, :] < np.minimum(got["count"], k)[:, None]
            assert np.array_equal(got["prim"][:, :8], np.where(cut, free["prim"][:, :min(k, 8)], nk.NO_HIT))
    # the float above the 5th distance holds at least five triangles wherever there are five
    got = wgt.nearest_k_points_spec(T, P, 1, max_dist=np.nextafter(D5, INF), first_prim=FP, want=("count",))
    assert (got["count"][np.isfinite(D5)] >= 5).all()
    inf = wgt.nearest_k_points_spec(T, P, 8, max_dist=np.inf, first_prim=FP)
    assert_same(inf, free, "NULL radius = +inf")


def test_ties_degenerates_and_padding(wgt):
    T, P, _ = nc.cpu_cases()["copies64"]
    got = wgt.nearest_k_points_spec(T, P, 32, first_prim=FP)
    assert (got["count"] == 64).all()
    assert (got["prim"] == FP + np.arange(32, dtype=np.uint32)[None, :]).all()  # ids 0..31 of the 64 tied triangles
    assert (bits(got["dist"]) == bits(got["dist"][:, :1])).all()
    # k above the triangle count pads with the miss entry
    for name, nt in (("kat", 1), ("no_triangles", 0)):
        T, P, _ = nc.cpu_cases()[name]
        got = wgt.nearest_k_points_spec(T, P, 8, first_prim=FP)
        assert (got["count"] == nt).all() and (got["prim"][:, :nt] == FP).all()
        assert (got["prim"][:, nt:] == nk.NO_HIT).all() and np.isposinf(got["dist"][:, nt:]).all()
        assert not got["pos"][:, nt:].any() and not got["uv"][:, nt:].any()
    T, P, _ = nc.cpu_cases()["bad_points"]
    got = wgt.nearest_k_points_spec(T, P, 8, first_prim=FP)
    odd = ~np.isfinite(P).all(1)
    assert odd.sum() >= 24 and (got["count"][odd] == 0).all() and (got["prim"][odd] == nk.NO_HIT).all()
    assert (got["count"][~odd] == np.isfinite(ranked("bad_points").all_dist[~odd]).sum(1)).all()
    for name in ("degenerate_mix", "degenerate_only"):
        T, P, _ = nc.cpu_cases()[name]
        got = wgt.nearest_k_points_spec(T, P, 32, first_prim=FP)
        assert not np.isnan(got["dist"]).any() and not np.isnan(got["pos"]).any()


def test_equal_dist_is_ordered_by_d2_not_by_id(wgt):
    """Two triangles whose d2 are neighbouring floats with the same rounded root: the one with the smaller
    d2 comes first although its id is higher.  The origin is nearest to corner v0 of both; v0 = (2.5, y, 0)
    with y^2 about 2^-21, one ulp of 6.25, gives d2 = the float above 6.25, whose root is 2.5 + 0.4 ulp."""
    y = f32(2.0 ** -10.5)
    tri = lambda y0: [[2.5, y0, 0], [3.5, y0 + 1, 0], [3.5, y0 - 1, 0]]
    T = wgt.make_triangles(np.array([tri(y), tri(0.0)], f32))
    P = np.zeros((1, 3), f32)
    rk = nk.Ranked(T, P)
    assert list(rk.order[0]) == [1, 0] and rk.d2[0, 0] == f32(6.25) and rk.d2[0, 1] == np.nextafter(f32(6.25), INF)
    assert rk.dist[0, 0] == rk.dist[0, 1] == f32(2.5)
    got = wgt.nearest_k_points_spec(T, P, 2)
    assert list(got["prim"][0]) == [1, 0] and got["dist"][0, 0] == got["dist"][0, 1] == f32(2.5)
    assert_same(got, nk.nearest_k_points(rk, 2), "equal dist")
    # a radius between the two would be between two equal dists: both are in or both are out
    for m, c in ((f32(2.5), 0), (np.nextafter(f32(2.5), INF), 2)):
        assert wgt.nearest_k_points_spec(T, P, 2, max_dist=m)["count"][0] == c
