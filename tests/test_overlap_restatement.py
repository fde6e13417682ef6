"""The triangle overlap query's definition (wgt_overlap_triangles_spec: the host brute force over wgt_overlap.h)
against an independent numpy statement of it (tests/overlap_restatement.py) bit for bit, its known answers,
its consequences, and its float32 decisions against the same formulas in float64.  No device (no GPU needed).
"""
import numpy as np
import pytest

import nearest_cases as nc
import overlap_cases as oc
import overlap_restatement as rs

f32 = np.float32
NO_HIT = np.uint32(0xFFFFFFFF)


def assert_same(got, want, what):
    for f in ("hit", "count", "prim"):
        if f in got:
            assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f)
            bad = np.flatnonzero((got[f] != want[f]).reshape(len(got[f]), -1).any(1))
            assert bad.size == 0, (f"{what}: {f} differs at {bad.size} of {len(got[f])} queries; first {bad[0]}: the spec "
                                   f"gives {got[f][bad[0]]!r}, the restatement {want[f][bad[0]]!r}")


def both(wgt, T, Q, k, what, first_prim=0):
    """The spec and the restatement on (T, Q) at k, compared; -> the spec's."""
    got = wgt.overlap_triangles_spec(T, Q, k, first_prim=first_prim)
    assert_same(got, rs.overlap(T, Q, k, first_prim=first_prim), what)
    return got


@pytest.fixture(scope="module")
def bunny_answer(wgt):
    """The spec on the main case at k = 32, computed once."""
    return wgt.overlap_triangles_spec(nc.bunny(), oc.bunny_queries(), 32, first_prim=7)


def test_bunny_against_its_own_triangles(wgt, bunny_answer):
    """bunny2000 against 512 queries made from its own triangles, rotated and shifted."""
    T, Q = nc.bunny(), oc.bunny_queries()
    assert_same(bunny_answer, rs.overlap(T, Q, 32, first_prim=7), "bunny, k = 32")
    c = bunny_answer["count"]
    print(f"bunny: {np.count_nonzero(c)} of {len(c)} queries overlap, at most {c.max()} triangles, {c.sum()} pairs")
    assert np.count_nonzero(c) > len(c) // 2 and c.max() < len(T) // 10


def test_known_answers(wgt):
    T = oc.unit_tris()
    for name, (q, count) in oc.known_answers().items():
        got = both(wgt, T, np.array([q], f32), 1, name, first_prim=3)
        assert got["count"][0] == count and got["hit"][0] == (count > 0), (name, got)
        assert got["prim"][0, 0] == (3 if count else NO_HIT), (name, got)
    # the box clause is what decides the one-ulp pair: it holds at the pad's plane and fails one float past it
    v0, e1, e2 = (T[f][:, :3] for f in ("v0", "e1", "e2"))
    lo, hi = rs.tri_box(v0, e1, e2)
    assert hi[0, 0] == oc.unit_box_hi_x() > 1.0
    ka = oc.known_answers()
    for name, holds in (("box touches the pad", True), ("box misses by one ulp", False)):
        a = np.array(ka[name][0], f32)
        assert bool(rs.box_clause(a[0], a[1], a[2], lo[0], hi[0])) == holds, name


def test_invalid_queries_are_empty(wgt):
    T = oc.unit_tris()
    for name, q in oc.invalid_queries().items():
        got = both(wgt, T, q[None], 2, name)
        assert not got["hit"][0] and got["count"][0] == 0 and (got["prim"] == NO_HIT).all(), (name, got)
    got = both(wgt, T, oc.longest_valid_query()[None], 2, "an edge of exactly 2^30")
    assert got["count"][0] == 1 and list(got["prim"][0]) == [0, NO_HIT]
    # between valid queries, in one call
    Q, odd = oc.interleaved(oc.bunny_queries()[:128])
    got = both(wgt, nc.bunny(), Q, 8, "interleaved")
    assert odd.sum() == 32 and not got["count"][odd].any() and got["count"][~odd].any()


def test_zero_area_queries_and_degenerate_meshes(wgt):
    """Whatever the restatement says, the spec says; counts stay counts."""
    for name, T in (("bunny", nc.bunny()), ("degenerate_mix", nc.degenerate_mix())):
        for what, Q in (("zero-area queries", oc.zero_area_queries(T)), ("own triangles", oc.from_own_triangles(T, 64, 29)),
                        ("its corners as queries", oc.corners(T)[:64])):
            got = both(wgt, T, Q, 8, f"{name}, {what}")
            assert (got["count"] <= len(T)).all() and ((got["prim"] == NO_HIT) | (got["prim"] < len(T))).all()
    assert not wgt.overlap_triangles_spec(nc.bunny()[:0], oc.bunny_queries()[:8], 4)["count"].any()  # no triangles


def test_copies64_overflows_the_list(wgt):
    Q = oc.through_copies64()
    got = both(wgt, nc.copies64(), Q, 32, "copies64", first_prim=5)
    assert list(got["count"]) == [64, 64, 0]
    assert (got["prim"][:2] == 5 + np.arange(32, dtype=np.uint32)).all() and (got["prim"][2] == NO_HIT).all()


def test_consequences(wgt, bunny_answer):
    """The list for k is a prefix of the list for any larger k; hit == (count > 0); kNoHit beyond
    min(count, k); ids ascending; only the mesh's ids."""
    T, Q = nc.bunny(), oc.bunny_queries()
    full = bunny_answer
    for k in oc.KS:
        if k == 0:  # no list: prim is refused at k == 0, the other two fields are the same
            got = wgt.overlap_triangles_spec(T, Q, 0, first_prim=7, want=("hit", "count"))
            with pytest.raises(wgt.tracer.WgtError, match="k == 0"):
                wgt.overlap_triangles_spec(T, Q, 0, first_prim=7)
        else:
            got = wgt.overlap_triangles_spec(T, Q, k, first_prim=7)
            assert np.array_equal(got["prim"], full["prim"][:, :k]), k
            have = np.arange(k)[None, :] < np.minimum(got["count"], k)[:, None]
            assert ((got["prim"] != NO_HIT) == have).all(), k
            assert (got["prim"][have] >= 7).all() and (got["prim"][have] < 7 + len(T)).all()
            assert (np.diff(got["prim"].astype(np.int64), axis=1)[have[:, 1:]] > 0).all(), k
        assert np.array_equal(got["count"], full["count"]) and np.array_equal(got["hit"], full["count"] > 0), k
        assert got["hit"].dtype == bool and got["count"].dtype == np.uint32
    # each field alone is the same field
    for f in ("hit", "count", "prim"):
        one = wgt.overlap_triangles_spec(T, Q, 8 if f == "prim" else 0, first_prim=7, want=(f,))
        assert list(one) == [f] and np.array_equal(one[f], full[f][:, :8] if f == "prim" else full[f])
    # coplanar pairs are never reported: a triangle of exact small integers against itself and against a
    # copy moved within its plane
    own = np.array([[[0, 0, 0], [4, 0, 0], [0, 4, 0]], [[1, 1, 0], [5, 1, 0], [1, 5, 0]]], f32)
    flat = wgt.overlap_triangles_spec(wgt.make_triangles(own[:1]), own, 1)
    assert not flat["hit"].any() and not flat["count"].any()


def spec_pairs(wgt, A, rec, chunk=32):
    """The spec's decision on pair i = (A[i], rec[i]): blocks of `chunk` records against their own queries at
    k = chunk (the list is complete), pair i's decision is whether query i lists triangle i."""
    v0, e1, e2 = rec
    n = len(A)
    T = np.zeros(n, wgt.tracer.TRI_DTYPE)
    T["v0"][:, :3], T["e1"][:, :3], T["e2"][:, :3] = v0, e1, e2
    yes = np.zeros(n, bool)
    own = np.arange(chunk, dtype=np.uint32)[:, None]
    for b in range(0, n, chunk):
        prim = wgt.overlap_triangles_spec(T[b:b + chunk], A[b:b + chunk], chunk, want=("prim",))["prim"]
        yes[b:b + chunk] = (prim == own[:len(prim)]).any(1)
    return yes


@pytest.mark.parametrize("name", list(oc.pair_sets()))
def test_float32_decisions_against_float64(wgt, name):
    """On 10^5 random pairs per set the float32 definition and the same formulas in float64 on the same
    float32 inputs agree on every pair that is not marginal (overlap_restatement.margins below 1e-4), and
    marginal pairs are at most 1 % of the set.  The restatement decides all pairs; the spec itself decides
    the first 8,192 of each set, block by block."""
    A, rec = oc.pair_sets()[name]
    d32 = rs.tri_overlap(A, *rec, dtype=f32)
    d64 = rs.tri_overlap(A, *rec, dtype=np.float64)
    marginal = rs.margins(A, *rec) < 1e-4
    differ = d32 != d64
    print(f"{name}: {d64.mean():.2%} of {len(A)} pairs overlap, {marginal.mean():.3%} are marginal, float32 and float64 "
          f"differ on {differ.sum()} ({(differ & ~marginal).sum()} of them not marginal)")
    assert marginal.mean() <= 0.01
    assert not (differ & ~marginal).any()
    assert 0.05 < d64.mean() < 0.6  # the sets do exercise both answers
    m = 8192
    assert np.array_equal(spec_pairs(wgt, A[:m], tuple(r[:m] for r in rec)), d32[:m])
