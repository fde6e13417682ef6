"""The self-intersection query's definition (wgt_overlap_self_spec: the host brute force over
wgt_overlap_self.h) against an independent numpy statement of it (tests/overlap_self_restatement.py) bit for
bit on every mesh of tests/self_overlap_cases.py, its consequences, its relation to wgt_overlap_triangles_spec,
and its float32 decisions against the same formulas in float64.  No device (no GPU needed).
"""
import numpy as np
import pytest

import overlap_cases as oc
import overlap_self_restatement as srs
import self_overlap_cases as sc

f32 = np.float32
NO_HIT = np.uint32(0xFFFFFFFF)
FIRST = 5  # the primitive id of triangle 0 in these tests


def assert_same(got, want, what):
    for f in ("hit", "count", "prim"):
        assert got[f].dtype == want[f].dtype and got[f].shape == want[f].shape, (what, f)
        bad = np.flatnonzero((got[f] != want[f]).reshape(len(got[f]), -1).any(1))
        assert bad.size == 0, (f"{what}: {f} differs at {bad.size} of {len(got[f])} triangles; first {bad[0]}: the spec "
                               f"gives {got[f][bad[0]]!r}, the restatement {want[f][bad[0]]!r}")


def spec(wgt, name, indexed, k):
    want = ("hit", "count", "prim") if k else ("hit", "count")
    got = wgt.overlap_self_spec(sc.records(name), sc.labels(name, indexed), k, first_prim=FIRST, want=want)
    if not k:
        got["prim"] = np.zeros((len(got["hit"]), 0), np.uint32)
    return got


def members(answer, n):
    """(n, n) bool from a complete list (every count <= k)."""
    assert (answer["count"] <= answer["prim"].shape[1]).all()
    M = np.zeros((n, n), bool)
    s, j = np.nonzero(answer["prim"] != NO_HIT)
    M[s, answer["prim"][s, j] - FIRST] = True
    return M


@pytest.mark.parametrize("indexed", [True, False], ids=["indexed", "unindexed"])
@pytest.mark.parametrize("name", sc.NAMES)
def test_the_spec_equals_the_restatement(wgt, name, indexed):
    """Bit for bit at k = 0, 1, 4, 32; the list for k is a prefix of the list for a larger k; hit == count > 0."""
    T, L = sc.records(name), sc.labels(name, indexed)
    got = {k: spec(wgt, name, indexed, k) for k in sc.KS}
    for k in sc.KS:
        assert_same(got[k], srs.overlap_self(T, L, k, first_prim=FIRST), f"{name}, k = {k}")
        assert np.array_equal(got[k]["hit"], got[k]["count"] > 0)
        assert np.array_equal(got[k]["prim"], got[32]["prim"][:, :k])
        assert np.array_equal(got[k]["count"], got[32]["count"])
    c = got[32]["count"]
    print(f"{name}, {'indexed' if indexed else 'unindexed'}: {len(T)} triangles, {np.count_nonzero(c)} cut something, "
          f"at most {c.max()}, {c.sum() // 2} pairs")


@pytest.mark.parametrize("indexed", [True, False], ids=["indexed", "unindexed"])
@pytest.mark.parametrize("name", sc.NAMES)
def test_symmetry(wgt, name, indexed):
    """t in S_s iff s in S_t, from the spec's own lists, which it fills one ordered pair at a time.  The large
    triangle's list is cut at 32, so its row is taken from its partners' lists and its count."""
    n = len(sc.records(name))
    a = spec(wgt, name, indexed, 32)
    long = np.flatnonzero(a["count"] > 32)
    assert list(long) == ([sc.BIG] if name == "forty_through_one" else [])
    M = np.zeros((n, n), bool)
    s, j = np.nonzero(a["prim"] != NO_HIT)
    M[s, a["prim"][s, j] - FIRST] = True
    for b in long:
        assert not (M[b] & ~M[:, b]).any() and M[:, b].sum() == a["count"][b]
        M[b] = M[:, b]
    assert np.array_equal(M, M.T) and not M.diagonal().any()
    assert np.array_equal(M.sum(1), a["count"])


@pytest.mark.parametrize("name", sc.NAMES)
def test_what_the_overlap_query_reports_is_reported(wgt, name):
    """For s < t not adjacent, tri_overlap(corners(s), record t) by wgt_overlap_triangles_spec implies
    self_overlap(s, t): the same segment tests, and a box clause that is a superset."""
    T, L = sc.records(name), sc.labels(name)
    n = len(T)
    Q = oc.corners(T)
    O = np.stack([wgt.overlap_triangles_spec(T[t:t + 1], Q, 0, want=("hit",))["hit"] for t in range(n)], 1)  # O[s, t]
    for indexed in (True, False):
        M = srs.matrix(T, L if indexed else None)  # equals the spec's (test_the_spec_equals_the_restatement)
        free = np.triu(~srs.adjacent(L if indexed else None, n), 1)
        assert not (O & free & ~M).any(), name
    print(f"{name}: the overlap query reports {int((O & np.triu(np.ones((n, n), bool), 1)).sum())} pairs s < t")


def test_the_flat_grid_is_empty_with_indices(wgt):
    a = spec(wgt, "grid", True, 32)
    assert not a["hit"].any() and not a["count"].any() and (a["prim"] == NO_HIT).all()


def test_without_indices_the_grid_reports_its_neighbours(wgt):
    """What the feature exists to remove: every interior triangle of the sheet reports triangles it merely
    touches, and every triangle reported shares a vertex with it."""
    a = spec(wgt, "grid", False, 32)
    inner = sc.grid_interior()
    assert len(inner) == 32 and (a["count"][inner] > 0).all(), a["count"][inner]
    M = members(a, 72)
    assert not (M & ~srs.adjacent(sc.labels("grid"), 72)).any()
    print(f"unindexed sheet: {a['count'].min()} to {a['count'].max()} neighbours reported per triangle")


def test_forty_crossings(wgt):
    a = spec(wgt, "forty_through_one", True, 32)
    others = np.array([i for i in range(41) if i != sc.BIG], np.uint32)
    assert a["count"][sc.BIG] == 40 and np.array_equal(a["prim"][sc.BIG], FIRST + others[:32])
    assert (a["count"][others] == 1).all() and (a["prim"][others, 0] == FIRST + sc.BIG).all()
    assert (a["prim"][others, 1:] == NO_HIT).all()


def test_known_small_cases(wgt):
    assert spec(wgt, "one", True, 4)["count"].tolist() == [0]
    assert spec(wgt, "shared_edge", True, 4)["count"].tolist() == [0, 0]
    a = spec(wgt, "crossing", True, 4)
    assert a["count"].tolist() == [1, 1] and a["prim"][:, 0].tolist() == [FIRST + 1, FIRST]
    # the fold: quad 5 (triangles 10, 11) comes down through quad 1 at x = 3.67, where it spans y = 0.57 .. 1.57;
    # of quad 1 only triangle 3 reaches there (triangle 2 ends at y = 0.35 on that line).  Nothing once it is opened.
    a = spec(wgt, "strip_folded", True, 32)
    assert set(np.flatnonzero(a["hit"])) == {3, 10, 11}, np.flatnonzero(a["hit"])
    T = wgt.make_triangles(sc.strip_opened()[0])
    assert not wgt.overlap_self_spec(T, sc.strip_opened()[1], 0, want=("hit",))["hit"].any()
    # unwelded, the fold is still found, and so is every neighbour
    u = spec(wgt, "strip_unwelded", True, 32)
    assert (u["count"] >= a["count"]).all() and u["count"].sum() > a["count"].sum()
    assert np.array_equal(u["prim"], spec(wgt, "strip_unwelded", False, 32)["prim"])
    # duplicates: both copies of the piercing triangle cut triangle 0 and its copy; copies do not cut each other
    d = members(spec(wgt, "degenerate", True, 32), 8)
    assert d[0, [1, 2, 3]].all() and d[7, [1, 2, 3]].all() and not d[1, [2, 3]].any() and not d[2, 3] and not d[0, 7]
    assert not d[4].any()  # a point cuts nothing: every determinant with a zero edge is zero


@pytest.mark.parametrize("name", sc.NAMES)
def test_float32_against_float64(name):
    """The restatement's decisions in float32 and in float64 on the fixtures.  Where they differ the pair is
    marginal (a touching or nearly coplanar pair, decided by rounding): those are listed by count.  Without
    indices they are many, for every pair of neighbours touches: one more reason adjacency is taken from labels."""
    T, L = sc.records(name), sc.labels(name)
    for labels in (L, None):
        m32, m64 = srs.matrix(T, labels), srs.matrix(T, labels, np.float64)
        differ = int(np.triu(m32 != m64, 1).sum())
        print(f"{name}, {'indexed' if labels is not None else 'unindexed'}: {int(np.triu(m64, 1).sum())} pairs in float64, "
              f"{int(np.triu(m32, 1).sum())} in float32, {differ} differ")
        if labels is not None and name not in ("degenerate", "strip_unwelded"):
            # with neighbours excluded nothing here touches: the fixtures' pairs are firm (the unwelded strip's
            # labels exclude nobody, and the degenerate mesh touches by construction)
            assert differ == 0, (name, np.argwhere(np.triu(m32 != m64, 1)))
