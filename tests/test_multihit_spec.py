"""The multi-hit specification helper (tests/multihit_spec.py) against the full CPU oracle, on the Cornell
box plus three concentric UV spheres with 4,000 random rays: the minimum over the single-primitive scenes is
the full scene's closest hit, and the second entry is the closest hit of the scene without the first
primitive (peeling one level).  CPU only; every comparison is equality."""
import numpy as np
import pytest

import multihit_spec as ms


@pytest.fixture(scope="module")
def case(wgt, oracle):
    L, Q, S, T = ms.concentric_scene(wgt)
    o, d = ms.random_rays(4000, np.random.default_rng(0))
    return (L, Q, S, T), o, d, ms.MultiHitSpec(oracle, L, Q, S, T, o, d)


def test_first_entry_is_the_closest_hit(case, oracle):
    (L, Q, S, T), o, d, spec = case
    assert len(T) == 504 and spec.P == len(L) + len(Q) + 504 + len(S)
    prim, dist = oracle.OracleScene(L, Q, S, T).trace(o, d)
    a = spec.answer(2)
    hit = prim != ms.NO_HIT
    assert np.count_nonzero(hit) >= 3000
    assert np.array_equal(a["count"] > 0, hit)
    assert np.array_equal(a["dist"][hit, 0].view(np.uint32), dist[hit].view(np.uint32))
    assert np.array_equal(a["prim"][hit, 0], prim[hit])
    assert (a["prim"][~hit] == ms.NO_HIT).all() and np.isinf(a["dist"][~hit]).all()
    print(f"hits {np.count_nonzero(hit)}, counts {a['count'].min()}..{a['count'].max()}")
    assert a["count"].min() == 0 and a["count"].max() >= 8


def test_order_ties_and_padding(case):
    _, _, _, spec = case
    a = spec.answer(32)
    n = np.arange(32)[None, :]
    have = n < a["count"][:, None]
    assert a["count"].max() < 32
    assert (a["prim"][~have] == ms.NO_HIT).all() and np.isinf(a["dist"][~have]).all()
    d0, d1, p0, p1 = a["dist"][:, :-1], a["dist"][:, 1:], a["prim"][:, :-1], a["prim"][:, 1:]
    both = have[:, 1:]
    assert ((d0 < d1) | ((d0 == d1) & (p0 < p1)))[both].all()
    assert np.count_nonzero(((d0 == d1) & both).any(1)) >= 20  # rays with a distance tie
    # a shorter list is a prefix; a limit and the triangle filter select a subset in the same order
    assert np.array_equal(spec.answer(4)["prim"], a["prim"][:, :4])
    t = spec.answer(32, max_dist=200.0, tris_only=True)
    keep = have & (a["dist"] < np.float32(200.0)) & (a["prim"] >= spec.n_lq) & (a["prim"] < spec.n_lq + spec.n_tris)
    assert np.array_equal(t["count"], keep.sum(1))
    for i in np.flatnonzero(t["count"])[:200]:
        assert np.array_equal(t["prim"][i, :t["count"][i]], a["prim"][i][keep[i]])
    for m in (0.0, -1.0, np.nan):
        assert not spec.answer(1, max_dist=m)["count"].any()


def test_peeling_one_level(case, oracle):
    """50 rays with at least two hits: the second entry is the closest hit without the first primitive."""
    (L, Q, S, T), o, d, spec = case
    a = spec.answer(2)
    rays = np.flatnonzero(a["count"] >= 2)[:50]
    assert len(rays) == 50
    sizes = np.cumsum([0, len(L), len(Q), len(T), len(S)])
    for i in rays:
        first = int(a["prim"][i, 0])
        which = int(np.searchsorted(sizes, first, side="right")) - 1
        parts = [L, Q, T, S]
        parts[which] = np.delete(parts[which], first - sizes[which])
        prim, dist = oracle.OracleScene(parts[0], parts[1], parts[3], parts[2]).trace(o[i:i + 1], d[i:i + 1])
        want = int(a["prim"][i, 1])
        assert int(prim[0]) == want - (1 if want > first else 0), (i, first, want, prim[0])
        assert dist[0].view(np.uint32) == a["dist"][i, 1].view(np.uint32)


def test_non_finite_rays_have_no_hits(case, oracle):
    (L, Q, S, T), o, d, _ = case
    o2, d2 = o[:4].copy(), d[:4].copy()
    o2[0, 1] = np.nan
    d2[1, 2] = np.inf
    o2[2, 0] = -np.inf
    a = ms.MultiHitSpec(oracle, L, Q, S, T, o2, d2).answer(3)
    assert not a["count"][:3].any() and (a["prim"][:3] == ms.NO_HIT).all() and a["count"][3] > 0
