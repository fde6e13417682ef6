"""Self-intersection queries on the resident BVH (wgt_overlap_self and its forms) against their definition:
every requested field equals wgt_overlap_self_spec (the host brute force over the shared arithmetic of
wgt_overlap_self.h) on the triangles that are resident, bit for bit, on every mesh of
tests/self_overlap_cases.py, with and without its index buffer, through the synchronous, the async and the
counting form, in the full form, with hit alone (the traversal ends at the first member), with count alone
and with prim alone.  No tolerance, no excluded triangle.
"""
import numpy as np
import pytest

import overlap_self_restatement as srs
import self_overlap_cases as sc

pytestmark = pytest.mark.gpu

NO_HIT = np.uint32(0xFFFFFFFF)
FIELDS = ("hit", "count", "prim")
FORMS = (FIELDS, ("hit",), ("count",), ("prim",))
KS = (0, 1, 32)


def assert_same(got, want, what, fields=FIELDS):
    for f in fields:
        g, w = got[f], want[f]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
        assert bad.size == 0, (f"{what}: {f} differs at {bad.size} of {len(g)} triangles; first {bad[0]}: got {g[bad[0]]!r}, "
                               f"the definition gives {w[bad[0]]!r}")


def first_prim(ctx):
    info = ctx.scene_info()
    return info["n_lights"] + info["n_quads"]


def upload(ctx, wgt, T, walls=False):
    """The mesh with the reference light and dummy sphere; walls: the Cornell box's quads too."""
    L, Q, S = wgt.cornell_scene()
    ctx.upload_scene(L, Q if walls else Q[:0], S, T)


def _dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _dev_outputs(n, k, fill=0x5A):
    """Device buffers of the three fields, every byte `fill`."""
    import torch

    dev = torch.device("cuda", 0)
    size = {"hit": n, "count": 4 * n, "prim": 4 * n * k}
    return {f: torch.full((max(size[f], 1),), fill, dtype=torch.uint8, device=dev) for f in FIELDS}


def _host_outputs(d, n, k):
    out = {}
    for f, t in d.items():
        a = t.cpu().numpy().copy()
        out[f] = (a[:n] != 0 if f == "hit" else a[:4 * n].view(np.uint32) if f == "count"
                  else np.ascontiguousarray(a[:4 * n * k].view(np.uint32).reshape(k, n).T))
        if f == "hit":
            assert set(np.unique(a[:n])) <= {0, 1}
    return out


def check(ctx, wgt, T, labels, what, ks=KS, device_forms=True):
    """Every form of the query at every k, with `labels` and without, against the definition on T, which is
    resident: the synchronous form, and on device buffers pre-filled with 0x5A the async form on a stream of
    its own and the counting form (every asked field fully written, the others untouched).  A form takes
    k > 0 iff it asks for prim; the other pairings are refused, by name.  -> the definition's with labels at
    the largest k, and the counting form's (node visits, triangle tests) there."""
    import torch

    n, fp = len(T), first_prim(ctx)
    assert ctx.scene_info()["n_tris"] == n
    stream = ctx.pipeline_stream(1)
    counts = None
    for idx in (labels, None):
        d_idx = _dev(idx.view(np.int32)) if idx is not None and device_forms else None  # the labels' bits
        for k in ks:
            for form in FORMS:
                tag = f"{what}, {'indexed' if idx is not None else 'unindexed'}, k = {k}, {form}"
                if (k > 0) != ("prim" in form):
                    with pytest.raises(wgt.tracer.WgtError, match="k == 0" if k == 0 else "k > 0 without prim"):
                        ctx.overlap_self(idx, k, want=form)
                    continue
                want = wgt.overlap_self_spec(T, idx, k, first_prim=fp, want=form)
                got = ctx.overlap_self(idx, k, want=form)
                assert list(got) == list(form)
                assert_same(got, want, tag, fields=form)
                if not device_forms:
                    continue
                ip = d_idx.data_ptr() if d_idx is not None else 0
                out = _dev_outputs(n, k)
                ctx.overlap_self_async(ip, k, stream=stream, **{f: out[f].data_ptr() for f in form})
                torch.cuda.synchronize()
                assert_same(_host_outputs({f: out[f] for f in form}, n, k), want, "async, " + tag, fields=form)
                assert all(bool((out[f] == 0x5A).all()) for f in FIELDS if f not in form), tag
                out = _dev_outputs(n, k)
                nodes, tests = ctx.overlap_self_stats(ip, k, **{f: out[f].data_ptr() for f in form})
                assert_same(_host_outputs({f: out[f] for f in form}, n, k), want, "counting, " + tag, fields=form)
                assert all(bool((out[f] == 0x5A).all()) for f in FIELDS if f not in form), tag
                assert nodes >= n and tests > 0, tag  # every lane visits the root
                if idx is not None and k == max(ks) and form == FIELDS:
                    counts = (nodes, tests)
    full = wgt.overlap_self_spec(T, labels, max(ks), first_prim=fp, want=FIELDS if max(ks) else FIELDS[:2])
    return full, counts


@pytest.mark.parametrize("name", sc.NAMES)
def test_every_mesh(ctx, wgt, name):
    """1. Each mesh of self_overlap_cases: all three entry forms, k = 0, 1, 32, each subset of the fields, with
    and without indices."""
    T = sc.records(name)
    upload(ctx, wgt, T)
    want, counts = check(ctx, wgt, T, sc.labels(name), name)
    print(f"{name}: {len(T)} triangles, {np.count_nonzero(want['count'])} cut something, {counts[0] / len(T):.1f} node visits "
          f"and {counts[1] / len(T):.1f} triangle tests per triangle")
    if name == "grid":
        assert not want["hit"].any()
        bare = ctx.overlap_self(None, 0, want=("count",))["count"]
        assert (bare[sc.grid_interior()] > 0).all()  # what the index buffer removes
    if name == "forty_through_one":
        others = np.array([i for i in range(41) if i != sc.BIG], np.uint32)
        assert want["count"][sc.BIG] == 40 and np.array_equal(want["prim"][sc.BIG], first_prim(ctx) + others[:32])
    if name == "crumpled":
        # the tree culls: far fewer triangle tests than the brute force's n^2
        assert len(T) == 200 and counts[1] < len(T) ** 2, counts


def test_the_mesh_moves(ctx, wgt):
    """2. One context through update_triangles (the fold opened: the pairs disappear) and rebuild_triangles to a
    different count: after each the answers equal the definition on the new triangles, ids unchanged."""
    T, L = sc.records("strip_folded"), sc.labels("strip_folded")
    upload(ctx, wgt, T)
    before, _ = check(ctx, wgt, T, L, "folded", ks=(32,), device_forms=False)
    assert set(np.flatnonzero(before["hit"])) == {3, 10, 11}
    opened = wgt.make_triangles(sc.strip_opened()[0])
    ctx.update_triangles(opened)
    after, _ = check(ctx, wgt, opened, L, "opened")
    assert not after["hit"].any() and (after["prim"] == NO_HIT).all()
    ctx.update_triangles(T)
    again, _ = check(ctx, wgt, T, L, "folded again", ks=(32,), device_forms=False)
    assert np.array_equal(again["prim"], before["prim"])
    big = sc.records("crumpled")
    ctx.rebuild_triangles(big)
    assert ctx.scene_info()["n_tris"] == 200
    want, _ = check(ctx, wgt, big, sc.labels("crumpled"), "rebuilt to 200 triangles")
    assert want["hit"].any()
    with pytest.raises(ValueError, match="3 per triangle"):
        ctx.overlap_self(L, 0, want=("hit",))  # the strip's 14 triangles of labels no longer fit


def test_ids_are_offset_by_the_lights_and_quads(ctx, wgt):
    """3. The two sheets inside the Cornell box, with its light, its quads and the sphere: prim holds
    n_lights + n_quads + id, and nothing but triangles is searched."""
    T, L = sc.records("two_grids"), sc.labels("two_grids")
    upload(ctx, wgt, T, walls=True)
    fp = first_prim(ctx)
    assert fp > 1 and ctx.scene_info()["n_spheres"] == 1
    want, _ = check(ctx, wgt, T, L, "two sheets in the box")
    listed = want["prim"][want["prim"] != NO_HIT]
    assert listed.size and listed.min() >= fp and listed.max() < fp + len(T)
    assert np.array_equal(want["prim"][:, 0] != NO_HIT, srs.matrix(T, L).any(1))


def test_refusals_and_a_scene_without_triangles(ctx, wgt):
    """4. The Python refusals, as the overlap query's; a scene without triangles is answered with empty arrays
    and nothing is written through the device forms."""
    import torch

    upload(ctx, wgt, sc.records("crossing"))
    with pytest.raises(wgt.tracer.WgtError, match="k > 0 without prim"):
        ctx.overlap_self(None, 4, want=("hit", "count"))
    with pytest.raises(wgt.tracer.WgtError, match="k == 0"):
        ctx.overlap_self(None, 0)
    with pytest.raises(wgt.tracer.WgtError, match="k out of range"):
        ctx.overlap_self(None, 33)
    with pytest.raises(wgt.tracer.WgtError, match="no overlap field"):
        ctx.overlap_self_async(0, 0)
    with pytest.raises(ValueError):
        ctx.overlap_self(None, 1, want=("prim", "dist"))
    L, Q, S = wgt.cornell_scene()
    ctx.upload_scene(L, Q, S)
    got = ctx.overlap_self(None, 4)
    assert [got[f].shape for f in FIELDS] == [(0,), (0,), (0, 4)]
    out = _dev_outputs(4, 1)
    ctx.overlap_self_async(0, 1, **{f: out[f].data_ptr() for f in FIELDS})
    assert ctx.overlap_self_stats(0, 1, **{f: out[f].data_ptr() for f in FIELDS}) == (0, 0)
    torch.cuda.synchronize()
    assert all(bool((out[f] == 0x5A).all()) for f in FIELDS)


@pytest.mark.parametrize("name", sc.NAMES)
def test_self_intersections(ctx, wgt, name):
    """5. Context.self_intersections returns exactly the definition's pairs, s < t in lexicographic order, and
    says truncated only where a triangle cuts more than k others: the forty crossings."""
    T, L = sc.records(name), sc.labels(name)
    upload(ctx, wgt, T)
    pairs, truncated = ctx.self_intersections(L)
    want = srs.pairs(srs.matrix(T, L))  # the spec's membership (tests/test_overlap_self_restatement.py)
    assert pairs.dtype == np.int64 and pairs.shape == want.shape and np.array_equal(pairs, want), name
    assert truncated == (name == "forty_through_one")
    if name == "forty_through_one":
        assert len(pairs) == 40  # every pair is still there: each small triangle lists the large one
    few, cut = ctx.self_intersections(L, k=1)
    assert cut == bool((srs.matrix(T, L).sum(1) > 1).any()) and set(map(tuple, few)) <= set(map(tuple, want))
