"""Triangle overlap queries on the resident BVH (wgt_overlap_triangles and its forms) against their definition:
every requested field equals wgt_overlap_triangles_spec (the host brute force over the shared arithmetic of
wgt_overlap.h) on the triangles that are resident, bit for bit, in the full form, with hit alone (the traversal
ends at the first overlapping triangle), with count alone and with prim alone.  No tolerance, no excluded query.
The overlap kernel reads the 128-B nodes at every scene size, as the closest-point kernels do, so there is no
compact-node form to cover.
"""
import numpy as np
import pytest

import adversarial_meshes as am
import nearest_cases as nc
import overlap_cases as oc
import overlap_restatement as rs
import refit_cases as rc

pytestmark = pytest.mark.gpu

f32 = np.float32
NO_HIT = np.uint32(0xFFFFFFFF)
FIELDS = ("hit", "count", "prim")
FORMS = (FIELDS, ("hit",), ("count",), ("prim",))


def assert_same(got, want, what, fields=FIELDS):
    for f in fields:
        g, w = got[f], want[f]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.shape, w.shape)
        bad = np.flatnonzero((g != w).reshape(len(g), -1).any(1))
        assert bad.size == 0, (f"{what}: {f} differs at {bad.size} of {len(g)} queries; first {bad[0]}: got {g[bad[0]]!r}, "
                               f"the definition gives {w[bad[0]]!r}")


def resident(ctx):
    """The resident triangles in original order (v0, e1, e2 of wgt_bvh_read's records)."""
    import webgputracer_amd as wgt

    recs = ctx.bvh_read()[1]
    T = np.zeros(len(recs), wgt.tracer.TRI_DTYPE)
    idx = np.ascontiguousarray(recs[:, 0, 3]).view(np.uint32).astype(np.int64)
    assert np.array_equal(np.sort(idx), np.arange(len(recs)))
    for k, row in (("v0", 0), ("e1", 1), ("e2", 2)):
        T[k][idx, :3] = recs[:, row, :3]
    return T


def first_prim(ctx):
    info = ctx.scene_info()
    return info["n_lights"] + info["n_quads"]


def check(ctx, wgt, Q, what, ks=oc.KS, tris=None):
    """Every form of the query on Q at every k against the definition on the resident triangles.  A form takes
    k > 0 iff it asks for prim; the other pairings are refused, by name.  -> the definition's at the largest k."""
    T = resident(ctx) if tris is None else tris
    fp = first_prim(ctx)
    for k in ks:
        for form in FORMS:
            if (k > 0) != ("prim" in form):
                with pytest.raises(wgt.tracer.WgtError, match="k == 0" if k == 0 else "k > 0 without prim"):
                    ctx.overlap_triangles(Q, k, want=form)
                continue
            want = wgt.overlap_triangles_spec(T, Q, k, first_prim=fp, want=form)
            got = ctx.overlap_triangles(Q, k, want=form)
            assert list(got) == list(form)
            assert_same(got, want, f"{what}, k = {k}, {form}", fields=form)
    return wgt.overlap_triangles_spec(T, Q, max(ks), first_prim=fp, want=FIELDS if max(ks) else FIELDS[:2])


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


def upload_bunny(ctx):
    L, Q, S, T = nc.bunny_scene()
    ctx.upload_scene(L, Q, S, T)
    return T


def test_main_cases(ctx, wgt):
    """1. The Cornell walls plus bunny2000 and 512 queries made from its own triangles, at k = 0, 1, 8, 32 in
    the full form, with hit alone, count alone and prim alone."""
    T = upload_bunny(ctx)
    want = check(ctx, wgt, oc.bunny_queries(), "bunny", tris=T)
    full = wgt.overlap_triangles_spec(T, oc.bunny_queries(), 32, first_prim=first_prim(ctx))
    assert np.array_equal(want["prim"], full["prim"])
    assert np.count_nonzero(full["count"]) > 256 and (full["prim"][full["hit"], 0] >= first_prim(ctx)).all()


@pytest.mark.parametrize("n", [1, 63, 65])
def test_launch_edges(ctx, wgt, n):
    """2. A partial workgroup, and a second one."""
    T = upload_bunny(ctx)
    check(ctx, wgt, oc.bunny_queries()[:n], f"n = {n}", ks=(0, 8), tris=T)
    assert ctx.overlap_triangles(np.zeros((0, 3, 3), f32), 8)["prim"].shape == (0, 8)


def test_device_pointer_entries(ctx, wgt):
    """3. The async call on device buffers pre-filled with 0x5A, on a non-default stream: every asked field
    is fully written, a null field's buffer is untouched; the counting kernel gives the same answers and
    non-zero counters."""
    import torch

    T = upload_bunny(ctx)
    Q = oc.bunny_queries()
    n = len(Q)
    dQ = _dev(Q.reshape(n, 9).T)
    s = ctx.pipeline_stream(1)
    for form in FORMS:
        k = 8 if "prim" in form else 0
        want = wgt.overlap_triangles_spec(T, Q, k, first_prim=first_prim(ctx), want=form)
        out = _dev_outputs(n, k)
        ctx.overlap_triangles_async(dQ.data_ptr(), n, k, stream=s, **{f: out[f].data_ptr() for f in form})
        torch.cuda.synchronize()
        assert_same(_host_outputs({f: out[f] for f in form}, n, k), want, f"async, {form}", fields=form)
        for f in FIELDS:
            if f not in form:
                assert bool((out[f] == 0x5A).all()), (form, f)
        out = _dev_outputs(n, k)
        nodes, tests = ctx.overlap_triangles_stats(dQ.data_ptr(), n, k, **{f: out[f].data_ptr() for f in form})
        assert_same(_host_outputs({f: out[f] for f in form}, n, k), want, f"counting, {form}", fields=form)
        for f in FIELDS:
            if f not in form:
                assert bool((out[f] == 0x5A).all()), (form, f)
        print(f"{form}: {nodes / n:.1f} node visits and {tests / n:.1f} triangle tests per query of {len(T)} triangles")
        assert nodes >= n and 0 < tests < n * len(T)


def test_the_mesh_moves(ctx, wgt):
    """4. One context through update_triangles, a rebuild to a different count and a refit of the rebuilt
    tree: after each the answers equal the definition on the triangles wgt_bvh_read returns."""
    L, Q, S, _ = nc.bunny_scene()
    A = rc.mesh("bunny2000")
    ctx.upload_scene(L, Q, S, A)
    queries = oc.bunny_queries()
    before = check(ctx, wgt, queries, "upload", ks=(8,))
    B = rc.moved("bunny2000", "jitter5")
    ctx.update_triangles(B)
    T = resident(ctx)
    assert np.array_equal(T["v0"][:, :3].view(np.uint32), B["v0"][:, :3].view(np.uint32))
    after = check(ctx, wgt, queries, "update_triangles", ks=(0, 8), tris=T)
    assert not np.array_equal(before["prim"], after["prim"])  # the update matters
    ctx.rebuild_triangles(A[::4])
    assert ctx.scene_info()["n_tris"] == len(A[::4])
    check(ctx, wgt, queries, "rebuild to a different count", ks=(0, 8, 32))
    moved = A[::4].copy()
    moved["v0"][:, :3] += np.random.default_rng(5).normal(0.0, 3.0, (len(moved), 3)).astype(f32)
    ctx.update_triangles(moved)
    check(ctx, wgt, queries, "refit of the rebuilt tree", ks=(0, 8))


def test_scenes_at_the_limits(ctx, wgt):
    """5. No triangles (the Cornell box alone): all answers empty.  Meshes of 1, 3 and 9 triangles: empty
    node slots, and a leaf of eight plus one."""
    L, Q, S, T = nc.bunny_scene()
    queries = oc.bunny_queries()[:128]
    ctx.upload_scene(L, Q, S)
    got = ctx.overlap_triangles(queries, 4)
    assert not got["hit"].any() and not got["count"].any() and (got["prim"] == NO_HIT).all()
    assert not ctx.overlap_triangles(queries, 0, want=("hit",))["hit"].any()
    live = np.flatnonzero(np.linalg.norm(np.cross(T["e1"][:, :3].astype(np.float64), T["e2"][:, :3].astype(np.float64)), axis=1) > 0)
    for m in (1, 3, 9):
        mesh = T[live[100:100 + m]]
        ctx.upload_scene(L, Q, S, mesh)
        if m == 1:
            assert ctx.scene_info()["bvh_nodes"] == 1
        own = np.concatenate([oc.from_own_triangles(mesh, 96, 37 + m), queries[:32]])
        want = check(ctx, wgt, own, f"{m} triangles", ks=(0, 1, 32))
        assert want["hit"].any() and (want["count"] <= m).all()


def test_the_list_overflows(ctx, wgt):
    """6. 64 exact copies of one triangle at k = 32: count 64, the 32 lowest ids."""
    L, Q, S, _ = nc.bunny_scene()
    ctx.upload_scene(L, Q, S, nc.copies64())
    queries = np.concatenate([oc.through_copies64(), oc.from_own_triangles(nc.copies64(), 125, 41)])
    want = check(ctx, wgt, queries, "64 copies", ks=(0, 1, 8, 32))
    fp = first_prim(ctx)
    assert list(want["count"][:3]) == [64, 64, 0] and set(np.unique(want["count"])) <= {0, 64}
    assert (want["prim"][:2] == fp + np.arange(32, dtype=np.uint32)).all()


@pytest.mark.parametrize("name", am.GPU)
def test_hard_meshes(ctx, wgt, name):
    """7. The meshes that reach the builder's depth limit and the stack bound, duplicated and degenerate
    triangles among them, with queries made from their own triangles."""
    L, Q, S = am.scene_parts(name)
    T = am.small_mesh(name)
    ctx.upload_scene(L, Q, S, T)
    queries = np.concatenate([oc.from_own_triangles(T, 384, 43), oc.corners(T)[:64], oc.zero_area_queries(T)])
    want = check(ctx, wgt, queries, name, ks=(0, 8, 32))
    assert want["hit"].any()


def test_invalid_queries_between_valid_ones(ctx, wgt):
    """8. A NaN, an infinity, a coordinate of 2^41 and an edge component of 2^31 in every fourth lane of the
    waves: those answers are empty, their neighbours' are not disturbed."""
    T = upload_bunny(ctx)
    queries, odd = oc.interleaved(oc.bunny_queries())
    want = check(ctx, wgt, queries, "interleaved", ks=(0, 8), tris=T)
    assert odd.sum() == 128 and not want["count"][odd].any() and (want["prim"][odd] == NO_HIT).all()
    clean = wgt.overlap_triangles_spec(T, oc.bunny_queries(), 8, first_prim=first_prim(ctx))
    assert np.array_equal(want["prim"][~odd], clean["prim"][~odd])


def test_bunny_against_a_shifted_copy(ctx, wgt):
    """9. End to end: the bunny's own triangles, moved by (7, 3, 5), as queries against the bunny.  The pairs
    the GPU reports, unioned over the queries, equal the pairs the float64 restatement finds, both restricted
    to the pairs that are not marginal (a float64 margin of at least 1e-4, overlap_restatement.margins)."""
    T = upload_bunny(ctx)
    fp = first_prim(ctx)
    queries = (oc.corners(T)[::4] + np.array([7.0, 3.0, 5.0], f32)).astype(f32)
    got = ctx.overlap_triangles(queries, 32)
    assert got["count"].max() <= 32  # the lists are complete
    rec = tuple(np.ascontiguousarray(T[f][:, :3]) for f in ("v0", "e1", "e2"))
    reported = np.zeros((len(queries), len(T)), bool)
    rows, cols = np.nonzero(got["prim"] != NO_HIT)
    reported[rows, got["prim"][rows, cols] - fp] = True
    d64 = np.stack([rs.tri_overlap(q, *rec, dtype=np.float64) for q in queries])
    firm = np.stack([rs.margins(q, *rec) for q in queries]) >= 1e-4
    print(f"{reported.sum()} pairs reported, {d64.sum()} in float64, {(d64 & ~firm).sum()} of those marginal")
    assert (d64 & firm).sum() >= 64 and np.array_equal(reported & firm, d64 & firm)
    assert np.array_equal(got["hit"], got["count"] > 0) and np.array_equal(got["count"], reported.sum(1))
