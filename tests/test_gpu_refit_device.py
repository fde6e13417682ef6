"""wgt_update_triangles_device and wgt_update_vertices_device: the refit from device memory.

Both must leave exactly what wgt_update_triangles(T) leaves, bit for bit, where T is the record
input's bytes, or for the vertex form what make_triangles builds from each triangle's gathered
vertices with the colour and emissive flag the triangle was uploaded with.  So the trees are compared
with the host specification (wgt_bvh_refit) and frames and queries with a second context's fresh
upload of T.  Inputs are torch tensors on the device; no test passes a pointer the device cannot
read.  Meshes and motions: tests/refit_cases.py; scenes, camera and rays: tests/test_gpu_refit.py.
"""
import functools

import numpy as np
import pytest

import hit_records as hr
import refit_cases as rc
import test_gpu_refit as host_form  # its scenes, camera and rays, not its tests

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def fresh(wgt):
    """A second context: the host-form updates and fresh uploads the device forms are compared with."""
    c = wgt.Context(0)
    yield c
    c.close()


def _dev(a):
    """A host array's bytes as a resident torch tensor (uint32 as int32: same bytes)."""
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = a.view(np.uint8)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(a.copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _host(t):
    return t.cpu().numpy().view(np.uint8).copy()


def _verts32(tris):
    """(n, 3, 3) float32 vertices of the triangles."""
    return rc.vertices(tris).astype(f32)


@functools.lru_cache(maxsize=None)
def _shaded(name):
    """Mesh A with a random colour per triangle and every 7th triangle emissive."""
    A = rc.mesh(name).copy()
    rng = np.random.default_rng(len(A))
    A["col"] = rng.uniform(0.1, 0.9, (len(A), 3)).astype(f32)
    A["emissive"] = (np.arange(len(A)) % 7 == 3).astype(f32)
    return A


def _records_of(wgt, V, shaded):
    """The host specification of the vertex form: make_triangles of the vertices, each triangle with
    the colour and emissive flag it was uploaded with."""
    T = wgt.make_triangles(V)
    T["col"] = shaded["col"]
    T["emissive"] = shaded["emissive"]
    return T


@functools.lru_cache(maxsize=None)
def _vertex_case(name, motion):
    """(A with shading, V of B as float32, T = the records the vertex form must build)."""
    import webgputracer_amd as wgt

    A = _shaded(name)
    V = _verts32(rc.moved(name, motion))
    return A, V, _records_of(wgt, V, A)


_refit_cache = {}


def _want_tree(wgt, key, A, T):
    """wgt_bvh_refit(A, T) without the info, computed once per key."""
    if key not in _refit_cache:
        _refit_cache[key] = wgt.bvh_refit(A, T)[1:]
    return _refit_cache[key]


def _indexed(V, seed):
    """Unique vertex rows of V (by bits) in a random order, and the (n, 3) index array onto them."""
    rows = rc.bits(V.reshape(-1, 3))
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    perm = np.random.default_rng(seed).permutation(len(uniq))
    where = np.empty(len(uniq), np.int64)
    where[perm] = np.arange(len(uniq))
    verts = np.ascontiguousarray(uniq[perm]).view(f32)
    index = where[np.asarray(inv).reshape(-1)].astype(np.uint32).reshape(-1, 3)
    assert np.array_equal(rc.bits(verts[index]), rc.bits(V))
    return verts, index


def _refused(ctx, call, code, *words):
    """The raw call returns `code`, the context's error holds every word, and nothing was raised."""
    from webgputracer_amd import _lib

    rcode = call(_lib.lib())
    msg = (_lib.lib().wgt_last_error(ctx.h) or b"").decode()
    assert rcode == code, (rcode, msg)
    for w in words:
        assert w in msg, (w, msg)


def _raw_records(ctx, ptr, n, stream=None):
    return lambda L: L.wgt_update_triangles_device(ctx.h, ptr or None, n, stream)


def _raw_verts(ctx, ptr, n_verts, n, index=None, stream=None):
    return lambda L: L.wgt_update_vertices_device(ctx.h, ptr or None, n_verts, index or None, n, stream)


def _same_info(ctx, fresh, L, Q, S, A, T):
    """The scene report equals what the host form leaves after upload(A), update(T)."""
    fresh.upload_scene(L, Q, S, A)
    fresh.update_triangles(T)
    assert ctx.scene_info() == fresh.scene_info()


def _record_form_case(ctx, fresh, wgt, A, B, key):
    """Test 1 on one (A, B): upload A in the tiny scene, device-update to B's records."""
    from webgputracer_amd import _lib

    L, Q, S = host_form._tiny_scene(wgt)
    ctx.upload_scene(L, Q, S, A)
    d = _dev(B)
    if not rc.within_limits(B):
        before = ctx.bvh_read()
        _refused(ctx, _raw_records(ctx, d.data_ptr(), len(B)), _lib.WGT_E_INVALID, "triangle")
        rc.assert_trees_equal(ctx.bvh_read(), before, what=f"{key} refused")
        return
    ctx.update_triangles_device(d.data_ptr(), len(B))
    rc.assert_trees_equal(ctx.bvh_read(), _want_tree(wgt, key, A, B), what=str(key))
    _same_info(ctx, fresh, L, Q, S, A, B)


def _vertex_form_case(ctx, fresh, wgt, A, V, T, key, index=None):
    """Test 3 on one (A, V): upload A in the tiny scene, device-update to the vertices (unindexed, or
    verts = V's unique rows with `index`); the tree is wgt_bvh_refit(A, T)."""
    from webgputracer_amd import _lib

    L, Q, S = host_form._tiny_scene(wgt)
    ctx.upload_scene(L, Q, S, A)
    dv = _dev(V)
    di = _dev(index) if index is not None else None
    n_verts = dv.numel() // 3
    if not rc.within_limits(T):
        before = ctx.bvh_read()
        _refused(ctx, _raw_verts(ctx, dv.data_ptr(), n_verts, len(A), di.data_ptr() if di is not None else None),
                 _lib.WGT_E_INVALID, "triangle")
        rc.assert_trees_equal(ctx.bvh_read(), before, what=f"{key} refused")
        return
    ctx.update_vertices_device(dv.data_ptr(), n_verts, len(A), d_index=di.data_ptr() if di is not None else 0)
    rc.assert_trees_equal(ctx.bvh_read(), _want_tree(wgt, key, A, T), what=str(key))
    _same_info(ctx, fresh, L, Q, S, A, T)


@pytest.mark.parametrize("motion", rc.MOTIONS)
@pytest.mark.parametrize("name", rc.MESHES)
def test_record_form_tree_equals_host_refit(ctx, fresh, wgt, name, motion):
    """1. upload(A), device update to B's records: wgt_bvh_refit(A, B) bit for bit, the host form's scene
    report; beyond the limits a refusal that names a triangle and leaves the tree."""
    _record_form_case(ctx, fresh, wgt, rc.mesh(name), rc.moved(name, motion), ("rec", name, motion))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_block_edges(ctx, fresh, wgt, n):
    """2. The first n triangles of bunny2000 under jitter5, around the 256-lane block: a tail lane or a
    reduction over a partial wave can go wrong here.  Both input forms."""
    A, B = rc.mesh("bunny2000")[:n].copy(), rc.moved("bunny2000", "jitter5")[:n].copy()
    _record_form_case(ctx, fresh, wgt, A, B, ("rec", "bunny", n))
    V = _verts32(B)
    _vertex_form_case(ctx, fresh, wgt, A, V, _records_of(wgt, V, A), ("vert", "bunny", n))


@pytest.mark.parametrize("motion", rc.MOTIONS)
@pytest.mark.parametrize("name", rc.MESHES)
def test_vertex_form_tree_equals_host_refit(ctx, fresh, wgt, name, motion):
    """3. upload(A with colours and emissive triangles), device update to B's vertices, unindexed: the tree
    of wgt_bvh_refit(A, make_triangles(V)) bit for bit, or the refusal."""
    A, V, T = _vertex_case(name, motion)
    _vertex_form_case(ctx, fresh, wgt, A, V, T, ("vert", name, motion))


def test_negative_zero_coordinates_become_positive_zero(ctx, fresh, wgt):
    """3b. make_triangles adds a zero translation, so a -0 coordinate becomes +0; the device does too."""
    A = _shaded("nine")
    V = _verts32(rc.moved("nine", "jitter5"))
    V[0, 0, 0] = -0.0  # one coordinate of a v0
    V[3, :, 1] = -0.0  # a whole triangle in the plane y = -0
    V[5, 2, :] = -0.0  # a vertex at the origin, all signs set
    T = _records_of(wgt, V, A)
    assert np.signbit(V).sum() >= 7 and rc.bits(T["v0"][0, 0]) == 0 and rc.bits(T["v0"][3, 1]) == 0
    _vertex_form_case(ctx, fresh, wgt, A, V, T, ("vert", "nine", "minus zero"))
    recs = ctx.bvh_read()[1]
    by_index = {int(i): r for i, r in zip(rc.bits(recs[:, 0, 3]), recs)}
    assert rc.bits(by_index[0][0, 0]) == 0 and rc.bits(by_index[3][0, 1]) == 0


@pytest.mark.parametrize("name,motion", [("bunny2000", "jitter5"), ("nine", "translate1000"), ("one", "scale8")])
def test_indexed_vertex_form(ctx, fresh, wgt, name, motion):
    """4. V's unique vertex rows, permuted, with an index array onto them: the tree of test 3.  A
    repeated index (a degenerate triangle) equals the unindexed form on the same gathered vertices."""
    A, V, T = _vertex_case(name, motion)
    verts, index = _indexed(V, 4)
    _vertex_form_case(ctx, fresh, wgt, A, verts, T, ("vert", name, motion), index=index)
    index2 = index.copy()
    index2[len(index2) // 2, 1] = index2[len(index2) // 2, 0]
    V2 = np.ascontiguousarray(verts[index2])
    T2 = _records_of(wgt, V2, A)
    _vertex_form_case(ctx, fresh, wgt, A, verts, T2, ("vert", name, motion, "repeat"), index=index2)
    indexed_tree = ctx.bvh_read()
    _vertex_form_case(ctx, fresh, wgt, A, V2, T2, ("vert", name, motion, "repeat"))
    rc.assert_trees_equal(ctx.bvh_read(), indexed_tree, what="indexed against unindexed")


def _device_forms(ctx, V, T):
    """(name, update) of the three device input forms of the same triangles T with vertices V."""
    verts, index = _indexed(V, 6)
    dT, dV, dU, dI = _dev(T), _dev(V), _dev(verts), _dev(index)
    return (("records", lambda: ctx.update_triangles_device(dT.data_ptr(), len(T))),
            ("vertices", lambda: ctx.update_vertices_device(dV.data_ptr(), 3 * len(T), len(T))),
            ("indexed", lambda: ctx.update_vertices_device(dU.data_ptr(), len(verts), len(T), d_index=dI.data_ptr())))


@pytest.mark.parametrize("motion", ["jitter5", "translate1000"])
@pytest.mark.parametrize("form", ["default", "WGT_KERNEL=1"])
def test_frames_and_queries_equal_a_fresh_upload(ctx, fresh, wgt, monkeypatch, form, motion):
    """5. After each device form: a 64x64, 4 spp frame (f32 bits, u8, hit ids), 20,000 rays' hit records by
    bytes and their occlusion answers, against a fresh upload of T.  The vertex forms thereby kept
    the colours and emissive flags and wrote the right normals."""
    if form != "default":
        monkeypatch.setenv(*form.split("="))
    A, V, T = _vertex_case("bunny2000", motion)
    L, Q, S = host_form._walls(wgt)
    fresh.upload_scene(L, Q, S, T)
    cam = host_form._camera_at(wgt, T, 1.0, 4, 11)
    want = fresh.render_tile(cam, 64, 64)
    o, d = host_form._query_rays(T, 20_000, 3)
    want_hits = fresh.trace_hits(o, d)
    lim = np.nextafter(want_hits["dist"], f32(np.inf))
    want_occ = fresh.occluded(o, d, lim)
    assert np.array_equal(want_occ, want_hits["prim"] != hr.NO_HIT)
    nlq = len(L) + len(Q)
    ctx.upload_scene(L, Q, S, A)
    for what, update in _device_forms(ctx, V, T):
        ctx.update_triangles(A)  # every form starts from A's geometry, colours and flags
        update()
        got = ctx.render_tile(cam, 64, 64, stats=True)
        tri_px = int(np.sum((got["hit"] >= nlq) & (got["hit"] < nlq + len(T))))
        print(f"{form} {motion} {what}: {tri_px} pixels see the mesh")
        assert tri_px >= 100
        host_form._same_frame(got, want, f"{form} {motion} {what}")
        assert got["stats"]["stack_overflows"] == 0
        hits = ctx.trace_hits(o, d)
        for f in hr.FIELDS:
            assert np.array_equal(hits[f].view(np.uint8), want_hits[f].view(np.uint8)), (what, f)
        assert np.array_equal(ctx.occluded(o, d, lim), want_occ), what


def test_degenerate_input_through_the_vertex_form(ctx, fresh, wgt):
    """6. Every triangle collapsed to a point: the tree, and closest hits against a fresh upload of T.
    Frames are not compared: the face normals are NaN, whose payload is unspecified."""
    A, V, T = _vertex_case("bunny2000", "collapse")
    assert rc.within_limits(T) and np.isnan(T["face_norm"][:, :3]).all()
    _vertex_form_case(ctx, fresh, wgt, A, V, T, ("vert", "bunny2000", "collapse"))
    L, Q, S = host_form._walls(wgt)
    ctx.upload_scene(L, Q, S, A)
    dV = _dev(V)
    ctx.update_vertices_device(dV.data_ptr(), 3 * len(A), len(A))
    fresh.upload_scene(L, Q, S, T)
    o, d = host_form._query_rays(A, 20_000, 8)
    prim, dist = ctx.trace_rays(o, d)
    wprim, wdist = fresh.trace_rays(o, d)
    assert np.array_equal(prim, wprim) and np.array_equal(hr.bits(dist), hr.bits(wdist))


def test_refusals_leave_everything_as_it_was(ctx, wgt):
    """7. Every refusal's status and message; afterwards the tree, a frame and the input's bytes."""
    from webgputracer_amd import _lib

    A = rc.mesh("bunny2000")
    n = len(A)
    V = _verts32(A)
    L, Q, S = host_form._walls(wgt)
    dA, dV = _dev(A), _dev(V)
    with wgt.Context(0) as empty:
        _refused(empty, _raw_records(empty, dA.data_ptr(), n), _lib.WGT_E_NOSCENE, "no scene")
        _refused(empty, _raw_verts(empty, dV.data_ptr(), 3 * n, n), _lib.WGT_E_NOSCENE, "no scene")
    ctx.upload_scene(L, Q, S)
    _refused(ctx, _raw_records(ctx, dA.data_ptr(), n), _lib.WGT_E_INVALID, "no triangles")
    _refused(ctx, _raw_verts(ctx, dV.data_ptr(), 3 * n, n), _lib.WGT_E_INVALID, "no triangles")
    ctx.upload_scene(L, Q, S, A)
    cam = wgt.camera_param(1.0, 1, 9)
    tree, frame = ctx.bvh_read(), ctx.render_tile(cam, 32, 32)

    two, long_edge = A.copy(), A.copy()
    two["v0"][17, 0] = np.nan
    two["v0"][1000, 1] = 2.0 ** 41
    long_edge["e1"][1979, 2] = 2.0 ** 31
    V_two, V_edge = V.copy(), V.copy()
    V_two[17, 0, 0] = np.nan
    V_two[1000, 1, 1] = 2.0 ** 41
    V_edge[5, 0, 0], V_edge[5, 1, 0] = -(2.0 ** 30.5), 2.0 ** 30.5  # both within 2^40, their edge beyond 2^30
    verts, index = _indexed(V, 7)
    index_bad = index.copy()
    index_bad[1979, 2] = len(verts)
    padded = np.concatenate([A.view(np.uint8), np.zeros(16, np.uint8)])  # room behind a pointer offset by 4 bytes
    d_two, d_edge, dV_two, dV_edge = _dev(two), _dev(long_edge), _dev(V_two), _dev(V_edge)
    dU, dI, dI_bad, d_pad = _dev(verts), _dev(index), _dev(index_bad), _dev(padded)
    assert dU.numel() == 3 * len(verts)
    cases = (
        ("null records", _raw_records(ctx, None, n), None, ("null",)),
        ("null vertices", _raw_verts(ctx, None, 3 * n, n), None, ("null",)),
        ("null vertices, indexed", _raw_verts(ctx, None, len(verts), n, dI.data_ptr()), dI, ("null",)),
        ("records, one fewer", _raw_records(ctx, dA.data_ptr(), n - 1), dA, ("count",)),
        ("vertices, one more", _raw_verts(ctx, dV.data_ptr(), 3 * n, n + 1), dV, ("count",)),
        ("records offset by 4 bytes", _raw_records(ctx, d_pad.data_ptr() + 4, n), d_pad, ("misaligned",)),
        ("unindexed n_verts", _raw_verts(ctx, dV.data_ptr(), 3 * n - 1, n), dV, ("vertex count",)),
        ("n_verts 0", _raw_verts(ctx, dU.data_ptr(), 0, n, dI.data_ptr()), dU, ("vertex count",)),
        ("records: NaN in 17, 2^41 in 1000", _raw_records(ctx, d_two.data_ptr(), n), d_two, ("triangle 17:", "2^40")),
        ("vertices: NaN in 17, 2^41 in 1000", _raw_verts(ctx, dV_two.data_ptr(), 3 * n, n), dV_two,
         ("triangle 17:", "2^40")),
        ("records: e1 of 2^31", _raw_records(ctx, d_edge.data_ptr(), n), d_edge, ("triangle 1979:", "2^30")),
        ("vertices: an edge of 2^31.5", _raw_verts(ctx, dV_edge.data_ptr(), 3 * n, n), dV_edge, ("triangle 5:", "2^30")),
        ("index == n_verts", _raw_verts(ctx, dU.data_ptr(), len(verts), n, dI_bad.data_ptr()), dI_bad,
         ("triangle 1979:", "index")),
    )
    for what, call, tensor, words in cases:
        held = _host(tensor) if tensor is not None else None
        _refused(ctx, call, _lib.WGT_E_INVALID, *words)
        rc.assert_trees_equal(ctx.bvh_read(), tree, what=what)
        host_form._same_frame(ctx.render_tile(cam, 32, 32), frame, what)
        if tensor is not None:
            assert np.array_equal(_host(tensor), held), f"{what}: the input was written"
    with pytest.raises(wgt.tracer.WgtError):
        ctx.update_triangles_device(d_two.data_ptr(), n)
    with pytest.raises(wgt.tracer.WgtError):
        ctx.update_vertices_device(dU.data_ptr(), len(verts), n, d_index=dI_bad.data_ptr())
    # and the valid indexed input is accepted, and not written either
    held = _host(dU), _host(dI)
    ctx.update_vertices_device(dU.data_ptr(), len(verts), n, d_index=dI.data_ptr())
    assert np.array_equal(_host(dU), held[0]) and np.array_equal(_host(dI), held[1])


def test_input_is_read_after_work_queued_on_the_stream(ctx, wgt):
    """8a. On a torch stream: large matmuls, then a copy of B into the tensor that holds A, then the
    device update with that stream's handle and no synchronisation: the tree is wgt_bvh_refit(A, B)."""
    import torch

    A, B = rc.mesh("bunny2000"), rc.moved("bunny2000", "jitter5")
    L, Q, S = host_form._tiny_scene(wgt)
    ctx.upload_scene(L, Q, S, A)
    d, dB = _dev(A), _dev(B)
    m = torch.ones((2048, 2048), device=d.device)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=d.device)
    with torch.cuda.stream(s):
        for _ in range(8):
            m = (m @ m) * (1.0 / 2048.0)
        d.copy_(dB, non_blocking=True)
    ctx.update_triangles_device(d.data_ptr(), len(A), stream=s.cuda_stream)
    rc.assert_trees_equal(ctx.bvh_read(), _want_tree(wgt, ("rec", "bunny2000", "jitter5"), A, B), what="after the copy")
    torch.cuda.synchronize()
    assert float(m[0, 0]) == 1.0
    # the vertex form the same way, back to A
    V_A, V_B = _verts32(A), _verts32(B)
    dv, dVA = _dev(V_B), _dev(V_A)
    with torch.cuda.stream(s):
        for _ in range(8):
            m = (m @ m) * (1.0 / 2048.0)
        dv.copy_(dVA, non_blocking=True)
    ctx.update_vertices_device(dv.data_ptr(), 3 * len(A), len(A), stream=s.cuda_stream)
    T_A = _records_of(wgt, V_A, A)
    rc.assert_trees_equal(ctx.bvh_read(), _want_tree(wgt, ("vert", "bunny2000", "to A"), A, T_A), what="vertices")
    torch.cuda.synchronize()


def test_device_update_is_ordered_after_queued_frames(ctx, fresh, wgt):
    """8b. Two frames queued on pipeline streams 0 and 1, then a device update without synchronising, then
    a third frame: the first two show A, the third B."""
    import torch

    from webgputracer_amd._lib import TILE_DTYPE

    A, B = rc.mesh("bunny2000"), rc.moved("bunny2000", "jitter5")
    L, Q, S = host_form._walls(wgt)
    W, H, spp = 64, 64, 64
    dev = torch.device("cuda", 0)
    ctx.upload_scene(L, Q, S, A)
    streams = [ctx.pipeline_stream(0), ctx.pipeline_stream(1), ctx.pipeline_stream(0)]
    outs, tiles = [], []
    for k in range(3):
        t = np.zeros(1, TILE_DTYPE)
        t["seed"] = 20 + k
        tiles.append(torch.from_numpy(t.view(np.uint8).copy()).to(dev))
        outs.append(torch.zeros((H, W, 4), dtype=torch.float32, device=dev))
    dB = _dev(B)
    cam = wgt.camera_param(W / H, spp, 0)
    for k in range(2):
        ctx.render_tiles_async(cam, W, H, W, H, tiles[k].data_ptr(), 1, d_f32=outs[k].data_ptr(), stream=streams[k])
    ctx.update_triangles_device(dB.data_ptr(), len(B))  # no sync: waits for the two frames itself
    ctx.render_tiles_async(cam, W, H, W, H, tiles[2].data_ptr(), 1, d_f32=outs[2].data_ptr(), stream=streams[2])
    ctx.sync()
    torch.cuda.synchronize()
    for k, T in enumerate((A, A, B)):
        fresh.upload_scene(L, Q, S, T)
        ref = fresh.render_tile(wgt.camera_param(W / H, spp, 20 + k), W, H, want=("f32",))["f32"]
        assert np.array_equal(outs[k].cpu().numpy().view(np.uint32), ref.view(np.uint32)), f"frame {k}"


def test_mixed_sequence_of_forms(ctx, wgt):
    """9. Host update to B, device records to C, device vertices back to A's, host update to A: the tree
    after each step; the last is the uploaded one."""
    A = rc.mesh("bunny2000")
    B, C = rc.moved("bunny2000", "jitter5"), rc.moved("bunny2000", "translate1000")
    L, Q, S = host_form._tiny_scene(wgt)
    ctx.upload_scene(L, Q, S, A)
    uploaded = ctx.bvh_read()
    ctx.update_triangles(B)
    rc.assert_trees_equal(ctx.bvh_read(), _want_tree(wgt, ("rec", "bunny2000", "jitter5"), A, B), what="host B")
    dC = _dev(C)
    ctx.update_triangles_device(dC.data_ptr(), len(C))
    rc.assert_trees_equal(ctx.bvh_read(), _want_tree(wgt, ("rec", "bunny2000", "translate1000"), A, C), what="device C")
    V_A = _verts32(A)
    T_A = _records_of(wgt, V_A, A)
    dV = _dev(V_A)
    ctx.update_vertices_device(dV.data_ptr(), 3 * len(A), len(A))
    rc.assert_trees_equal(ctx.bvh_read(), _want_tree(wgt, ("vert", "bunny2000", "to A"), A, T_A), what="vertices of A")
    same = all(np.array_equal(rc.bits(T_A[k][:, :3]), rc.bits(A[k][:, :3])) for k in ("v0", "e1", "e2"))
    print(f"make_triangles of A's vertices reproduces A: {same}")
    if same:
        rc.assert_trees_equal(ctx.bvh_read(), uploaded, what="vertices of A against the upload")
    ctx.update_triangles(A)
    rc.assert_trees_equal(ctx.bvh_read(), uploaded, what="host A")
