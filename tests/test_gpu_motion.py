"""The motion passes on the GPU (wgt_motion_snapshot, wgt_motion_reproject,
wgt_temporal_accumulate_motion): every output equals tests/motion_restatement.py bit for bit (floats
viewed as uint32; where the restatement is NaN, a NaN), on meshes moved through each of the three
update forms, on synthetic accumulation inputs built to reach every branch, and on two rendered
six-frame sequences of a moving mesh; then the calls' refusals in their order.
"""
import ctypes

import numpy as np
import pytest

import hit_records as hr
import motion_restatement as mr
import temporal_cases as tc
import temporal_restatement as tr
from test_gpu_temporal import Dev, _addr, _assert_state, _host, _np

pytestmark = pytest.mark.gpu

f32, U32 = np.float32, np.uint32
W, H, FRAMES = 64, 48, 6
GUIDES = ("prim", "pos", "norm", "flags")
STATE = ("f32", "len", "moments")
FORMS = ("host", "records", "vertices")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(U32)


def _dev(a):
    """A host array's bytes as a resident torch tensor."""
    import torch

    a = np.ascontiguousarray(a)
    a = a.view(np.uint8) if a.dtype.fields is not None else (a.view(np.int32) if a.dtype == np.uint32 else a)
    t = torch.from_numpy(a.copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _snap_of(tris):
    """What wgt_motion_snapshot_read returns for resident triangles `tris`: (n, 12)."""
    return np.concatenate([tris[k][:, :3] for k in ("v0", "e1", "e2", "face_norm")], axis=1).astype(f32)


def _triangles(wgt, verts, like):
    """wgt_make_triangles of (n, 9) vertices with the colours and flags of `like`."""
    t = wgt.make_triangles(verts)
    t["col"], t["emissive"] = like["col"], like["emissive"]
    return t


def _update(ctx, form, tris, verts):
    """Move the resident mesh to `tris` (= wgt_make_triangles of `verts`) through one of the update forms;
    returns the device tensor the call read, to be kept alive by the caller."""
    if form == "host":
        ctx.update_triangles(tris)
        return None
    d = _dev(tris if form == "records" else verts)
    if form == "records":
        ctx.update_triangles_device(d.data_ptr(), len(tris))
    else:
        ctx.update_vertices_device(d.data_ptr(), 3 * len(tris), len(tris))
    return d


def _assert_motion(got, ref, what):
    for k in ("pos_prev", "norm_prev"):
        g, r = np.asarray(got[k], f32), np.asarray(ref[k], f32)
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        same = (_bits(g) == _bits(r)) | (np.isnan(r) & np.isnan(g))
        bad = np.argwhere(~same)
        assert len(bad) == 0, f"{what}: {len(bad)} words of {k} differ, first at {bad[0]}: {g[tuple(bad[0])]!r} != {r[tuple(bad[0])]!r}"


@pytest.fixture(scope="module")
def bunny(wgt):
    return wgt.mesh_scene("bunny", 2000)


# ---- 1. the snapshot -------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 255, 256, 257, 2000])
def test_snapshot(ctx, wgt, bunny, n):
    """snapshot_read equals (v0, e1, e2, face_norm) of the triangles last uploaded or updated, after an
    upload and after each update form; an update alone does not touch it; a second snapshot replaces
    the first; a re-upload drops it."""
    from webgputracer_amd import _lib

    L, Q, S, T = bunny
    T = T[:n].copy()
    ctx.upload_scene(L, Q, S, T)
    with pytest.raises(wgt.tracer.WgtError, match="snapshot"):
        ctx.motion_snapshot_read()
    ctx.motion_snapshot()
    assert np.array_equal(_bits(ctx.motion_snapshot_read()), _bits(_snap_of(T))), "after the upload"
    resident = T
    for k, form in enumerate(FORMS):
        verts = mr.translated(mr.vertices_of(resident), (3.0 + k, -2.0, 0.5 * k))
        moved = _triangles(wgt, verts, T)
        keep = _update(ctx, form, moved, verts)
        assert np.array_equal(_bits(ctx.motion_snapshot_read()), _bits(_snap_of(resident))), f"{form}: the update wrote it"
        ctx.motion_snapshot(stream=ctx.pipeline_stream(k % 2))
        assert np.array_equal(_bits(ctx.motion_snapshot_read()), _bits(_snap_of(moved))), f"after the {form} update"
        del keep
        resident = moved
    assert ctx.scene_info()["n_tris"] == len(T)  # the "2,000-triangle" bunny has 1,980
    ctx.upload_scene(L, Q, S, T)  # a re-upload drops the snapshot
    g = {"prim": np.zeros(1, U32), "flags": np.zeros(1, np.uint8), "pos": np.zeros((1, 3), f32), "norm": np.zeros((1, 3), f32)}
    with pytest.raises(wgt.tracer.WgtError, match="snapshot") as e:
        ctx.motion_reproject(g)
    assert e.value.code == _lib.WGT_E_INVALID
    with pytest.raises(wgt.tracer.WgtError, match="snapshot"):
        ctx.motion_snapshot_read()


# ---- 2. the reprojection ---------------------------------------------------------------------

def _moved_vertices(base, motion):
    """(before, now): the (n, 9) vertices uploaded and the vertices updated to, and the collapsed pair."""
    n = len(base)
    pts = base.reshape(-1, 3).astype(np.float64)
    centre = pts.mean(axis=0)
    a, b = 7 % n, (n // 2 + 3) % n
    if motion == "none":
        return base, base.copy(), None
    if motion == "half":
        now = base.copy()
        part = base[:, 1] > np.median(base[:, 1])
        now[part] = mr.translated(base[part], (25.0, -4.0, 2.5))
        return base, now, None
    if motion == "rotate_scale":
        q = mr.rotated_y(base, 7.0, centre).reshape(-1, 3).astype(np.float64)
        now = ((q - centre) * np.array([1.1, 0.9, 1.05]) + centre).astype(f32).reshape(-1, 9)
        return base, now, None
    assert motion == "collapse"  # triangle a has zero area before, triangle b after; everything moves
    before, now = base.copy(), mr.translated(base, (5.0, 1.0, -3.0))
    before[a, 6:9] = before[a, 3:6]
    now[b, 6:9] = now[b, 3:6]
    return before, now, (a, b)


def _records(ctx, wgt, nlq, n_tris, extra):
    """The bunny G-buffer at 64 x 48, 1,000 trace_hits records, and synthetic records whose prim ids
    are quads, the sphere, misses, 0xfffffffe and the triangles in `extra`: flat, n records."""
    g = ctx.render_gbuffer(wgt.camera_param(W / H, 4, 3), W, H)
    o, d = hr.random_rays(1000, np.random.default_rng(5))
    t = ctx.trace_hits(o, d)
    rng = np.random.default_rng(9)
    ids = np.array(list(range(nlq)) + [nlq + n_tris, nlq + n_tris + 1, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000] +
                   [nlq + k for k in extra] * 8, U32)
    syn = {"prim": ids, "flags": rng.integers(0, 4, len(ids)).astype(np.uint8),
           "pos": rng.uniform(100, 400, (len(ids), 3)).astype(f32), "norm": rng.normal(size=(len(ids), 3)).astype(f32)}
    flat = {k: np.concatenate([np.asarray(g[k]).reshape((-1, 3) if k in ("pos", "norm") else -1),
                               np.asarray(t[k]).reshape((-1, 3) if k in ("pos", "norm") else -1), syn[k]]) for k in GUIDES}
    is_tri = (flat["prim"] >= nlq) & (flat["prim"] < nlq + n_tris)
    assert is_tri.sum() > 200 and (~is_tri).sum() > 2000
    return flat, is_tri


@pytest.mark.parametrize("motion", ["none", "half", "rotate_scale", "collapse"])
def test_reproject(ctx, wgt, bunny, motion):
    """Bit equality with the restatement for every update form; records that hit no triangle, and
    every record of an unmoved mesh, pass through bitwise; n = 1, 255, 256, 257; the async form on a
    second stream gives the same bits."""
    import torch

    L, Q, S, T = bunny
    nlq = len(L) + len(Q)
    v_before, v_now, pair = _moved_vertices(mr.vertices_of(T), motion)
    before = T.copy() if motion != "collapse" else _triangles(wgt, v_before, T)
    now = before.copy() if motion == "none" else _triangles(wgt, v_now, T)
    if motion == "none":
        v_now = mr.vertices_of(before)
    for form in FORMS:
        ctx.upload_scene(L, Q, S, before)
        ctx.motion_snapshot()
        if form == "vertices" and motion == "none":
            # the vertex form rebuilds e1, e2 from v0 + e1, v0 + e2: the same bits only by chance
            now_f = _triangles(wgt, v_now, T)
        else:
            now_f = now
        keep = _update(ctx, form, now_f, v_now)
        flat, is_tri = _records(ctx, wgt, nlq, len(T), pair or ())
        ref = mr.reproject(flat, nlq, now_f, before)
        got = ctx.motion_reproject(flat)
        _assert_motion(got, ref, f"{motion} {form}")
        for k, src in (("pos_prev", "pos"), ("norm_prev", "norm")):
            assert np.array_equal(_bits(got[k][~is_tri]), _bits(flat[src][~is_tri])), f"{motion} {form}: {k} of a non-triangle"
        if motion == "none" and form != "vertices":
            assert np.array_equal(_bits(got["pos_prev"]), _bits(flat["pos"]))
            assert np.array_equal(_bits(got["norm_prev"]), _bits(flat["norm"]))
        elif motion != "none":
            moved = (_bits(got["pos_prev"]) != _bits(flat["pos"])).any(axis=1)
            assert moved[is_tri].mean() > 0.1 and not moved[~is_tri].any()
        del keep
    if pair:  # the collapsed triangles give NaN, on the side the specification says
        a, b = (flat["prim"] == nlq + pair[0]), (flat["prim"] == nlq + pair[1])
        assert a.sum() >= 8 and np.isnan(got["norm_prev"][a]).all() and np.isfinite(got["pos_prev"][a]).all()
        assert b.sum() >= 8 and np.isnan(got["pos_prev"][b]).all() and np.isfinite(got["norm_prev"][b]).all()
    # sizes around the 256-lane block, from the triangle records on
    first = int(np.flatnonzero(is_tri)[0])
    for n in (1, 255, 256, 257):
        sub = {k: v[first:first + n] for k, v in flat.items()}
        _assert_motion(ctx.motion_reproject(sub), {k: v[first:first + n] for k, v in ref.items()}, f"{motion} n = {n}")
    # the async form on a second stream
    n = len(flat["prim"])
    d = {k: _dev(np.ascontiguousarray(flat[k].T) if flat[k].ndim == 2 else flat[k]) for k in GUIDES}
    out = {k: torch.full((3, n), float("nan"), dtype=torch.float32, device=d["pos"].device) for k in ("pos_prev", "norm_prev")}
    torch.cuda.synchronize()
    ctx.motion_reproject_async(n, {k: v.data_ptr() for k, v in d.items()}, out["pos_prev"].data_ptr(),
                               out["norm_prev"].data_ptr(), stream=ctx.pipeline_stream(1))
    torch.cuda.synchronize()
    _assert_motion({k: _np(v).T for k, v in out.items()}, ref, f"{motion} async")


# ---- 3. the accumulation ---------------------------------------------------------------------

def _synthetic_motion(g, seed):
    """pos_prev and norm_prev for tc.synthetic's guides: copies, perturbed copies, other axes, and NaN,
    inf and 2^101 entries."""
    rng = np.random.default_rng(seed)
    h, w = g["prim"].shape
    pp, npv = g["pos"].copy(), g["norm"].copy()
    k = rng.random((h, w)) < 0.5
    pp[k] += rng.normal(0, 0.3, (int(k.sum()), 3)).astype(f32)
    k = rng.random((h, w)) < 0.25
    npv[k] = tc.AXES[rng.integers(0, 6, int(k.sum()))]
    for field in (pp, npv):
        for bad in tc.BAD:
            k = np.argwhere(rng.random((h, w)) < 0.01)
            field[k[:, 0], k[:, 1], rng.integers(0, 3, len(k))] = bad
    return {"pos_prev": pp, "norm_prev": npv}


@pytest.mark.parametrize("size", tc.SIZES, ids=[f"{w}x{h}" for w, h in tc.SIZES])
def test_accumulate_motion_synthetic(ctx, size):
    """Every camera pair; with and without moments and WGT_TEMPORAL_MATCH_PRIM; max_history 1, 4 and
    65536; the first-frame form with motion = NULL; the identity with wgt_temporal_accumulate."""
    w, h = size
    color, g, prev, gp = tc.synthetic(w, h, 100 * w + h)
    m = _synthetic_motion(g, 7 * w + h)
    for name, (cam, cam_prev) in tc.camera_pairs(w, h).items():
        for i, (moments, match) in enumerate(((True, False), (False, True), (True, True), (False, False))):
            kw = dict(max_history=(65536, 4, 1, 32)[i], match_prim=match, moments=moments)
            ref = mr.accumulate_motion(color, g, cam, m["pos_prev"], m["norm_prev"], prev, gp, cam_prev, **kw)
            assert tc.valid_outputs_finite(ref, color, g)
            got = ctx.temporal_accumulate_motion(color, g, cam, m, prev, gp, cam_prev, **kw)
            _assert_state(got, ref, f"{w}x{h} {name} {kw}")
    if w * h > 100:  # the motion buffers matter: histories found without them are lost with them
        cam, cam_prev = tc.camera_pairs(w, h)["subpixel"]
        plain = tr.accumulate(color, g, cam, prev, gp, cam_prev)["len"]
        with_m = mr.accumulate_motion(color, g, cam, m["pos_prev"], m["norm_prev"], prev, gp, cam_prev)["len"]
        assert ((plain > 1) & (with_m == 1)).any()
    cam, cam_prev = tc.camera_pairs(w, h)["pixels"]
    same = {"pos_prev": g["pos"], "norm_prev": g["norm"]}
    for moments in (True, False):
        got = ctx.temporal_accumulate_motion(color, g, cam, same, prev, gp, cam_prev, moments=moments)
        _assert_state(got, ctx.temporal_accumulate(color, g, cam, prev, gp, cam_prev, moments=moments), f"{w}x{h} identity")
        got = ctx.temporal_accumulate_motion(color, g, tc.camera(w, h), None, moments=moments)
        _assert_state(got, tr.accumulate(color, g, tc.camera(w, h), moments=moments), f"{w}x{h} first frame")
        got = ctx.temporal_accumulate_motion(color, g, tc.camera(w, h), m, moments=moments)  # motion given: ignored
        _assert_state(got, tr.accumulate(color, g, tc.camera(w, h), moments=moments), f"{w}x{h} first frame, motion set")


def test_accumulate_motion_async_in_place(ctx):
    """The async form equals the restatement; out.rgba32f == rgba32f_in in place equals out of place;
    the inputs, the motion buffers and the previous state are not written."""
    import torch

    w, h = 67, 35
    color, g, prev, gp = tc.synthetic(w, h, 7)
    m = _synthetic_motion(g, 3)
    cam, cam_prev = tc.camera_pairs(w, h)["subpixel"]
    ref = mr.accumulate_motion(color, g, cam, m["pos_prev"], m["norm_prev"], prev, gp, cam_prev)
    cur, old = Dev(color, g), Dev(prev["f32"], gp)
    dm = {k: cur.up(np.moveaxis(v, -1, 0)) for k, v in m.items()}
    d_prev, out = cur.state(fill=prev), cur.state()
    u8 = torch.full((h, w, 4), 0x5A, dtype=torch.uint8, device=cur.dev)
    torch.cuda.synchronize()
    ctx.temporal_accumulate_motion_async(w, h, cam, cur.color.data_ptr(), cur.guides(), _addr(out), _addr(dm), _addr(d_prev),
                                         old.guides(), cam_prev, d_u8_out=u8.data_ptr())
    ctx.sync()
    _assert_state(dict(_host(out), u8=_np(u8)), ref, "async")
    assert np.array_equal(_bits(_np(cur.color)), _bits(color)), "the input was written"
    for k, v in m.items():
        assert np.array_equal(_bits(_np(dm[k])), _bits(np.moveaxis(v, -1, 0))), f"motion.{k} was written"
    for k in STATE:
        assert np.array_equal(_bits(_np(d_prev[k])), _bits(prev[k])), f"prev.{k} was written"
    out2 = {"f32": cur.color, "len": cur.state()["len"]}  # in place, without moments, on a pipeline stream
    nomom = {k: v for k, v in d_prev.items() if k != "moments"}
    torch.cuda.synchronize()
    ctx.temporal_accumulate_motion_async(w, h, cam, cur.color.data_ptr(), cur.guides(), _addr(out2), _addr(dm), _addr(nomom),
                                         old.guides(), cam_prev, stream=ctx.pipeline_stream(0))
    torch.cuda.synchronize()
    _assert_state(_host(out2), mr.accumulate_motion(color, g, cam, m["pos_prev"], m["norm_prev"], prev, gp, cam_prev,
                                                    moments=False), "in place")
    cur = Dev(color, g)  # the first-frame form with motion = NULL
    out3 = cur.state()
    torch.cuda.synchronize()
    ctx.temporal_accumulate_motion_async(w, h, cam, cur.color.data_ptr(), cur.guides(), _addr(out3))
    ctx.sync()
    _assert_state(_host(out3), tr.accumulate(color, g, cam), "first frame")


# ---- 4. refusals -----------------------------------------------------------------------------

def test_reproject_and_snapshot_refusals(ctx, wgt, bunny):
    """In the documented order, each naming its argument, nothing written."""
    from webgputracer_amd import _lib

    Lib = _lib.lib()
    P = ctypes.c_void_p
    n = 16
    host = {"prim": np.zeros(n, U32), "flags": np.zeros(n, np.uint8), "pos": np.zeros((3, n), f32), "norm": np.zeros((3, n), f32)}
    out = {k: np.full((3, n), 7.0, f32) for k in ("pos_prev", "norm_prev")}

    def reproject(h, count=n, guides=GUIDES, planes=("pos_prev", "norm_prev"), no_guides=False, no_out=False):
        gb = _lib.WgtHitBuffers(**{k: host[k].ctypes.data for k in guides})
        mb = _lib.WgtMotionBuffers(**{k: out[k].ctypes.data for k in planes})
        return Lib.wgt_motion_reproject(h, count, None if no_guides else ctypes.byref(gb), None if no_out else ctypes.byref(mb))

    def refused(rc, h, word, code=_lib.WGT_E_INVALID):
        assert rc == code, (rc, word)
        assert word in Lib.wgt_last_error(h).decode(), (word, Lib.wgt_last_error(h))

    refused(reproject(None), None, "null context")
    with wgt.Context(0) as empty:  # before an upload
        refused(reproject(empty.h, no_guides=True), empty.h, "no scene", _lib.WGT_E_NOSCENE)
        refused(Lib.wgt_motion_snapshot(empty.h, None), empty.h, "no scene", _lib.WGT_E_NOSCENE)
        refused(Lib.wgt_motion_snapshot_read(empty.h, P(out["pos_prev"].ctypes.data), 1), empty.h, "no scene", _lib.WGT_E_NOSCENE)
    ctx.upload_scene(*wgt.cornell_scene())  # a scene without triangles
    refused(Lib.wgt_motion_snapshot(ctx.h, None), ctx.h, "no triangles")
    refused(reproject(ctx.h), ctx.h, "snapshot")
    L, Q, S, T = bunny
    ctx.upload_scene(L, Q, S, T)
    refused(reproject(ctx.h, no_guides=True, count=0), ctx.h, "snapshot")  # the earlier refusal wins
    ctx.motion_snapshot()
    refused(reproject(ctx.h, no_guides=True, no_out=True, count=0), ctx.h, "null guides")
    for k in GUIDES:
        refused(reproject(ctx.h, guides=[j for j in GUIDES if j != k], no_out=True), ctx.h, f"guides.{k}")
    refused(reproject(ctx.h, no_out=True, count=0), ctx.h, "null out")
    refused(reproject(ctx.h, planes=("norm_prev",), count=0), ctx.h, "out.pos_prev")
    refused(reproject(ctx.h, planes=("pos_prev",), count=0), ctx.h, "out.norm_prev")
    for count in (0, (1 << 25) + 1, 0xFFFFFFFF):
        refused(reproject(ctx.h, count=count), ctx.h, "is not in 1..")
    small = np.zeros((len(T) - 1, 12), f32)
    refused(Lib.wgt_motion_snapshot_read(ctx.h, P(small.ctypes.data), len(T) - 1), ctx.h, "capacity")
    refused(Lib.wgt_motion_snapshot_read(ctx.h, None, len(T)), ctx.h, "null out")
    ctx.sync()
    assert all((v == 7.0).all() for v in out.values())
    assert reproject(ctx.h) == 0  # and a valid call works: unmoved, so the records come back
    assert (out["pos_prev"] == 0).all() and (out["norm_prev"] == 0).all()


def test_accumulate_motion_refusals(ctx):
    """The motion buffers are checked right after the first-frame triple, in both forms; every other
    refusal is wgt_temporal_accumulate's."""
    from webgputracer_amd import _lib

    Lib = _lib.lib()
    P = ctypes.c_void_p
    w, h = 17, 5
    color, g, prev, gp = tc.synthetic(w, h, 3)
    m = _synthetic_motion(g, 1)
    cam = tc.camera(w, h)
    cur, old = Dev(color, g), Dev(prev["f32"], gp)
    d_prev, d_out = cur.state(fill=prev), cur.state()
    dm = {k: cur.up(np.moveaxis(v, -1, 0)) for k, v in m.items()}
    hm = {k: np.ascontiguousarray(np.moveaxis(v, -1, 0)) for k, v in m.items()}
    planar = {k: np.ascontiguousarray(np.moveaxis(g[k], -1, 0) if g[k].ndim == 3 else g[k]) for k in GUIDES}
    planar_p = {k: np.ascontiguousarray(np.moveaxis(gp[k], -1, 0) if gp[k].ndim == 3 else gp[k]) for k in GUIDES}
    h_out = {"f32": np.full((h, w, 4), 7.0, f32), "len": np.full((h, w), 7.0, f32), "moments": np.full((2, h, w), 7.0, f32)}
    cur.torch.cuda.synchronize()

    def call(form, motion=("pos_prev", "norm_prev"), prev_fields=STATE, triple=(True, True, True), W=w, inp=True):
        host = form == "sync"
        gb = _lib.WgtHitBuffers(**{k: (planar[k].ctypes.data if host else cur.g[k].data_ptr()) for k in GUIDES})
        gpb = _lib.WgtHitBuffers(**{k: (planar_p[k].ctypes.data if host else old.g[k].data_ptr()) for k in GUIDES})
        mb = None if motion is None else _lib.WgtMotionBuffers(**{k: (hm[k].ctypes.data if host else dm[k].data_ptr()) for k in motion})
        sp = _lib.WgtTemporalState(*((prev[k].ctypes.data if host else d_prev[k].data_ptr()) if k in prev_fields else None
                                     for k in STATE))
        so = _lib.WgtTemporalState(*(h_out[k].ctypes.data if host else d_out[k].data_ptr() for k in STATE))
        ref = lambda x, on=True: ctypes.byref(x) if x is not None and on else None  # noqa: E731
        args = [ctx.h, None, W, h, cam.ctypes.data_as(P), cam.ctypes.data_as(P) if triple[2] else None,
                P((color.ctypes.data if host else cur.color.data_ptr()) if inp else None), ref(gb), ref(mb), ref(sp, triple[0]),
                ref(gpb, triple[1]), ref(so), None]
        return Lib.wgt_temporal_accumulate_motion(*args) if host else Lib.wgt_temporal_accumulate_motion_async(*args, None)

    cases = [("null motion", dict(motion=None)), ("motion.pos_prev", dict(motion=("norm_prev",))),
             ("motion.norm_prev", dict(motion=("pos_prev",))),
             # the order: what comes before the motion buffers wins, what comes after loses
             ("input", dict(motion=None, inp=False)), ("first-frame", dict(motion=None, triple=(True, False, True))),
             ("null motion", dict(motion=None, prev_fields=("len", "moments"))), ("null motion", dict(motion=None, W=0)),
             ("prev.rgba32f", dict(prev_fields=("len", "moments"))), ("size", dict(W=0))]
    for form in ("sync", "async"):
        for word, over in cases:
            assert call(form, **over) == _lib.WGT_E_INVALID, (form, word, over)
            assert word in Lib.wgt_last_error(ctx.h).decode(), (form, word, Lib.wgt_last_error(ctx.h))
    ctx.sync()
    for k in STATE:
        assert (_np(d_out[k]).view(np.uint8) == 0x5A).all() and (h_out[k] == 7.0).all(), k
    assert call("sync") == 0 and call("async") == 0
    ctx.sync()
    ref = mr.accumulate_motion(color, g, cam, m["pos_prev"], m["norm_prev"], prev, gp, cam)
    _assert_state(h_out, ref, "sync after the refusals")
    _assert_state(_host(d_out), ref, "async after the refusals")
    assert call("sync", motion=None, triple=(False, False, False)) == 0  # the first frame needs no motion
    _assert_state(h_out, tr.accumulate(color, g, cam), "first frame")


# ---- 5. rendered sequences of a moving mesh ------------------------------------------------------

@pytest.fixture(scope="module", params=["translate", "rotate"])
def rendered(request, ctx, wgt, bunny):
    """Six frames (seed = frame index, a static camera) of the bunny scene moved between frames with
    update_vertices_device: snapshot, update, render and G-buffer, reproject, accumulate.  Chain B on the
    GPU and through the restatement, chain A (the plain accumulation) through the restatement."""
    L, Q, S, T = bunny
    nlq = len(L) + len(Q)
    ctx.upload_scene(L, Q, S, T)
    verts = mr.sequence_vertices(T, request.param, FRAMES)
    meshes = [T] + [_triangles(wgt, v, T) for v in verts[1:]]
    got, ref, plain, frames, motions = [], [], [], [], []
    for f in range(FRAMES):
        if f:
            ctx.motion_snapshot()
            keep = _dev(verts[f])
            ctx.update_vertices_device(keep.data_ptr(), 3 * len(T), len(T))
        cam = wgt.camera_param(W / H, 4, f)
        color = ctx.render_tile(cam, W, H, want=("f32",))["f32"]
        g = ctx.render_gbuffer(cam, W, H)
        if f:
            m = ctx.motion_reproject(g)
            mref = mr.reproject(g, nlq, meshes[f], meshes[f - 1])
            motions.append((m, mref))
            got.append(ctx.temporal_accumulate_motion(color, g, cam, m, got[-1], frames[-1], cam))
            ref.append(mr.accumulate_motion(color, g, cam, mref["pos_prev"], mref["norm_prev"], ref[-1], frames[-1], cam))
            plain.append(tr.accumulate(color, g, cam, plain[-1], frames[-1], cam))
        else:
            got.append(ctx.temporal_accumulate_motion(color, g, cam))
            ref.append(mr.accumulate_motion(color, g, cam))
            plain.append(tr.accumulate(color, g, cam))
        frames.append(g)
    return request.param, (nlq, len(T)), frames, motions, got, ref, plain


def test_rendered_sequence_equals_the_restatement(ctx, rendered):
    """Bit equality of the reprojection and of the state at every frame; the last state goes through
    wgt_denoise_variance once: the pipeline joins."""
    motion, (nlq, n_tris), frames, motions, got, ref, plain = rendered
    for f, (m, mref) in enumerate(motions, 1):
        _assert_motion(m, mref, f"{motion} frame {f}")
    for f in range(FRAMES):
        _assert_state(got[f], ref[f], f"{motion} frame {f}")
        is_tri = (frames[f]["prim"] >= nlq) & (frames[f]["prim"] < nlq + n_tris)
        assert np.array_equal(_bits(plain[f]["len"][~is_tri]), _bits(got[f]["len"][~is_tri])), f
    out = ctx.denoise_variance(got[-1], frames[-1], want=("f32", "var"))
    valid = got[-1]["len"] >= 1
    assert out["f32"].shape == (H, W, 4) and np.isfinite(out["f32"][valid]).all() and (out["var"][~valid] == 0).all()
    assert (out["f32"][valid] != got[-1]["f32"][valid]).any()


def test_rendered_sequence_keeps_its_history(rendered):
    """The share conditions of tests/test_motion_restatement.py::test_history_follows_the_mesh, on the
    GPU's own frames: at frame 5, of the triangle pixels, the plain accumulation keeps len >= 3 on at
    most 0.15 (translation) / 0.25 (rotation), the motion form has len == 6 on at least 0.60 / 0.65.

    "len == 6" is the length that rounds to 6, as motion_restatement.shares says.  Measured on an
    MI355X: A 0.051 and 0.126; B 0.730 and 0.779, the restatement's figures exactly."""
    motion, (nlq, n_tris), frames, _, got, _, plain = rendered
    is_tri = (frames[-1]["prim"] >= nlq) & (frames[-1]["prim"] < nlq + n_tris)
    share_a, share_b = mr.shares(plain[-1], got[-1], is_tri, FRAMES)
    print(f"{motion}: A len >= 3: {share_a:.3f}; B len == 6: {share_b:.3f}")
    max_a, min_b = {"translate": (0.15, 0.60), "rotate": (0.25, 0.65)}[motion]
    assert share_a <= max_a, share_a
    assert share_b >= min_b, share_b
