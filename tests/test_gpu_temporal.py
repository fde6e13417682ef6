"""wgt_temporal_accumulate on the GPU: every output equals tests/temporal_restatement.py bit for bit
(floats viewed as uint32), on synthetic two-frame sequences built to reach every branch of the kernel
and on rendered sequences with a static camera, a moving camera and a moved mesh; then the call's
behaviour (in place, ping-pong on one stream, two streams, rgba8, the first-frame form), its refusals
and the frames CLI.
"""
import ctypes

import numpy as np
import pytest

import temporal_cases as tc
import temporal_restatement as tr

pytestmark = pytest.mark.gpu

f32, U32 = np.float32, np.uint32
W, H = 64, 48
GUIDES = ("prim", "pos", "norm", "flags")
STATE = ("f32", "len", "moments")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(U32)


def _assert_state(got, ref, what):
    """got: Context.temporal_accumulate's dict (or device arrays read back); ref: the restatement's."""
    for k in STATE:
        if ref[k] is None:
            assert got.get(k) is None, f"{what}: {k} given without moments"
            continue
        bad = np.argwhere(_bits(got[k]) != _bits(ref[k]))
        assert len(bad) == 0, f"{what}: {len(bad)} words of {k} differ, first at {bad[0]}"
    if got.get("u8") is not None:
        assert np.array_equal(got["u8"], tr.unorm8(ref["f32"])), f"{what}: rgba8 differs"


# ---- 1. synthetic sequences ------------------------------------------------------------------

@pytest.mark.parametrize("size", tc.SIZES, ids=[f"{w}x{h}" for w, h in tc.SIZES])
def test_synthetic(ctx, size):
    """Sizes that are no multiple of the 64 x 4 block; every camera pair; with and without moments and
    WGT_TEMPORAL_MATCH_PRIM; max_history 1, 4 and 65536; then the first-frame form."""
    w, h = size
    color, g, prev, gp = tc.synthetic(w, h, 100 * w + h)
    if w * h > 100:
        v = tr.valid_mask(color, g)
        assert 0.5 * v.size < v.sum() < v.size
    for name, (cam, cam_prev) in tc.camera_pairs(w, h).items():
        for i, (moments, match) in enumerate(((True, False), (False, True), (True, True), (False, False))):
            max_history = (65536, 4, 1, 32)[i]
            kw = dict(max_history=max_history, match_prim=match, moments=moments)
            ref = tr.accumulate(color, g, cam, prev, gp, cam_prev, **kw)
            # no accumulated pixel is NaN (a NaN's sign and payload would be the hardware's choice)
            assert tc.valid_outputs_finite(ref, color, g)
            got = ctx.temporal_accumulate(color, g, cam, prev, gp, cam_prev, **kw)
            _assert_state(got, ref, f"{w}x{h} {name} {kw}")
    for kw in (dict(normal_min=-1.0, plane_tol=0.0), dict(normal_min=1.0, plane_tol=100.0), dict(normal_min=0.918)):
        cam, cam_prev = tc.camera_pairs(w, h)["subpixel"]
        got = ctx.temporal_accumulate(color, g, cam, prev, gp, cam_prev, **kw)
        _assert_state(got, tr.accumulate(color, g, cam, prev, gp, cam_prev, **kw), f"{w}x{h} {kw}")
    for moments in (True, False):
        got = ctx.temporal_accumulate(color, g, tc.camera(w, h), moments=moments)
        _assert_state(got, tr.accumulate(color, g, tc.camera(w, h), moments=moments), f"{w}x{h} first frame")


def test_degenerate_camera(ctx):
    """A camera with NaN constants is no error: every accumulated pixel starts a history."""
    w, h = 17, 5
    color, g, prev, gp = tc.synthetic(w, h, 5)
    for bad in (tc.camera(w, h, (1, 2, 3), (1, 2, 3)), tc.camera(w, h, (1, 2, 3), (1, 9, 3))):
        for cam, cam_prev in ((bad, tc.camera(w, h)), (tc.camera(w, h), bad)):
            got = ctx.temporal_accumulate(color, g, cam, prev, gp, cam_prev)
            _assert_state(got, tr.accumulate(color, g, cam, prev, gp, cam_prev), "degenerate camera")
            v = tr.valid_mask(color, g)
            assert (got["len"][v] == 1).all() and (got["len"][~v] == 0).all()


# ---- 2. rendered sequences -------------------------------------------------------------------

def _render(ctx, cam):
    color = ctx.render_tile(cam, W, H, want=("f32",))["f32"]
    g = ctx.render_gbuffer(cam, W, H)
    return color, {k: g[k] for k in GUIDES}


@pytest.mark.parametrize("name", ["cornell", "bunny"])
def test_rendered_sequence(ctx, wgt, name):
    """Four frames with a static camera, three with the origin moved a few units per frame, one after
    update_triangles moved part of the mesh (the bunny scene): chained through the GPU call and,
    separately, through the restatement, equal bits at every frame."""
    scene = wgt.cornell_scene() + (None,) if name == "cornell" else wgt.mesh_scene("bunny", 2000)
    ctx.upload_scene(*scene)
    cams = [wgt.camera_param(W / H, 4, f) for f in range(4)]
    cams += [wgt.camera_param(W / H, 4, 4 + k, origin=(278.0 + 7.0 * (k + 1), 278.0 - 3.0 * (k + 1), -800.0 + 2.0 * k))
             for k in range(3)]
    cams.append(wgt.camera_param(W / H, 4, 7, origin=cams[-1]["origin"][0]))
    got = ref = g_prev = cam_prev = None
    lens = []
    for f, cam in enumerate(cams):
        if f == 7 and name == "bunny":
            tris = scene[3].copy()
            part = tris["v0"][:, 1] > np.median(tris["v0"][:, 1])
            tris["v0"][part, 0] += 25.0
            ctx.update_triangles(tris)
        color, g = _render(ctx, cam)
        first = f == 0
        got = ctx.temporal_accumulate(color, g, cam, *((None,) * 3 if first else (got, g_prev, cam_prev)))
        ref = tr.accumulate(color, g, cam, *((None,) * 3 if first else (ref, g_prev, cam_prev)))
        _assert_state(got, ref, f"{name} frame {f}")
        g_prev, cam_prev = g, cam
        lens.append(got["len"])
    v = lens[3] > 0
    assert (lens[3][v] > 1).any() and lens[3].max() == 4  # the static frames accumulate
    for f in (4, 5, 6):  # after the camera moves: history found and history lost
        assert (lens[f] > 1).any() and (lens[f] == 1).any(), f
    if name == "bunny":
        assert (lens[7] == 1).sum() > (lens[6] == 1).sum()  # the moved part restarted


# ---- 3. behaviour ----------------------------------------------------------------------------

class Dev:
    """A frame (colour and guides) or a state on the device (torch tensors), with raw addresses."""

    def __init__(self, color, g):
        import torch

        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.h, self.w = color.shape[:2]
        self.color = self.up(color)
        self.g = {k: self.up(np.moveaxis(g[k], -1, 0) if g[k].ndim == 3 else g[k]) for k in GUIDES}

    def up(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        return self.torch.from_numpy(a.copy()).to(self.dev)

    def guides(self):
        return {k: v.data_ptr() for k, v in self.g.items()}

    def state(self, moments=True, fill=None):
        """A state set: {"f32", "len", "moments"} tensors, filled with 0x5A bytes or from a host state."""
        t = self.torch
        shapes = {"f32": (self.h, self.w, 4), "len": (self.h, self.w), "moments": (2, self.h, self.w)}
        if fill is not None:
            return {k: self.up(fill[k]) for k in STATE if fill[k] is not None}
        return {k: t.full(shapes[k][:-1] + (4 * shapes[k][-1],), 0x5A, dtype=t.uint8, device=self.dev).view(t.float32)
                for k in STATE if moments or k != "moments"}


def _addr(state):
    return {k: v.data_ptr() for k, v in state.items()}


def _np(t):
    return t.cpu().numpy()


def _host(state):
    return {k: _np(state[k]) if k in state else None for k in STATE}


def test_async_in_place_rgba8_and_first_frame(ctx):
    """Async equals the restatement; out.rgba32f == rgba32f_in in place equals out of place; rgba8 is
    unorm8 of the f32 result; the inputs and the previous state are not written; the first-frame form."""
    import torch

    w, h = 67, 35
    color, g, prev, gp = tc.synthetic(w, h, 7)
    cam, cam_prev = tc.camera_pairs(w, h)["subpixel"]
    ref = tr.accumulate(color, g, cam, prev, gp, cam_prev)
    cur, old = Dev(color, g), Dev(prev["f32"], gp)
    d_prev, out = cur.state(fill=prev), cur.state()
    u8 = torch.full((h, w, 4), 0x5A, dtype=torch.uint8, device=cur.dev)
    torch.cuda.synchronize()
    ctx.temporal_accumulate_async(w, h, cam, cur.color.data_ptr(), cur.guides(), _addr(out), _addr(d_prev), old.guides(),
                                  cam_prev, d_u8_out=u8.data_ptr())
    ctx.sync()
    _assert_state(dict(_host(out), u8=_np(u8)), ref, "async")
    assert np.array_equal(_bits(_np(cur.color)), _bits(color)), "the input was written"
    for k in STATE:
        assert np.array_equal(_bits(_np(d_prev[k])), _bits(prev[k])), f"prev.{k} was written"
    for k in GUIDES:
        assert np.array_equal(_np(old.g[k]).view(np.uint8), np.ascontiguousarray(
            np.moveaxis(gp[k], -1, 0) if gp[k].ndim == 3 else gp[k]).view(np.uint8)), f"guides_prev.{k} was written"
    # in place, without moments, no rgba8
    out2 = {"f32": cur.color, "len": cur.state()["len"]}
    nomom = {k: v for k, v in d_prev.items() if k != "moments"}
    torch.cuda.synchronize()
    ctx.temporal_accumulate_async(w, h, cam, cur.color.data_ptr(), cur.guides(), _addr(out2), _addr(nomom), old.guides(),
                                  cam_prev)
    ctx.sync()
    _assert_state(_host(out2), tr.accumulate(color, g, cam, prev, gp, cam_prev, moments=False), "in place")
    # the first-frame form, on a pipeline stream
    cur = Dev(color, g)
    out3 = cur.state()
    torch.cuda.synchronize()
    ctx.temporal_accumulate_async(w, h, cam, cur.color.data_ptr(), cur.guides(), _addr(out3), stream=ctx.pipeline_stream(0))
    torch.cuda.synchronize()
    _assert_state(_host(out3), tr.accumulate(color, g, cam), "first frame")


def _sequence(w, h, seed, n):
    """n synthetic frames (colour, guides) under slowly moving cameras, and the restated states."""
    frames, cams, states = [], [], []
    px = 582.0 / h
    for f in range(n):
        color, g, _, gp = tc.synthetic(w, h, seed + f)
        frames.append((color, g if f % 2 == 0 else gp))
        cams.append(tc.camera(w, h, (278.0 + 0.4 * px * f, 278.0, -800.0), (278.0 + 0.4 * px * f, 278.0, 0.0)))
        prev = states[-1] if states else None
        states.append(tr.accumulate(*frames[f], cams[f], prev, frames[f - 1][1] if f else None, cams[f - 1] if f else None))
        assert tc.valid_outputs_finite(states[-1], *frames[f])
    return frames, cams, states


def _upload(frames):
    """The frames and two state sets on the device."""
    devs = [Dev(c, g) for c, g in frames]
    return devs, [devs[0].state(), devs[0].state()]


def _queue(ctx, devs, sets, cams, f, stream):
    """Frame f of a sequence on `stream`: out = set f % 2, prev = the other; no synchronisation."""
    d = devs[f]
    ctx.temporal_accumulate_async(d.w, d.h, cams[f], d.color.data_ptr(), d.guides(), _addr(sets[f % 2]),
                                  _addr(sets[(f + 1) % 2]) if f else None, devs[f - 1].guides() if f else None,
                                  cams[f - 1] if f else None, stream=stream)


def test_ping_pong_on_one_stream(ctx):
    import torch

    frames, cams, states = _sequence(67, 35, 40, 5)
    devs, sets = _upload(frames)
    torch.cuda.synchronize()
    for f in range(5):
        _queue(ctx, devs, sets, cams, f, ctx.pipeline_stream(0))
    torch.cuda.synchronize()
    _assert_state(_host(sets[0]), states[4], "frame 4 (set 0)")
    _assert_state(_host(sets[1]), states[3], "frame 3 (set 1)")
    assert (states[4]["len"] > 2).any()


def test_two_sequences_on_two_streams(ctx):
    import torch

    a, b = _sequence(130, 9, 60, 4), _sequence(67, 35, 80, 4)
    (da, sa), (db, sb) = _upload(a[0]), _upload(b[0])
    torch.cuda.synchronize()
    for f in range(4):  # interleaved: the two streams' calls overlap
        _queue(ctx, da, sa, a[1], f, ctx.pipeline_stream(0))
        _queue(ctx, db, sb, b[1], f, ctx.pipeline_stream(1))
    torch.cuda.synchronize()
    _assert_state(_host(sa[1]), a[2][3], "sequence a")
    _assert_state(_host(sb[1]), b[2][3], "sequence b")


# ---- 4. refusals -----------------------------------------------------------------------------

def test_refusals(ctx, wgt):
    """Each refusal of both forms is WGT_E_INVALID, names its argument and leaves the outputs
    untouched; the earlier refusal wins; a valid call afterwards works."""
    from webgputracer_amd import _lib

    L = _lib.lib()
    w, h = 17, 5
    color, g, prev, gp = tc.synthetic(w, h, 3)
    cam = tc.camera(w, h)
    cur, old = Dev(color, g), Dev(prev["f32"], gp)
    d_prev, d_out = cur.state(fill=prev), cur.state()
    planar = {k: np.ascontiguousarray(np.moveaxis(g[k], -1, 0) if g[k].ndim == 3 else g[k]) for k in GUIDES}
    planar_p = {k: np.ascontiguousarray(np.moveaxis(gp[k], -1, 0) if gp[k].ndim == 3 else gp[k]) for k in GUIDES}
    h_out = {"f32": np.full((h, w, 4), 7.0, f32), "len": np.full((h, w), 7.0, f32), "moments": np.full((2, h, w), 7.0, f32)}
    P = ctypes.c_void_p
    n = w * h
    cur.torch.cuda.synchronize()

    def call(form, **over):
        """The valid call of `form` with the arguments in `over` replaced."""
        a = dict(ctx=ctx.h, params=None, W=w, H=h, cam=cam, cam_prev=cam, inp=True, guides={k: True for k in GUIDES},
                 guides_prev={k: True for k in GUIDES}, prev={k: 0 for k in STATE}, out={k: 0 for k in STATE})
        a.update(over)
        host = form == "sync"

        def hits(which, src_host, src_dev):
            if which is None:
                return None
            return _lib.WgtHitBuffers(**{k: (src_host[k].ctypes.data if host else src_dev.g[k].data_ptr())
                                         for k in GUIDES if which.get(k)})

        def state(which, src_host, src_dev):
            """which: None (no struct) or {field: byte offset, None = a null field}."""
            if which is None:
                return None
            base = {k: (src_host[k].ctypes.data if host else src_dev[k].data_ptr()) for k in STATE}
            return _lib.WgtTemporalState(*(None if which.get(k) is None else base[k] + which[k] for k in STATE))

        gb, gpb = hits(a["guides"], planar, cur), hits(a["guides_prev"], planar_p, old)
        sp, so = state(a["prev"], prev, d_prev), state(a["out"], h_out, d_out)
        if a.get("out_over_prev"):  # out's field on top of prev's, shifted by bytes
            k, shift = a["out_over_prev"]
            setattr(so, {"f32": "rgba32f"}.get(k, k), getattr(sp, {"f32": "rgba32f"}.get(k, k)) + shift)
        inp = (color.ctypes.data if host else cur.color.data_ptr()) if a["inp"] else None
        ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
        cam_p = lambda c: c.ctypes.data_as(P) if c is not None else None  # noqa: E731
        args = [a["ctx"], ref(a["params"]), a["W"], a["H"], cam_p(a["cam"]), cam_p(a["cam_prev"]), P(inp), ref(gb), ref(sp),
                ref(gpb), ref(so), None]
        if host:
            return L.wgt_temporal_accumulate(*args)
        return L.wgt_temporal_accumulate_async(*args, None)

    def params(**kw):
        p = wgt.temporal_defaults()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def without(k):
        return {j: (None if j == k else 0) for j in STATE}

    nan, inf = float("nan"), float("inf")
    cases = [("context", dict(ctx=None)), ("input", dict(inp=False)), ("camera", dict(cam=None)),
             ("guides", dict(guides=None)), ("out", dict(out=None)), ("out.rgba32f", dict(out=without("f32"))),
             ("out.len", dict(out=without("len")))]
    cases += [(f"guides.{k}", dict(guides={j: j != k for j in GUIDES})) for k in GUIDES]
    cases += [("first-frame", dict(prev=None)), ("first-frame", dict(guides_prev=None)), ("first-frame", dict(cam_prev=None)),
              ("first-frame", dict(prev=None, cam_prev=None)), ("prev.rgba32f", dict(prev=without("f32"))),
              ("prev.len", dict(prev=without("len")))]
    cases += [(f"guides_prev.{k}", dict(guides_prev={j: j != k for j in GUIDES})) for k in GUIDES]
    cases += [("moments", dict(prev=without("moments"))), ("moments", dict(out=without("moments"))),
              ("size", dict(W=0)), ("size", dict(H=0)), ("size", dict(W=32769, H=1)), ("size", dict(W=8192, H=8192)),
              ("max_history", dict(params=params(max_history=0))), ("max_history", dict(params=params(max_history=65537))),
              ("normal_min", dict(params=params(normal_min=nan))), ("normal_min", dict(params=params(normal_min=1.5))),
              ("normal_min", dict(params=params(normal_min=-inf))), ("plane_tol", dict(params=params(plane_tol=-1.0))),
              ("plane_tol", dict(params=params(plane_tol=nan))), ("plane_tol", dict(params=params(plane_tol=inf))),
              ("flags", dict(params=params(flags=2))),
              ("cam: ", dict(cam=tc.camera(w, h, (nan, 0, 0)))), ("cam_prev: ", dict(cam_prev=tc.camera(w, h, (0, 0, 2.0 ** 41)))),
              ("overlap: out.rgba32f", dict(out_over_prev=("f32", 0))), ("overlap: out.rgba32f", dict(out_over_prev=("f32", 16 * n - 4))),
              ("overlap: out.len", dict(out_over_prev=("len", -4 * n + 4))), ("overlap: out.moments", dict(out_over_prev=("moments", 8)))]
    for form in ("sync", "async"):
        for word, over in cases:
            assert call(form, **over) == _lib.WGT_E_INVALID, (form, word, over)
            msg = L.wgt_last_error(over.get("ctx", ctx.h)).decode()
            assert word in msg, (form, word, msg)
    # the order of the checks: the earlier refusal wins
    for over, word in ((dict(inp=False, W=0, prev=None), "input"), (dict(guides={}, prev=None), "guides.prim"),
                       (dict(prev=None, W=0), "first-frame"), (dict(W=0, params=params(max_history=0)), "size"),
                       (dict(params=params(max_history=0), cam=tc.camera(w, h, (nan, 0, 0))), "max_history"),
                       (dict(cam=tc.camera(w, h, (nan, 0, 0)), out_over_prev=("f32", 0)), "cam: ")):
        assert call("async", **over) == _lib.WGT_E_INVALID and word in L.wgt_last_error(ctx.h).decode(), (over, word)
    ctx.sync()
    for k in STATE:
        assert (_np(d_out[k]).view(np.uint8) == 0x5A).all() and (h_out[k] == 7.0).all(), k
    # adjacent buffers do not overlap; a valid call of each form works
    assert call("sync") == 0 and call("async") == 0
    ctx.sync()
    ref = tr.accumulate(color, g, cam, prev, gp, cam)
    _assert_state(h_out, ref, "sync after the refusals")
    _assert_state(_host(d_out), ref, "async after the refusals")
    assert call("sync", prev=None, guides_prev=None, cam_prev=None) == 0  # the first-frame form
    _assert_state(h_out, tr.accumulate(color, g, cam), "first frame")


# ---- 5. the frames CLI -----------------------------------------------------------------------

def _png(path):
    from PIL import Image

    return np.asarray(Image.open(path).convert("RGBA"))


@pytest.mark.parametrize("pipeline", ["1", "2"])
def test_frames_cli_accumulate(tmp_path, ctx, wgt, pipeline):
    """frames --accumulate writes NNN_accum.png = the restatement chained over the same renders, in
    frame order across batches and pipeline streams; with --denoise also NNN_accum_denoised.png, and
    NNN.png and NNN_denoised.png byte-identical to a run without --accumulate."""
    from webgputracer_amd import frames

    common = ["--frame", "1", "3", "--width", "64", "--height", "48", "--spp", "4", "--scene", "cornell", "--batch", "1",
              "--pipeline", pipeline]
    plain, acc = tmp_path / "plain", tmp_path / "acc"
    frames.main(common + ["--out", str(plain), "--denoise"])
    frames.main(common + ["--out", str(acc), "--denoise", "--accumulate", "--max-history", "8"])
    names = [f"{f:03d}{s}.png" for f in range(3) for s in ("", "_denoised", "_accum", "_accum_denoised")]
    assert sorted(p.name for p in acc.iterdir()) == sorted(names)
    ctx.upload_scene(*wgt.cornell_scene())
    ref = g_prev = cam_prev = None
    for f in range(3):
        for s in ("", "_denoised"):
            assert (acc / f"{f:03d}{s}.png").read_bytes() == (plain / f"{f:03d}{s}.png").read_bytes(), (f, s)
        cam = wgt.camera_param(64 / 48, 4, f)
        color, g = _render(ctx, cam)
        ref = tr.accumulate(color, g, cam, ref, g_prev, cam_prev, max_history=8)
        g_prev, cam_prev = g, cam
        assert np.array_equal(_png(acc / f"{f:03d}_accum.png"), tr.unorm8(ref["f32"])), f
        gd = ctx.render_gbuffer(cam, 64, 48)
        want = ctx.denoise(ref["f32"], gd, want=("u8",))["u8"]
        assert np.array_equal(_png(acc / f"{f:03d}_accum_denoised.png"), want), f
    assert (ref["len"] == 3).any()


def test_frames_cli_accumulate_refusals(monkeypatch, tmp_path):
    from webgputracer_amd import frames

    with pytest.raises(SystemExit):
        frames.main(["--frame", "1", "2", "--accumulate"])  # needs --out
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "0")
    with pytest.raises(SystemExit):
        frames.main(["--frame", "1", "2", "--accumulate", "--out", str(tmp_path)])
