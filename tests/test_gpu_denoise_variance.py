"""wgt_denoise_variance on the GPU: every output (rgba32f, rgba8, the variance) equals
tests/denoise_variance_restatement.py bit for bit (floats viewed as uint32), on synthetic states built
to reach every branch of the kernels and on rendered, accumulated scenes; then the call's behaviour
(in place, each output alone, ordering, two streams), its refusals and the frames CLI.
"""
import ctypes

import numpy as np
import pytest

import denoise_restatement as dr
import denoise_variance_restatement as dv
import temporal_restatement as tr
import test_gpu_denoise as tgd

pytestmark = pytest.mark.gpu

f32, U32 = np.float32, np.uint32
W, H = 64, 48
GUIDES = tgd.GUIDES
STATE = ("f32", "len", "moments")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(U32)


def _assert_equal(got, st, g, what, ref=None, **kw):
    """got: Context.denoise_variance's dict; the restatement of (st, g) with the keywords of
    dv.denoise_variance (or `ref`, its result)."""
    ref, var = ref if ref is not None else dv.denoise_variance(st, g, **kw)
    if got.get("f32") is not None:
        bad = np.argwhere(_bits(got["f32"]) != _bits(ref))
        assert len(bad) == 0, f"{what}: {len(bad)} float words differ, first at (y, x, c) = {bad[0]}"
    if got.get("u8") is not None:
        assert np.array_equal(got["u8"], dr.unorm8(ref)), f"{what}: rgba8 differs"
    if got.get("var") is not None:
        bad = np.argwhere(_bits(got["var"]) != _bits(var))
        assert len(bad) == 0, f"{what}: {len(bad)} variances differ, first at (y, x) = {bad[0]}"


ALL = ("f32", "u8", "var")

# ---- 1. synthetic states ---------------------------------------------------------------------

LENS = np.array([0, 1, 1, 2.5, 3, 3, 4, 4, 63, 64, 1000, 1000], f32)


def synthetic(w, h, seed):
    """test_gpu_denoise.synthetic's image and guides as a state: history lengths of 0, 1,
    min_history - 1 and min_history (for min_history 1, 4 and 64), a blended 2.5, and 1000; moments
    with m2 < m1^2 from rounding, a variance of exactly 0, denormal, ordinary and large, negative
    means, and NaN, inf and 2^101 sprinkled over both planes."""
    color, g = tgd.synthetic(w, h, seed)
    rng = np.random.default_rng(seed + 77)
    n = w * h
    length = LENS[rng.integers(0, len(LENS), n)]
    m1 = rng.gamma(0.5, 1.0, n).astype(f32)
    m1[rng.random(n) < 0.1] *= f32(-1)
    m1[rng.random(n) < 0.05] = 0
    sq = (m1 * m1).astype(f32)
    kind = rng.integers(0, 6, n)
    m2 = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                   [sq, np.nextafter(sq, f32(0)), sq + f32(1e-40), (sq + f32(1e30)).astype(f32),
                    np.nextafter(sq, f32(np.inf))], (sq + rng.gamma(0.5, 0.3, n)).astype(f32)).astype(f32)
    for plane in (m1, m2):
        for bad in (np.nan, np.inf, -np.inf, 2.0 ** 101, -(2.0 ** 101), 2.0 ** 100):
            plane[rng.random(n) < 0.006] = bad
    return {"f32": color, "len": length.reshape(h, w), "moments": np.stack([m1, m2]).reshape(2, h, w)}, g


def test_synthetic_reaches_every_case():
    """The generator's claim, on the CPU: both variance paths at every min_history, variances of 0,
    denormal and large, and pixels refused by len and by each moment alone."""
    st, g = synthetic(67, 35, 6735)
    v = dv.valid_mask(st, g)
    plain = dr.valid_mask(st["f32"], g)
    assert 0.4 * v.size < v.sum() < plain.sum()
    m1, m2 = st["moments"]
    with np.errstate(all="ignore"):
        assert (plain & (st["len"] == 0)).any() and (plain & ~(np.abs(m1) <= dv.OK_LIMIT)).any()
        assert (plain & ~(np.abs(m2) <= dv.OK_LIMIT)).any()
        raw = (m2 - m1 * m1)[v]
    for mh in (1, 4, 64):
        assert (st["len"][v] >= mh).any() and ((st["len"][v] == mh - 1) | (mh == 1)).any()
    assert (raw < 0).any() and (raw == 0).any() and ((raw > 0) & (raw < 1e-38)).any() and (raw > 1e29).any()
    _, var = dv.denoise_variance(st, g, iters=1)
    assert np.isfinite(var).all() and (var[~v] == 0).all() and (var[v] > 0).any() and (var[v] == 0).any()


SIZES = tgd.SIZES


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_synthetic(ctx, size):
    """Sizes that are no multiple of the 64 x 4 block, narrower than the 7 x 7 window and the
    2 * 2^i footprints, with a one-row and a one-column lattice; iterations 1..8 with normal_power 0, 7
    and 10; sigma_lum 0.25, 4 and 64; min_history 1, 4 and 64; demodulation on and off."""
    w, h = size
    st, g = synthetic(w, h, 100 * w + h)
    v = dv.valid_mask(st, g)
    if w * h > 100:
        assert 0.4 * v.size < v.sum() < v.size
    # no filtered pixel is NaN (a NaN's sign and payload would be the hardware's choice)
    out, var = dv.denoise_variance(st, g, iters=8, npow=10)
    assert np.isfinite(out[..., :3][v]).all() and np.isfinite(var).all()
    for it in range(1, 9):
        for npow in (0, 7, 10):
            got = ctx.denoise_variance(st, g, iterations=it, normal_power=npow, want=ALL)
            _assert_equal(got, st, g, f"{w}x{h} iterations {it} normal_power {npow}", iters=it, npow=npow)
    for sigma_lum in (0.25, 4.0, 64.0):
        for mh in (1, 4, 64):
            demod = (sigma_lum, mh) not in ((0.25, 1), (4.0, 4), (64.0, 64), (64.0, 1))
            got = ctx.denoise_variance(st, g, iterations=3, sigma_lum=sigma_lum, min_history=mh, demodulate=demod,
                                       want=ALL)
            _assert_equal(got, st, g, f"{w}x{h} sigma_lum {sigma_lum} min_history {mh} demodulate {demod}", iters=3,
                          sigma_lum=sigma_lum, min_history=mh, demod=demod)
    got = ctx.denoise_variance(st, g, iterations=8, sigma_pos=0.05, demodulate=False, want=ALL)
    _assert_equal(got, st, g, f"{w}x{h} sigma_pos 0.05", iters=8, sigma_p=0.05, demod=False)


@pytest.mark.parametrize("size", [(5, 3), (1, 17), (67, 35), (130, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_pass_forms_at_every_step(ctx, monkeypatch, size):
    """The passes' two forms compute the same bits: WGT_DENOISE_TILED_STEP = 0 runs every pass as the
    gather, 16 runs the LDS-tiled form at every step its tile fits (the default switches at 8)."""
    w, h = size
    st, g = synthetic(w, h, 100 * w + h)
    for it in range(1, 9):
        kw = dict(iters=it, npow=(0, 7, 10)[it % 3], min_history=(1, 4, 64)[it % 3])
        ref = dv.denoise_variance(st, g, **kw)
        for tiled_step in ("0", "16"):
            monkeypatch.setenv("WGT_DENOISE_TILED_STEP", tiled_step)
            got = ctx.denoise_variance(st, g, iterations=it, normal_power=kw["npow"], min_history=kw["min_history"],
                                       want=ALL)
            _assert_equal(got, st, g, f"tiled step {tiled_step}, {w}x{h} iterations {it}", ref=ref)


# ---- 2. rendered, accumulated scenes ---------------------------------------------------------

@pytest.fixture(scope="module")
def accumulated(ctx, wgt):
    """Cornell and the 2,000-triangle bunny scene at 64 x 48, spp 4: three frames (seeds 3, 4, 5, one
    camera position) through ctx.temporal_accumulate, and the last frame's G-buffer."""
    out = {}
    for name, scene in (("cornell", wgt.cornell_scene() + (None,)), ("bunny", wgt.mesh_scene("bunny", 2000))):
        ctx.upload_scene(*scene)
        st = g = cam = None
        for seed in (3, 4, 5):
            cam_prev, g_prev, cam = cam, g, wgt.camera_param(W / H, 4, seed)
            color = ctx.render_tile(cam, W, H, want=("f32",))["f32"]
            g = ctx.render_gbuffer(cam, W, H)
            st = ctx.temporal_accumulate(color, g, cam, st, g_prev, cam_prev, want=())
        out[name] = (scene, st, g)
    return out


@pytest.mark.parametrize("name", ["cornell", "bunny"])
@pytest.mark.parametrize("kw", [{}, {"demod": False}, {"min_history": 1}, {"sigma_lum": 0.25, "min_history": 3},
                                {"sigma_p": 16.0, "sigma_lum": 64.0}],
                         ids=["defaults", "no_demodulation", "min_history_1", "sigma_lum_0.25", "sigma_lum_64"])
def test_rendered_scenes(ctx, accumulated, name, kw):
    _, st, g = accumulated[name]
    valid = dv.valid_mask(st, g)
    assert 0 < valid.sum() < valid.size  # filtered pixels and pass-through pixels (the light at least)
    assert (st["len"][valid] == 3).any()
    got = ctx.denoise_variance(st, g, sigma_pos=kw.get("sigma_p"), sigma_lum=kw.get("sigma_lum"),
                               min_history=kw.get("min_history"), demodulate=kw.get("demod", True), want=ALL)
    _assert_equal(got, st, g, f"{name} {kw}", **kw)
    assert not np.array_equal(_bits(got["f32"]), _bits(st["f32"]))  # it filtered
    assert (got["var"][valid] > 0).any() and (got["var"][~valid] == 0).all()


# ---- 3. behaviour ----------------------------------------------------------------------------

class Dev(tgd.Dev):
    """A state and its guides on the device, with the raw addresses denoise_variance_async takes."""

    def __init__(self, wgt, st, g):
        super().__init__(wgt, st["f32"], g)
        self.len, self.mom = self.up(st["len"]), self.up(st["moments"])
        self.ws_bytes = wgt.denoise_variance_workspace_bytes(self.w, self.h)
        self.ws = self.torch.empty(self.ws_bytes, dtype=self.torch.uint8, device=self.dev)
        assert self.ws.data_ptr() % 256 == 0

    def state(self):
        return {"f32": self.color.data_ptr(), "len": self.len.data_ptr(), "moments": self.mom.data_ptr()}

    def var(self):
        return self.torch.full((self.h, self.w), 0x5A, dtype=self.torch.float32, device=self.dev)

    def run(self, ctx, f32_out=None, u8_out=None, var_out=None, stream=0, **kw):
        ctx.denoise_variance_async(self.w, self.h, self.state(), self.ws.data_ptr(), self.ws_bytes,
                                   d_f32_out=f32_out.data_ptr() if f32_out is not None else 0,
                                   d_u8_out=u8_out.data_ptr() if u8_out is not None else 0,
                                   d_var_out=var_out.data_ptr() if var_out is not None else 0, stream=stream,
                                   **self.guides(), **kw)


_np = tgd._np


def test_async_forms_outputs_and_in_place(ctx, wgt):
    """Async equals sync and the restatement; each output alone equals its part of a call with all
    three; in place equals out of place; the state and the guides are not written."""
    import torch

    st, g = synthetic(67, 35, 7)
    ref, var = dv.denoise_variance(st, g)
    d = Dev(wgt, st, g)
    before = {k: _np(v).copy() for k, v in d.g.items()}
    o32, o8, ov, only32, only8 = d.out("f32"), d.out("u8"), d.var(), d.out("f32"), d.out("u8")
    torch.cuda.synchronize()
    d.run(ctx, o32, o8, ov)
    d.run(ctx, f32_out=only32)
    d.run(ctx, u8_out=only8)
    ctx.sync()
    assert np.array_equal(_bits(_np(o32)), _bits(ref)) and np.array_equal(_np(o8), dr.unorm8(ref))
    assert np.array_equal(_bits(_np(ov)), _bits(var))
    assert np.array_equal(_bits(_np(only32)), _bits(ref)) and np.array_equal(_np(only8), dr.unorm8(ref))
    assert np.array_equal(_bits(_np(d.color)), _bits(st["f32"])), "state.rgba32f was written"
    assert np.array_equal(_bits(_np(d.len)), _bits(st["len"])), "state.len was written"
    assert np.array_equal(_bits(_np(d.mom)), _bits(st["moments"])), "state.moments was written"
    for k in GUIDES:
        assert np.array_equal(_np(d.g[k]).view(np.uint8), before[k].view(np.uint8)), f"guides.{k} was written"
    sync = ctx.denoise_variance(st, g, want=ALL)
    _assert_equal(sync, st, g, "sync", ref=(ref, var))
    for want in ALL:
        half = ctx.denoise_variance(st, g, want=(want,) if want != "var" else ("u8", "var"))
        assert [k for k in ALL if half[k] is not None] == ([want] if want != "var" else ["u8", "var"])
        _assert_equal(half, st, g, f"want {want}", ref=(ref, var))
    ov2 = d.var()
    d.run(ctx, f32_out=d.color, u8_out=o8, var_out=ov2)  # in place
    ctx.sync()
    assert np.array_equal(_bits(_np(d.color)), _bits(ref)) and np.array_equal(_np(o8), dr.unorm8(ref))
    assert np.array_equal(_bits(_np(ov2)), _bits(var))


def test_ordered_after_the_accumulation_on_its_stream(ctx, wgt, accumulated):
    """temporal_accumulate_async and denoise_variance_async (in place on the new state) queued on one
    stream without a synchronisation in between equal the stepwise result."""
    import torch

    scene, st, g = accumulated["bunny"]
    ctx.upload_scene(*scene)
    cam = wgt.camera_param(W / H, 4, 6)
    color = ctx.render_tile(cam, W, H, want=("f32",))["f32"]
    g2 = ctx.render_gbuffer(cam, W, H)
    prev_cam = wgt.camera_param(W / H, 4, 5)
    step = ctx.temporal_accumulate(color, g2, cam, st, g, prev_cam, want=())
    want = ctx.denoise_variance(step, g2, want=ALL)
    d_prev, d_new = Dev(wgt, st, g), Dev(wgt, {"f32": color, "len": np.zeros((H, W), f32),
                                               "moments": np.zeros((2, H, W), f32)}, g2)
    o8, ov = d_new.out("u8"), d_new.var()
    torch.cuda.synchronize()
    s = ctx.pipeline_stream(1)
    ctx.temporal_accumulate_async(W, H, cam, d_new.color.data_ptr(), d_new.guides(), d_new.state(), d_prev.state(),
                                  d_prev.guides(), prev_cam, stream=s)
    d_new.run(ctx, f32_out=d_new.color, u8_out=o8, var_out=ov, stream=s)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_np(d_new.len)), _bits(step["len"]))
    assert np.array_equal(_bits(_np(d_new.color)), _bits(want["f32"])) and np.array_equal(_np(o8), want["u8"])
    assert np.array_equal(_bits(_np(ov)), _bits(want["var"]))


def test_two_streams_two_workspaces(ctx, wgt):
    """Two states on two pipeline streams, each with its own workspace: each equals its restatement."""
    import torch

    a, b = synthetic(130, 9, 21), synthetic(67, 35, 22)
    da, db = Dev(wgt, *a), Dev(wgt, *b)
    oa, ob = da.out("f32"), db.out("f32")
    torch.cuda.synchronize()
    for _ in range(3):
        da.run(ctx, f32_out=oa, stream=ctx.pipeline_stream(0), iterations=8)
        db.run(ctx, f32_out=ob, stream=ctx.pipeline_stream(1), iterations=8)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_np(oa)), _bits(dv.denoise_variance(*a, iters=8)[0]))
    assert np.array_equal(_bits(_np(ob)), _bits(dv.denoise_variance(*b, iters=8)[0]))


# ---- 4. refusals -----------------------------------------------------------------------------

def test_refusals(ctx, wgt):
    """Each refusal of both forms is WGT_E_INVALID, names its argument and leaves the outputs
    untouched, in the header's order; a valid call afterwards works."""
    from webgputracer_amd import _lib

    L = _lib.lib()
    st, g = synthetic(17, 5, 3)
    d = Dev(wgt, st, g)
    o32, o8, ov = d.out("f32"), d.out("u8"), d.var()
    h32, h8, hv = np.full((5, 17, 4), 7.0, f32), np.full((5, 17, 4), 7, np.uint8), np.full((5, 17), 7.0, f32)
    planar = {k: np.ascontiguousarray(np.moveaxis(g[k], -1, 0) if g[k].ndim == 3 else g[k]) for k in GUIDES}
    host_state = {k: np.ascontiguousarray(st[k], f32) for k in STATE}
    dev_state = d.state()
    FIELD = {"f32": "rgba32f", "len": "len", "moments": "moments"}
    P = ctypes.c_void_p

    def call(form, **over):
        """The valid call of `form` with the arguments in `over` replaced."""
        a = dict(ctx=ctx.h, params=None, W=17, H=5, state={k: True for k in STATE}, guides={k: True for k in GUIDES},
                 ws=d.ws.data_ptr(), ws_bytes=d.ws_bytes, o32=True, o8=True, ov=True)
        a.update(over)
        host = form == "sync"
        gb = sb = None
        if a["guides"] is not None:
            gb = _lib.WgtHitBuffers(**{k: (planar[k].ctypes.data if host else d.g[k].data_ptr())
                                       for k in GUIDES if a["guides"].get(k)})
        if a["state"] is not None:
            sb = _lib.WgtTemporalState(**{FIELD[k]: (host_state[k].ctypes.data if host else dev_state[k])
                                          for k in STATE if a["state"].get(k)})
        out32 = (h32.ctypes.data if host else o32.data_ptr()) if a["o32"] else None
        out8 = (h8.ctypes.data if host else o8.data_ptr()) if a["o8"] else None
        outv = (hv.ctypes.data if host else ov.data_ptr()) if a["ov"] else None
        par = ctypes.byref(a["params"]) if a["params"] is not None else None
        gref = ctypes.byref(gb) if gb is not None else None
        sref = ctypes.byref(sb) if sb is not None else None
        if host:
            return L.wgt_denoise_variance(a["ctx"], par, a["W"], a["H"], sref, gref, P(out32), P(out8), P(outv))
        return L.wgt_denoise_variance_async(a["ctx"], par, a["W"], a["H"], sref, gref, P(a["ws"] or None),
                                            a["ws_bytes"], P(out32), P(out8), P(outv), None)

    def params(**kw):
        p = wgt.denoise_variance_defaults()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    cases = [("context", dict(ctx=None)), ("null state", dict(state=None)), ("null guides", dict(guides=None))]
    cases += [(f"state.{FIELD[k]}", dict(state={j: j != k for j in STATE})) for k in STATE]
    cases += [(f"guides.{k}", dict(guides={j: j != k for j in GUIDES})) for k in GUIDES]
    cases += [("outputs", dict(o32=False, o8=False)), ("size", dict(W=0)), ("size", dict(H=0)),
              ("size", dict(W=32769, H=1)), ("size", dict(W=8192, H=8192)),
              ("iterations", dict(params=params(iterations=0))), ("iterations", dict(params=params(iterations=9))),
              ("normal_power", dict(params=params(normal_power=11))),
              ("sigma_pos", dict(params=params(sigma_pos=0.0))), ("sigma_pos", dict(params=params(sigma_pos=float("nan")))),
              ("flags", dict(params=params(flags=2))),
              ("sigma_lum", dict(params=params(sigma_lum=0.0))), ("sigma_lum", dict(params=params(sigma_lum=-1.0))),
              ("sigma_lum", dict(params=params(sigma_lum=float("nan")))),
              ("sigma_lum", dict(params=params(sigma_lum=float("inf")))),
              ("min_history", dict(params=params(min_history=0))), ("min_history", dict(params=params(min_history=65)))]
    only_async = [("workspace", dict(ws=0)), ("workspace", dict(ws=d.ws.data_ptr() + 64)),
                  ("workspace_bytes", dict(ws_bytes=d.ws_bytes - 1))]
    for form in ("sync", "async"):
        for word, over in cases + (only_async if form == "async" else []):
            assert call(form, **over) == _lib.WGT_E_INVALID, (form, word, over)
            msg = L.wgt_last_error(over.get("ctx", ctx.h)).decode()
            assert word in msg, (form, word, msg)

    # the order of the checks: the earlier refusal wins
    def first(word, **over):
        assert call("async", **over) == _lib.WGT_E_INVALID
        assert word in L.wgt_last_error(ctx.h).decode(), (word, over)

    no_len, no_pos = {j: j != "len" for j in STATE}, {j: j != "pos" for j in GUIDES}
    bad = params(iterations=0)
    first("null guides", guides=None, state=no_len)
    first("state.len", state=no_len, guides=no_pos, o32=False, o8=False, W=0, params=bad, ws=0)
    first("guides.pos", guides=no_pos, o32=False, o8=False, W=0, params=bad, ws=0)
    first("outputs", o32=False, o8=False, W=0, params=bad, ws=0)
    first("size", W=0, params=bad, ws=0)
    first("iterations", params=bad, ws=0)
    first("sigma_pos", params=params(sigma_pos=0.0, sigma_lum=0.0, min_history=0), ws=0)
    first("sigma_lum", params=params(sigma_lum=0.0, min_history=0), ws=0)
    ctx.sync()
    assert (_np(o32) == 0x5A).all() and (_np(o8) == 0x5A).all() and (_np(ov) == 0x5A).all()
    assert (h32 == 7.0).all() and (h8 == 7).all() and (hv == 7.0).all()
    assert call("sync") == 0 and call("async") == 0
    ctx.sync()
    ref, var = dv.denoise_variance(st, g)
    assert np.array_equal(_bits(h32), _bits(ref)) and np.array_equal(_bits(_np(o32)), _bits(ref))
    assert np.array_equal(h8, dr.unorm8(ref)) and np.array_equal(_np(o8), dr.unorm8(ref))
    assert np.array_equal(_bits(hv), _bits(var)) and np.array_equal(_bits(_np(ov)), _bits(var))
    # the variance output alone is optional
    assert call("async", ov=False) == 0 and call("sync", ov=False) == 0


# ---- 5. the frames CLI -----------------------------------------------------------------------

def test_frames_cli_denoise_variance(tmp_path, ctx, wgt):
    """frames --accumulate --denoise-variance writes NNN_accum_vdenoised.png = Context.denoise_variance
    of the host chain's state, and the other files as without the flag; the flag alone is refused."""
    from PIL import Image

    from webgputracer_amd import frames

    n = 32
    common = ["--frame", "1", "3", "--width", str(n), "--height", str(n), "--spp", "4", "--scene", "cornell",
              "--batch", "2", "--accumulate"]
    plain, vdn = tmp_path / "plain", tmp_path / "vdn"
    frames.main(common + ["--out", str(plain)])
    frames.main(common + ["--out", str(vdn), "--denoise-variance"])
    names = [f"{f:03d}{s}.png" for f in range(3) for s in ("", "_accum")]
    assert sorted(p.name for p in plain.iterdir()) == sorted(names)
    assert sorted(p.name for p in vdn.iterdir()) == sorted(names + [f"{f:03d}_accum_vdenoised.png" for f in range(3)])
    ctx.upload_scene(*wgt.cornell_scene())
    st = g_prev = cam_prev = None
    for f in range(3):
        for name in (f"{f:03d}.png", f"{f:03d}_accum.png"):
            assert (vdn / name).read_bytes() == (plain / name).read_bytes(), name
        cam = wgt.camera_param(1.0, 4, f)
        color = ctx.render_tile(cam, n, n, want=("f32",))["f32"]
        g = ctx.render_gbuffer(cam, n, n)
        st = tr.accumulate(color, g, cam, st, g_prev, cam_prev)
        g_prev, cam_prev = g, cam
        want = ctx.denoise_variance(st, g, want=("u8",))["u8"]
        got = np.asarray(Image.open(vdn / f"{f:03d}_accum_vdenoised.png").convert("RGBA"))
        assert np.array_equal(got, want), f
        assert np.array_equal(want, dr.unorm8(dv.denoise_variance(st, g)[0])), f
    for argv in (["--frame", "1", "2", "--denoise-variance"], ["--frame", "1", "2", "--denoise-variance", "--out",
                                                                str(tmp_path / "no")],
                 ["--frame", "1", "2", "--denoise-variance", "--accumulate"]):
        with pytest.raises(SystemExit):
            frames.main(argv)
