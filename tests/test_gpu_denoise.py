"""wgt_denoise on the GPU: every output equals tests/denoise_restatement.py bit for bit (floats
viewed as uint32), on rendered scenes and on synthetic images built to reach every branch of the
kernels; then the call's behaviour (in place, outputs, ordering, two streams), its refusals and the
frames CLI.
"""
import ctypes

import numpy as np
import pytest

import denoise_restatement as dr

pytestmark = pytest.mark.gpu

f32, U32 = np.float32, np.uint32
W, H = 64, 48
GUIDES = ("prim", "pos", "norm", "col", "flags")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(U32)


def _assert_equal(got, color, g, what, **kw):
    """got: Context.denoise's dict; the restatement of (color, g) with the keywords of dr.denoise."""
    ref = dr.denoise(color, g, **kw)
    if got["f32"] is not None:
        bad = np.argwhere(_bits(got["f32"]) != _bits(ref))
        assert len(bad) == 0, f"{what}: {len(bad)} float words differ, first at (y, x, c) = {bad[0]}"
    if got["u8"] is not None:
        assert np.array_equal(got["u8"], dr.unorm8(ref)), f"{what}: rgba8 differs"


# ---- 1. rendered scenes --------------------------------------------------------------------

@pytest.fixture(scope="module")
def rendered(ctx, wgt):
    """Cornell and the 2,000-triangle bunny scene at 64 x 48, spp 4: radiance and G-buffer."""
    out = {}
    cam = wgt.camera_param(W / H, 4, 3)
    for name, scene in (("cornell", wgt.cornell_scene() + (None,)), ("bunny", wgt.mesh_scene("bunny", 2000))):
        ctx.upload_scene(*scene)
        color = ctx.render_tile(cam, W, H, want=("f32",))["f32"]
        g = ctx.render_gbuffer(cam, W, H)
        out[name] = (scene, color, g)
    return out


@pytest.mark.parametrize("name", ["cornell", "bunny"])
@pytest.mark.parametrize("kw", [{}, {"demod": False}, {"sigma_p": 0.25}, {"sigma_p": 16.0}],
                         ids=["defaults", "no_demodulation", "sigma_0.25", "sigma_16"])
def test_rendered_scenes(ctx, rendered, name, kw):
    _, color, g = rendered[name]
    valid = dr.valid_mask(color, g)
    assert 0 < valid.sum() < valid.size  # filtered pixels and pass-through pixels (the light at least)
    got = ctx.denoise(color, g, sigma_pos=kw.get("sigma_p"), demodulate=kw.get("demod", True))
    _assert_equal(got, color, g, f"{name} {kw}", **kw)
    assert not np.array_equal(_bits(got["f32"]), _bits(color))  # it filtered


# ---- 2. synthetic images ---------------------------------------------------------------------

AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)


def synthetic(w, h, seed):
    """A w x h image and guides that reach the kernels' cases: normals from six unit vectors, scaled
    and perturbed so that the normal weight is neither 0 nor 1 and, squared ten times, passes through
    the denormals (0.918^1024 = 9e-39); positions on a lattice along the axes (plane distances 0,
    fractions and tens: falloff 1, in between, 0) with a little noise; albedo above, at and below the
    2^-8 floor; and sprinkled misses, emissive pixels, NaN, inf and 2^101 in every field, and -0
    colours."""
    rng = np.random.default_rng(seed)
    n = w * h
    axis = AXES[rng.integers(0, 6, n)]
    scale = rng.choice(np.array([1.0, 1.0, 1.0, 0.99, 0.97, 0.93, 0.918], f32), n)
    norm = axis * scale[:, None] + np.where(rng.random((n, 1)) < 0.3, rng.normal(0, 0.05, (n, 3)), 0)
    # no longer than 1 (but for a rounding), so that no weight overflows when squared ten times
    norm = (norm / np.maximum(1.0, np.linalg.norm(norm, axis=1, keepdims=True))).astype(f32)
    lattice = np.array([0, 0, 0.25, 0.5, 1, 2, 3, 8, 40], f32)
    pos = (lattice[rng.integers(0, len(lattice), (n, 3))] +
           np.where(rng.random((n, 1)) < 0.5, rng.normal(0, 0.3, (n, 3)), 0)).astype(f32)
    col = rng.choice(np.array([0.73, 0.65, 0.05, 2.0 ** -8, 2.0 ** -9, 0.0, 1.0], f32), (n, 3))
    color = np.concatenate([rng.gamma(0.5, 1.0, (n, 3)), rng.random((n, 1))], axis=1).astype(f32)
    rgb = color[:, :3]  # a view
    rgb[rng.random((n, 3)) < 0.05] = 0.0
    rgb[rng.random((n, 3)) < 0.05] = -0.0
    rgb[rng.random((n, 3)) < 0.03] *= -1.0
    prim = rng.integers(0, 50, n).astype(U32)
    flags = (rng.integers(0, 2, n) * 2).astype(np.uint8)  # WGT_HIT_FRONT_FACE on and off
    prim[rng.random(n) < 0.04] = dr.MISS
    flags[rng.random(n) < 0.04] |= 1
    for field in (pos, norm, col, rgb):
        for bad in (np.nan, np.inf, -np.inf, 2.0 ** 101, -(2.0 ** 101)):
            k = rng.random(n) < 0.008
            field[k, rng.integers(0, 3, k.sum())] = bad
    field = None
    color[rng.random(n) < 0.01, 3] = np.nan  # alpha is carried, never looked at
    g = {"prim": prim.reshape(h, w), "flags": flags.reshape(h, w), "pos": pos.reshape(h, w, 3),
         "norm": norm.reshape(h, w, 3), "col": col.reshape(h, w, 3)}
    return color.reshape(h, w, 4), g


SIZES = [(1, 1), (5, 3), (17, 1), (1, 17), (67, 35), (130, 9)]


@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_synthetic(ctx, size):
    """Sizes that are no multiple of the 64 x 4 block and narrower than the footprint (2 * 2^i each
    way, i up to 7); iterations 1..8 with normal_power 0, 7 and 10."""
    w, h = size
    color, g = synthetic(w, h, 100 * w + h)
    v = dr.valid_mask(color, g)
    if w * h > 100:
        assert 0.5 * v.size < v.sum() < v.size
    # no filtered pixel is NaN (a NaN's sign and payload would be the hardware's choice)
    assert np.isfinite(dr.denoise(color, g, iters=8, npow=10)[..., :3][v]).all()
    for it in range(1, 9):
        for npow in (0, 7, 10):
            got = ctx.denoise(color, g, iterations=it, normal_power=npow)
            _assert_equal(got, color, g, f"{w}x{h} iterations {it} normal_power {npow}", iters=it, npow=npow)
    got = ctx.denoise(color, g, iterations=8, sigma_pos=0.05, demodulate=False)
    _assert_equal(got, color, g, f"{w}x{h} sigma 0.05", iters=8, sigma_p=0.05, demod=False)


@pytest.mark.parametrize("tiled_step", ["0", "16"], ids=["gather_only", "tiled_to_16"])
@pytest.mark.parametrize("size", [(5, 3), (1, 17), (67, 35), (130, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_both_pass_forms_at_every_step(ctx, monkeypatch, size, tiled_step):
    """The passes' two forms compute the same bits: WGT_DENOISE_TILED_STEP = 0 runs every pass as the
    gather, 16 runs the LDS-tiled form at every step its tile fits (the default switches at 8)."""
    monkeypatch.setenv("WGT_DENOISE_TILED_STEP", tiled_step)
    w, h = size
    color, g = synthetic(w, h, 100 * w + h)
    for it in range(1, 9):
        got = ctx.denoise(color, g, iterations=it, normal_power=(0, 7, 10)[it % 3])
        _assert_equal(got, color, g, f"tiled step {tiled_step}, {w}x{h} iterations {it}", iters=it,
                      npow=(0, 7, 10)[it % 3])


def test_synthetic_weights_reach_the_denormals():
    """The synthetic generator's claim, on the CPU: at normal_power 10 some normal weights of
    neighbouring pixels are denormal, some 0, some 1."""
    _, g = synthetic(67, 35, 6735)
    n = g["norm"]
    with np.errstate(all="ignore"):
        wn = dr.max0(dr.dot3(n[:, 1:], n[:, :-1]))
        for _ in range(10):
            wn = wn * wn
    tiny = np.finfo(f32).tiny
    assert ((wn > 0) & (wn < tiny)).any() and (wn == 0).any() and (wn == 1).any()


# ---- 3. behaviour ----------------------------------------------------------------------------

class Dev:
    """An image and its guides on the device (torch tensors), with the raw addresses denoise_async takes."""

    def __init__(self, wgt, color, g):
        import torch

        self.torch, self.dev = torch, torch.device("cuda", 0)
        self.h, self.w = color.shape[:2]
        self.color = self.up(color)
        self.g = {k: self.up(np.moveaxis(g[k], -1, 0) if g[k].ndim == 3 else g[k]) for k in GUIDES}
        self.ws_bytes = wgt.denoise_workspace_bytes(self.w, self.h)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=self.dev)
        assert self.ws.data_ptr() % 256 == 0

    def up(self, a):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        return self.torch.from_numpy(a.copy()).to(self.dev)

    def out(self, dtype):
        t = self.torch
        return t.full((self.h, self.w, 4), 0x5A, dtype=t.uint8 if dtype == "u8" else t.float32, device=self.dev)

    def guides(self):
        return {k: v.data_ptr() for k, v in self.g.items()}

    def run(self, ctx, d_in, f32_out=None, u8_out=None, stream=0, **kw):
        ctx.denoise_async(self.w, self.h, d_in.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                          d_f32_out=f32_out.data_ptr() if f32_out is not None else 0,
                          d_u8_out=u8_out.data_ptr() if u8_out is not None else 0, stream=stream, **self.guides(), **kw)


def _np(t):
    return t.cpu().numpy()


def test_async_forms_outputs_and_in_place(ctx, wgt):
    """Async equals sync and the restatement; f32-only and u8-only equal the halves of a call with
    both; in place equals out of place; the input and the guides are not written."""
    import torch

    color, g = synthetic(67, 35, 7)
    ref = dr.denoise(color, g)
    d = Dev(wgt, color, g)
    before = {k: _np(v).copy() for k, v in d.g.items()}
    o32, o8, only32, only8 = d.out("f32"), d.out("u8"), d.out("f32"), d.out("u8")
    torch.cuda.synchronize()
    d.run(ctx, d.color, o32, o8)
    d.run(ctx, d.color, f32_out=only32)
    d.run(ctx, d.color, u8_out=only8)
    ctx.sync()
    assert np.array_equal(_bits(_np(o32)), _bits(ref)) and np.array_equal(_np(o8), dr.unorm8(ref))
    assert np.array_equal(_bits(_np(only32)), _bits(ref)) and np.array_equal(_np(only8), dr.unorm8(ref))
    assert np.array_equal(_bits(_np(d.color)), _bits(color)), "the input was written"
    for k in GUIDES:
        assert np.array_equal(_np(d.g[k]).view(np.uint8), before[k].view(np.uint8)), f"guides.{k} was written"
    sync = ctx.denoise(color, g)
    assert np.array_equal(_bits(sync["f32"]), _bits(ref)) and np.array_equal(sync["u8"], dr.unorm8(ref))
    half = ctx.denoise(color, g, want=("u8",))
    assert half["f32"] is None and np.array_equal(half["u8"], sync["u8"])
    half = ctx.denoise(color, g, want=("f32",))
    assert half["u8"] is None and np.array_equal(_bits(half["f32"]), _bits(ref))
    d.run(ctx, d.color, f32_out=d.color, u8_out=o8)  # in place
    ctx.sync()
    assert np.array_equal(_bits(_np(d.color)), _bits(ref)) and np.array_equal(_np(o8), dr.unorm8(ref))


def test_ordered_after_the_render_on_its_stream(ctx, wgt, rendered):
    """render_tiles_async, render_gbuffer_async and denoise_async queued on one stream without a
    synchronisation in between equal the stepwise result."""
    import torch

    from webgputracer_amd._lib import TILE_DTYPE

    scene, color, g = rendered["bunny"]
    ctx.upload_scene(*scene)
    cam = wgt.camera_param(W / H, 4, 3)
    d = Dev(wgt, np.zeros_like(color), {k: np.zeros_like(g[k]) for k in GUIDES})
    tile = np.zeros(1, TILE_DTYPE)
    tile["seed"] = 3
    d_tile = torch.from_numpy(tile.view(np.uint8).copy()).to(d.dev)
    o32, o8 = d.out("f32"), d.out("u8")
    torch.cuda.synchronize()
    s = ctx.pipeline_stream(1)
    ctx.render_tiles_async(cam, W, H, W, H, d_tile.data_ptr(), 1, d_f32=d.color.data_ptr(), stream=s)
    ctx.render_gbuffer_async(cam, W, H, W, H, d_tile.data_ptr(), 1, stream=s, **d.guides())
    d.run(ctx, d.color, o32, o8, stream=s)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_np(d.color)), _bits(color))
    step = ctx.denoise(color, g)
    assert np.array_equal(_bits(_np(o32)), _bits(step["f32"])) and np.array_equal(_np(o8), step["u8"])


def test_two_streams_two_workspaces(ctx, wgt):
    """Two images on two pipeline streams, each with its own workspace: each equals its restatement."""
    import torch

    a, b = synthetic(130, 9, 21), synthetic(67, 35, 22)
    da, db = Dev(wgt, *a), Dev(wgt, *b)
    oa, ob = da.out("f32"), db.out("f32")
    torch.cuda.synchronize()
    for _ in range(3):
        da.run(ctx, da.color, f32_out=oa, stream=ctx.pipeline_stream(0), iterations=8)
        db.run(ctx, db.color, f32_out=ob, stream=ctx.pipeline_stream(1), iterations=8)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_np(oa)), _bits(dr.denoise(*a, iters=8)))
    assert np.array_equal(_bits(_np(ob)), _bits(dr.denoise(*b, iters=8)))


# ---- 4. refusals -----------------------------------------------------------------------------

def test_refusals(ctx, wgt):
    """Each refusal of both forms is WGT_E_INVALID, names its argument and leaves the outputs
    untouched; a valid call afterwards works."""
    from webgputracer_amd import _lib

    L = _lib.lib()
    color, g = synthetic(17, 5, 3)
    d = Dev(wgt, color, g)
    o32, o8 = d.out("f32"), d.out("u8")
    h32, h8 = np.full((5, 17, 4), 7.0, f32), np.full((5, 17, 4), 7, np.uint8)
    planar = {k: np.ascontiguousarray(np.moveaxis(g[k], -1, 0) if g[k].ndim == 3 else g[k]) for k in GUIDES}
    P = ctypes.c_void_p

    def call(form, **over):
        """The valid call of `form` with the arguments in `over` replaced."""
        a = dict(ctx=ctx.h, params=None, W=17, H=5, inp=True, guides={k: True for k in GUIDES}, ws=d.ws.data_ptr(),
                 ws_bytes=d.ws_bytes, o32=True, o8=True)
        a.update(over)
        host = form == "sync"
        gb = None
        if a["guides"] is not None:
            gb = _lib.WgtHitBuffers(**{k: (planar[k].ctypes.data if host else d.g[k].data_ptr())
                                       for k in GUIDES if a["guides"].get(k)})
        inp = (color.ctypes.data if host else d.color.data_ptr()) if a["inp"] else None
        out32 = (h32.ctypes.data if host else o32.data_ptr()) if a["o32"] else None
        out8 = (h8.ctypes.data if host else o8.data_ptr()) if a["o8"] else None
        par = ctypes.byref(a["params"]) if a["params"] is not None else None
        gref = ctypes.byref(gb) if gb is not None else None
        if host:
            return L.wgt_denoise(a["ctx"], par, a["W"], a["H"], P(inp), gref, P(out32), P(out8))
        return L.wgt_denoise_async(a["ctx"], par, a["W"], a["H"], P(inp), gref, P(a["ws"] or None), a["ws_bytes"],
                                   P(out32), P(out8), None)

    def params(**kw):
        p = wgt.denoise_defaults()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    cases = [("context", dict(ctx=None)), ("input", dict(inp=False)), ("guides", dict(guides=None))]
    cases += [(f"guides.{k}", dict(guides={j: j != k for j in GUIDES})) for k in GUIDES]
    cases += [("outputs", dict(o32=False, o8=False)), ("size", dict(W=0)), ("size", dict(H=0)),
              ("size", dict(W=32769, H=1)), ("size", dict(W=8192, H=8192)),
              ("iterations", dict(params=params(iterations=0))), ("iterations", dict(params=params(iterations=9))),
              ("normal_power", dict(params=params(normal_power=11))),
              ("sigma_pos", dict(params=params(sigma_pos=0.0))), ("sigma_pos", dict(params=params(sigma_pos=-1.0))),
              ("sigma_pos", dict(params=params(sigma_pos=float("nan")))),
              ("sigma_pos", dict(params=params(sigma_pos=float("inf")))), ("flags", dict(params=params(flags=2)))]
    only_async = [("workspace", dict(ws=0)), ("workspace", dict(ws=d.ws.data_ptr() + 64)),
                  ("workspace_bytes", dict(ws_bytes=d.ws_bytes - 1))]
    for form in ("sync", "async"):
        for word, over in cases + (only_async if form == "async" else []):
            assert call(form, **over) == _lib.WGT_E_INVALID, (form, word, over)
            msg = L.wgt_last_error(over.get("ctx", ctx.h)).decode()
            assert word in msg, (form, word, msg)
    # the order of the checks: the earlier refusal wins
    assert call("async", inp=False, W=0, ws=0) == _lib.WGT_E_INVALID and "input" in L.wgt_last_error(ctx.h).decode()
    assert call("async", W=0, params=params(iterations=0), ws=0) == _lib.WGT_E_INVALID
    assert "size" in L.wgt_last_error(ctx.h).decode()
    assert call("async", params=params(iterations=0), ws=0) == _lib.WGT_E_INVALID
    assert "iterations" in L.wgt_last_error(ctx.h).decode()
    ctx.sync()
    assert (_np(o32) == 0x5A).all() and (_np(o8) == 0x5A).all()
    assert (h32 == 7.0).all() and (h8 == 7).all()
    assert call("sync") == 0 and call("async") == 0
    ctx.sync()
    ref = dr.denoise(color, g)
    assert np.array_equal(_bits(h32), _bits(ref)) and np.array_equal(_bits(_np(o32)), _bits(ref))
    assert np.array_equal(h8, dr.unorm8(ref)) and np.array_equal(_np(o8), dr.unorm8(ref))


# ---- 5. the frames CLI -----------------------------------------------------------------------

def test_frames_cli_denoise(tmp_path, ctx, wgt):
    """frames --denoise writes NNN_denoised.png = Context.denoise of that frame's render and
    G-buffer, and the same NNN.png as without the flag."""
    from PIL import Image

    from webgputracer_amd import frames

    common = ["--frame", "1", "3", "--width", "64", "--height", "48", "--spp", "4", "--scene", "cornell", "--batch", "2"]
    plain, dn = tmp_path / "plain", tmp_path / "dn"
    frames.main(common + ["--out", str(plain)])
    frames.main(common + ["--out", str(dn), "--denoise"])
    assert sorted(p.name for p in plain.iterdir()) == [f"{f:03d}.png" for f in range(3)]
    assert sorted(p.name for p in dn.iterdir()) == sorted([f"{f:03d}.png" for f in range(3)] +
                                                          [f"{f:03d}_denoised.png" for f in range(3)])
    ctx.upload_scene(*wgt.cornell_scene())
    for f in range(3):
        assert (dn / f"{f:03d}.png").read_bytes() == (plain / f"{f:03d}.png").read_bytes()
        cam = wgt.camera_param(64 / 48, 4, f)
        color = ctx.render_tile(cam, 64, 48, want=("f32",))["f32"]
        want = ctx.denoise(color, ctx.render_gbuffer(cam, 64, 48), want=("u8",))["u8"]
        got = np.asarray(Image.open(dn / f"{f:03d}_denoised.png").convert("RGBA"))
        assert np.array_equal(got, want), f
