"""Properties of the temporal accumulation's specification itself (tests/temporal_restatement.py,
DESIGN.md §4.8), on the CPU: oracle frames of the Cornell box and synthetic data.  The GPU result is
compared with the same restatement bit for bit in tests/test_gpu_temporal.py."""
import numpy as np
import pytest

import hit_records as hr
import temporal_cases as tc
import temporal_restatement as tr
from test_gpu_gbuffer import camera_rays

f32 = np.float32
K, N = 16, 32


@pytest.fixture(scope="module")
def cornell_frames(oracle):
    """K oracle renders of the 32 x 32 Cornell box at spp 4, seeds 0..K-1, under one camera; the
    first-hit guides of seed 0's frame (the restated quad scan on sample 0's camera rays), held for
    every frame: the sequence's colours alone change, as the properties below need (under each frame's
    own jitter an edge pixel's first hit changes surface, and its history rightly restarts)."""
    L, Q, S = oracle.cornell_scene()
    scene = oracle.OracleScene(L, Q, S)
    cams = [oracle.camera_param(1.0, 4, s) for s in range(K)]
    colors = [scene.render(c, N, N, want=("f32",))["f32"] for c in cams]
    o, d = camera_rays(cams[0], N, N)
    rec = hr.quad_sphere_records(o.reshape(-1, 3), d.reshape(-1, 3), L, Q, S)
    g = {k: rec[k].reshape((N, N) + rec[k].shape[1:]) for k in ("prim", "flags", "pos", "norm")}
    return cams[0], colors, g


def _chain(cam, colors, g, **kw):
    states, prev = [], None
    for c in colors:
        prev = tr.accumulate(c, g, cam, prev, None if prev is None else g, None if prev is None else cam, **kw)
        states.append(prev)
    return states


def test_static_camera_is_the_running_mean(cornell_frames):
    cam, colors, g = cornell_frames
    valid = np.logical_and.reduce([tr.valid_mask(c, g) for c in colors])
    assert 0.5 * valid.size < valid.sum() < valid.size  # the light at least passes through
    states = _chain(cam, colors, g, max_history=65536)
    stack = np.stack([c[..., :3] for c in colors]).astype(np.float64)
    bound = 1e-5 * np.abs(stack).max()  # about three roundings of 2^-24 per step
    for k, st in enumerate(states, 1):
        assert (st["len"][valid] == k).all(), k
        err = np.abs(st["f32"][..., :3].astype(np.float64) - stack[:k].mean(axis=0))[valid].max()
        assert err <= bound, (k, err, bound)
        inval = ~tr.valid_mask(colors[k - 1], g)
        assert np.array_equal(st["f32"][inval].view(np.uint32), colors[k - 1][inval].view(np.uint32))
        assert (st["len"][inval] == 0).all() and (st["moments"][:, inval] == 0).all()
        assert np.array_equal(st["f32"][..., 3].view(np.uint32), colors[k - 1][..., 3].view(np.uint32))
        # the moments are the running means of luminance and its square
        lum = tr.luminance(stack[:k].astype(f32)).astype(np.float64)
        assert np.abs(st["moments"][0].astype(np.float64) - lum.mean(axis=0))[valid].max() <= bound
        assert np.abs(st["moments"][1] - (lum * lum).mean(axis=0))[valid].max() <= 1e-5 * (lum * lum).max()


def test_max_history_is_an_exponential_average(cornell_frames):
    cam, colors, g = cornell_frames
    valid = np.logical_and.reduce([tr.valid_mask(c, g) for c in colors])
    states = _chain(cam, colors, g, max_history=4)
    bound = 1e-5 * max(np.abs(c[..., :3]).max() for c in colors)
    e = None
    for k, (st, c) in enumerate(zip(states, colors), 1):
        c64 = c[..., :3].astype(np.float64)
        e = c64 if e is None else e + (c64 - e) / min(k, 4)
        assert (st["len"][valid] == min(k, 4)).all(), k
        assert np.abs(st["f32"][..., :3] - e)[valid].max() <= bound, k
    # 1 = no accumulation: hist + 1 * (cur - hist), the current colour to two roundings
    one = _chain(cam, colors[:3], g, max_history=1)[-1]
    assert np.abs(one["f32"] - colors[2])[valid].max() <= bound and (one["len"][valid] == 1).all()


def _plane_frame(cam, w, h):
    """The guides of a fronto-parallel plane z = 0 with normal -z, seen through the pixel centres."""
    C = tr.camera_constants(cam, w, h)
    ys, xs = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    d = (C["c"] + xs[..., None] * C["du"] + ys[..., None] * C["dv"]).astype(f32)
    pos = (C["o"] + (-C["o"][2] / d[..., 2])[..., None] * d).astype(f32)
    pos[..., 2] = 0.0
    norm = np.broadcast_to(np.array([0, 0, -1], f32), pos.shape).copy()
    return {"prim": np.full((h, w), 7, np.uint32), "flags": np.full((h, w), 2, np.uint8), "pos": pos, "norm": norm}, C


def test_translated_camera_disoccludes_a_strip():
    w, h = 32, 24
    cam_a = tc.camera(w, h)
    px = float(np.linalg.norm(tr.camera_constants(cam_a, w, h)["du"]))  # the plane lies at the focal distance
    cam_b = tc.camera(w, h, (278.0 + 3.25 * px, 278.0, -800.0), (278.0 + 3.25 * px, 278.0, 0.0))
    ga, _ = _plane_frame(cam_a, w, h)
    gb, _ = _plane_frame(cam_b, w, h)
    rng = np.random.default_rng(1)
    ca, cb = (np.concatenate([rng.random((h, w, 3)), np.ones((h, w, 1))], axis=2).astype(f32) for _ in range(2))
    first = tr.accumulate(ca, ga, cam_a)
    assert (first["len"] == 1).all()
    st = tr.accumulate(cb, gb, cam_b, first, ga, cam_a)
    fresh = st["len"] == 1
    assert ((st["len"] == 2) | fresh).all()
    cols = np.flatnonzero(fresh.all(axis=0))
    assert np.array_equal(fresh, np.broadcast_to(fresh.all(axis=0), fresh.shape))  # whole columns
    assert 2 <= len(cols) <= 4 and (np.diff(cols) == 1).all() and (cols[0] == 0 or cols[-1] == w - 1), cols
    # an accumulated pixel is the mean of its colour and the bilinear history at 3.25 pixels' distance
    x = 10 if cols[0] == 0 else 20
    sgn = -1 if cols[0] == 0 else 1
    want = 0.5 * (cb[5, x, :3] + 0.75 * ca[5, x + 3 * sgn, :3] + 0.25 * ca[5, x + 4 * sgn, :3])
    assert np.abs(st["f32"][5, x, :3] - want).max() < 1e-3  # the shift is 3.25 pixels to a few 1e-4


def _one_pixel(**change):
    """A 1 x 1 sequence under one camera: the state after the second frame, whose previous guides
    carry `change`."""
    cam = tc.camera(1, 1)
    g = {"prim": np.full((1, 1), 3, np.uint32), "flags": np.zeros((1, 1), np.uint8),
         "pos": np.array([[[1.0, 2.0, 3.0]]], f32), "norm": np.array([[[0.0, 0.6, 0.8]]], f32)}
    c0, c1 = np.array([[[0.5, 0.25, 1.0, 1.0]]], f32), np.array([[[1.5, 0.75, 0.0, 1.0]]], f32)
    params = {k: change.pop(k) for k in ("match_prim", "normal_min", "plane_tol") if k in change}
    gp = {k: (np.array(change[k], g[k].dtype).reshape(g[k].shape) if k in change else g[k]) for k in g}
    first = tr.accumulate(c0, gp, cam)
    return tr.accumulate(c1, g, cam, first, gp, cam, **params)


def test_taps_are_rejected_by_normal_plane_and_primitive():
    kept = _one_pixel()
    assert kept["len"][0, 0] == 2 and np.array_equal(kept["f32"][0, 0], np.array([1.0, 0.5, 0.5, 1.0], f32))
    assert _one_pixel(norm=[0.0, 0.8, 0.6])["len"][0, 0] == 2          # dot = 0.96
    assert _one_pixel(norm=[0.0, 1.0, 0.0])["len"][0, 0] == 1          # dot = 0.6 < 0.9
    assert _one_pixel(norm=[0.0, 1.0, 0.0], normal_min=0.5)["len"][0, 0] == 2
    assert _one_pixel(pos=[9.0, 2.0, 3.0])["len"][0, 0] == 2           # moved within the plane
    assert _one_pixel(pos=[1.0, 2.0, 4.0])["len"][0, 0] == 2           # 0.8 off the plane
    assert _one_pixel(pos=[1.0, 2.0, 5.0])["len"][0, 0] == 1           # 1.6 off the plane
    assert _one_pixel(pos=[1.0, 2.0, 5.0], plane_tol=2.0)["len"][0, 0] == 2
    assert _one_pixel(pos=[1.0, 2.0, 3.5], plane_tol=0.0)["len"][0, 0] == 1
    assert _one_pixel(prim=4)["len"][0, 0] == 2                        # the flag is off by default
    assert _one_pixel(prim=4, match_prim=True)["len"][0, 0] == 1
    assert _one_pixel(match_prim=True)["len"][0, 0] == 2
    for st in (_one_pixel(norm=[0.0, 1.0, 0.0]), _one_pixel(prim=4, match_prim=True)):
        assert np.array_equal(st["f32"][0, 0], np.array([1.5, 0.75, 0.0, 1.0], f32))  # a history restarted


@pytest.mark.parametrize("pair", ["identical", "subpixel", "pixels", "rotated"])
def test_non_finite_history_never_reaches_an_accumulated_pixel(pair):
    """NaN and inf (and 2^101) in every previous field, len among them, under cameras that reach one
    and four taps: the accumulated rgb, len and moments stay finite.  The previous moments hold no NaN
    or inf themselves: they are not part of the tap test and flow into the moments alone."""
    w, h = 67, 35
    color, g, prev, gp = tc.synthetic(w, h, 11)
    cam, cam_prev = tc.camera_pairs(w, h)[pair]
    for max_history in (1, 4, 65536):
        st = tr.accumulate(color, g, cam, prev, gp, cam_prev, max_history=max_history)
        v = tr.valid_mask(color, g)
        assert tc.valid_outputs_finite(st, color, g)
        assert ((st["len"][v] >= 1) & (st["len"][v] <= max_history)).all() and (st["len"][~v] == 0).all()
    # moments with NaN and inf: the colour and the length do not see them
    prev["moments"][:, ::3, ::2] = np.nan
    prev["moments"][:, 1::3, ::2] = np.inf
    st2 = tr.accumulate(color, g, cam, prev, gp, cam_prev, max_history=65536)
    assert np.array_equal(st2["f32"].view(np.uint32), st["f32"].view(np.uint32))
    assert np.array_equal(st2["len"].view(np.uint32), st["len"].view(np.uint32))


def test_synthetic_reaches_every_branch():
    """The generator's claim: under the translated cameras pixels find one to four usable taps, and
    taps fail each test alone."""
    w, h = 67, 35
    color, g, prev, gp = tc.synthetic(w, h, 11)
    cams = tc.camera_pairs(w, h)
    lens = {k: tr.accumulate(color, g, *cams[k][:1], prev, gp, cams[k][1], max_history=65536)["len"] for k in cams}
    v = tr.valid_mask(color, g)
    for k in ("identical", "subpixel", "pixels", "rotated"):
        assert (lens[k][v] == 1).sum() > 20 and (lens[k][v] > 1).sum() > 100, k
    assert (lens["subpixel"] != np.floor(lens["subpixel"])).any()  # lengths blended over several taps
    front = tr.project(tr.camera_constants(cams["behind"][1], w, h), g["pos"])[2]
    assert front[v].any() and not front[v].all()  # part of the image lies behind the previous camera
    loose = tr.accumulate(color, g, cams["identical"][0], prev, gp, cams["identical"][1], normal_min=-1.0)["len"]
    far = tr.accumulate(color, g, cams["identical"][0], prev, gp, cams["identical"][1], plane_tol=100.0)["len"]
    strict = tr.accumulate(color, g, cams["identical"][0], prev, gp, cams["identical"][1], match_prim=True)["len"]
    base = tr.accumulate(color, g, cams["identical"][0], prev, gp, cams["identical"][1])["len"]
    assert ((loose > 1) & (base == 1)).any() and ((far > 1) & (base == 1)).any() and ((strict == 1) & (base > 1)).any()


@pytest.mark.parametrize("degenerate", ["origin_is_target", "along_up"])
def test_degenerate_camera_finds_no_history(degenerate):
    w, h = 17, 5
    color, g, prev, gp = tc.synthetic(w, h, 5)
    bad = tc.camera(w, h, (1.0, 2.0, 3.0), (1.0, 2.0, 3.0) if degenerate == "origin_is_target" else (1.0, 9.0, 3.0))
    C = tr.camera_constants(bad, w, h)
    assert np.isnan(C["k"])
    v = tr.valid_mask(color, g)
    for cam, cam_prev in ((bad, tc.camera(w, h)), (tc.camera(w, h), bad), (bad, bad)):
        st = tr.accumulate(color, g, cam, prev, gp, cam_prev)
        assert (st["len"][v] == 1).all() and (st["len"][~v] == 0).all()
        assert np.array_equal(st["f32"].view(np.uint32), color.view(np.uint32))
