"""wgt_sample_plan and wgt_sample_plan_async against the numpy specification
(tests/sample_plan_restatement.py) bit for bit: the map and its total, at 37 x 21 and
64 x 64, on synthetic states that take every branch and on accumulated Cornell frames of the oracle;
and the calls' refusals through the library, in the documented order.
"""
import ctypes

import numpy as np
import pytest

import sample_plan_cases as sc
import sample_plan_restatement as sp

pytestmark = pytest.mark.gpu

PARAMS = [{}, {"dilate": 0}, {"dilate": 3}, {"side_min": 0, "side_max": 255, "gain": 40.0},
          {"side_min": 3, "side_max": 3}, {"gain": 3e38, "lum_floor": 1e-45}, {"gain": 1e-30, "min_history": 1},
          {"min_history": 64, "dilate": 2}, {"gain": 0.75, "lum_floor": 0.5, "side_max": 5}]


def check(ctx, state, **params):
    want = sp.plan(state, **params)
    got = ctx.sample_plan(state, **params)
    assert got["map"].dtype == np.uint8
    assert np.array_equal(got["map"], want["map"]), f"{np.count_nonzero(got['map'] != want['map'])} sides differ"
    assert got["total"] == want["total"]
    return want


@pytest.fixture(scope="module")
def states(oracle):
    return {(w, h): [sc.synthetic(w, h, 1), sc.synthetic(w, h, 2), sc.quiet_corners(w, h)] +
            sc.cornell_states(oracle, w, h, frames=5)[2:] for w, h in sc.SIZES}


@pytest.mark.parametrize("w,h", sc.SIZES)
@pytest.mark.parametrize("params", PARAMS, ids=lambda p: ",".join(f"{k}={v}" for k, v in p.items()) or "defaults")
def test_plan_equals_the_specification(ctx, states, w, h, params):
    for st in states[(w, h)]:
        check(ctx, st, **params)


@pytest.mark.parametrize("w,h", sc.SIZES)
def test_budgets(ctx, states, w, h):
    """Caps on side_min, on side_max and in between, a budget not even side_min meets, and none."""
    caps = set()
    for st in states[(w, h)][:4]:
        base = dict(side_min=1, side_max=12, gain=2.0)
        for budget in (0.0, 0.5, 1.0, 1.7, 4.0, 9.0, 30.0, 100.0, 144.0, 1e6, 3e38):
            want = check(ctx, st, budget_spp=budget, **base)
            if budget > 0:
                caps.add(want["cap"])
                if sp.capped_total(sp.plan(st, **base)["map"].astype(np.int64), 1) <= want["budget"]:
                    assert want["total"] <= want["budget"]
        over = check(ctx, st, side_min=2, side_max=9, budget_spp=0.5)
        assert over["cap"] == 2 and over["total"] > over["budget"]
    assert {1, 12} <= caps and len(caps) > 3


def test_async_equals_sync_and_feeds_a_sampled_render(ctx, wgt, states):
    """Device pointers: the map and the total of the async form equal the sync form's, its workspace
    holds nothing between calls, and a sampled render queued behind it on the stream reads the map."""
    import torch

    w, h = 64, 64
    dev = torch.device("cuda", 0)
    ws_bytes = wgt.sample_plan_workspace_bytes(w, h)
    ws = torch.full((ws_bytes,), 0xA5, dtype=torch.uint8, device=dev)  # dirty: the call clears what it counts in
    d_map = torch.full((h, w), 0xEE, dtype=torch.uint8, device=dev)
    d_total = torch.zeros(1, dtype=torch.int64, device=dev)
    L, Q, S = wgt.cornell_scene()
    ctx.upload_scene(L, Q, S)
    from webgputracer_amd._lib import TILE_DTYPE

    d_tiles = torch.from_numpy(np.zeros(1, TILE_DTYPE).view(np.uint8).copy()).to(dev)
    d_f32 = torch.zeros((h, w, 4), dtype=torch.float32, device=dev)
    stream = ctx.pipeline_stream(0)
    for st, params in ((states[(w, h)][0], {"budget_spp": 6.0}), (states[(w, h)][4], {"side_max": 3}),
                       (states[(w, h)][1], {"dilate": 3, "budget_spp": 2.0})):
        want = sp.plan(st, **params)
        d_len = torch.from_numpy(np.ascontiguousarray(st["len"], np.float32)).to(dev)
        d_mom = torch.from_numpy(np.ascontiguousarray(st["moments"], np.float32)).to(dev)
        torch.cuda.synchronize()
        ctx.sample_plan_async(w, h, {"len": d_len.data_ptr(), "moments": d_mom.data_ptr()}, ws.data_ptr(), ws_bytes,
                              d_map.data_ptr(), d_total.data_ptr(), stream=stream, **params)
        ctx.render_tiles_async(wgt.camera_param(1.0, 1, 0), w, h, w, h, d_tiles.data_ptr(), 1, d_f32=d_f32.data_ptr(),
                               stream=stream, d_sample_map=d_map.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(d_map.cpu().numpy(), want["map"])
        assert int(d_total.cpu()[0]) == want["total"]
        sync = ctx.render_tile(wgt.camera_param(1.0, 1, 0), w, h, want=("f32",), sample_map=want["map"])["f32"]
        assert np.array_equal(d_f32.cpu().numpy().view(np.uint32), sync.view(np.uint32))


def test_refusals_in_order(ctx, wgt):
    """Each check's refusal names its argument, with every later argument bad as well."""
    from webgputracer_amd import _lib

    L = _lib.lib()
    n = 16
    buf = np.zeros(2 * n, np.float32)
    out = np.zeros(n, np.uint8)
    ok_state = _lib.WgtTemporalState(None, buf.ctypes.data, buf.ctypes.data)
    bad_p = _lib.WgtSamplePlanParams(256, 0, float("nan"), 0.0, 0, 4, -1.0)

    def refused(word, state, map_out, W, H, params):
        rc = L.wgt_sample_plan(ctx.h, ctypes.byref(params) if params is not None else None, W, H,
                               ctypes.byref(state) if state is not None else None, _lib.ptr(map_out), None)
        assert rc == _lib.WGT_E_INVALID and word in L.wgt_last_error(ctx.h).decode(), (word, L.wgt_last_error(ctx.h))

    refused("null state", None, None, 0, 0, bad_p)
    refused("state.len", _lib.WgtTemporalState(None, None, None), None, 0, 0, bad_p)
    refused("state.moments", _lib.WgtTemporalState(None, buf.ctypes.data, None), None, 0, 0, bad_p)
    refused("null map_out", ok_state, None, 0, 0, bad_p)
    refused("image size", ok_state, out, 0, 4, bad_p)
    refused("image size", ok_state, out, 32768, 1025, bad_p)
    p = _lib.WgtSamplePlanParams(256, 0, float("nan"), 0.0, 0, 4, -1.0)
    for word, fix in (("side_min", ("side_min", 2)), ("side_max", ("side_max", 2)), ("gain", ("gain", 1.0)),
                      ("lum_floor", ("lum_floor", 1.0)), ("min_history", ("min_history", 64)), ("dilate", ("dilate", 3)),
                      ("budget_spp", ("budget_spp", 0.0))):
        refused(word, ok_state, out, 4, 4, p)
        setattr(p, *fix)
    assert L.wgt_sample_plan(ctx.h, ctypes.byref(p), 4, 4, ctypes.byref(ok_state), _lib.ptr(out), None) == 0
    for bad in (float("inf"), float("nan"), -0.5):
        q = wgt.sample_plan_defaults()
        q.budget_spp = bad
        refused("budget_spp", ok_state, out, 4, 4, q)
    # the async form's workspace, after everything else; nothing was written
    sentinel = out.copy()
    need = wgt.sample_plan_workspace_bytes(4, 4)
    for ws, size, word in ((None, need, "null workspace"), (0x100000080, need, "misaligned"), (0x100000000, need - 1, "workspace_bytes")):
        rc = L.wgt_sample_plan_async(ctx.h, None, 4, 4, ctypes.byref(ok_state), ctypes.c_void_p(ws), size,
                                     ctypes.c_void_p(0x200000000), None, None)
        assert rc == _lib.WGT_E_INVALID and word in L.wgt_last_error(ctx.h).decode()
    assert np.array_equal(out, sentinel)

    # the sampled renders: the plain calls' checks with spp taken as 1, then the map
    Lq, Q, S = wgt.cornell_scene()
    ctx.upload_scene(Lq, Q, S)
    cam = wgt.camera_param(1.0, 0xFFFFFFFF, 1)  # an spp the plain call refuses
    smap = np.ones((4, 4), np.uint8)

    def render_refused(word, *args):
        rc = L.wgt_render_tile_sampled(ctx.h, *args)
        assert rc == _lib.WGT_E_INVALID and word in L.wgt_last_error(ctx.h).decode(), (word, L.wgt_last_error(ctx.h))

    assert L.wgt_render_tile(ctx.h, _lib.ptr(cam), 4, 4, 0, 0, 4, 4, None, None, None, None) == _lib.WGT_E_INVALID
    render_refused("null camera", None, 0, 0, 9, 9, 0, 0, None, None, None, None, None)
    render_refused("empty frame", _lib.ptr(cam), 0, 4, 9, 9, 0, 0, None, None, None, None, None)
    render_refused("empty tile", _lib.ptr(cam), 4, 4, 9, 9, 0, 4, None, None, None, None, None)
    render_refused("tile origin", _lib.ptr(cam), 4, 4, 4, 0, 4, 4, None, None, None, None, None)
    render_refused("null sample map", _lib.ptr(cam), 4, 4, 0, 0, 4, 4, None, None, None, None, None)
    assert L.wgt_render_tile_sampled(ctx.h, _lib.ptr(cam), 4, 4, 0, 0, 4, 4, _lib.ptr(smap), None, None, None, None) == 0
    one = _lib.WgtHitBuffers(prim=0x200000000)
    tile = ctypes.c_void_p(0x300000000)
    assert L.wgt_render_tiles_sampled_async(ctx.h, _lib.ptr(cam), 4, 4, 4, 4, tile, 1, None, None, None, None,
                                            None) == _lib.WGT_E_INVALID
    assert "null sample map" in L.wgt_last_error(ctx.h).decode()
    assert L.wgt_render_tiles_sampled_async(ctx.h, _lib.ptr(cam), 4, 4, 4, 4, None, 0, None, None, None, None, None) == 0
    assert L.wgt_render_gbuffer_sampled(ctx.h, _lib.ptr(cam), 4, 4, 0, 0, 4, 4, None, None, None) == _lib.WGT_E_INVALID
    assert "null buffer" in L.wgt_last_error(ctx.h).decode()  # the plain call's own check comes first
    assert L.wgt_render_gbuffer_sampled(ctx.h, _lib.ptr(cam), 4, 4, 0, 0, 4, 4, None, ctypes.byref(one),
                                        None) == _lib.WGT_E_INVALID
    assert "null sample map" in L.wgt_last_error(ctx.h).decode()
    assert L.wgt_render_gbuffer_sampled_async(ctx.h, _lib.ptr(cam), 4, 4, 4, 4, tile, 1, None, ctypes.byref(one), None,
                                              None) == _lib.WGT_E_INVALID
    assert "null sample map" in L.wgt_last_error(ctx.h).decode()


def test_frames_adaptive_loop_equals_the_sync_calls(ctx, wgt):
    """FrameRenderer.stream_adaptive (`frames --accumulate --adaptive`): frame 0 uniform at spp, every
    later frame with the map planned from the previous frame's state, all queued on one stream, equals
    the same loop made of the synchronous calls, and no frame spends more than the plain run."""
    from webgputracer_amd.frames import FrameRenderer

    W, H, spp, frames = 40, 24, 4, [3, 4, 5, 6]
    L, Q, S = wgt.cornell_scene()
    ctx.upload_scene(L, Q, S)
    totals = {}
    got = list(FrameRenderer(ctx, W, H, spp).stream_adaptive(frames, max_history=32, totals=totals))
    state = guides = smap = None
    for (f, img, accum) in got:
        cam = wgt.camera_param(W / H, spp, f)
        r = ctx.render_tile(cam, W, H, want=("u8", "f32"), sample_map=smap)
        g = ctx.render_gbuffer(cam, W, H, want=("prim", "pos", "norm", "flags"), sample_map=smap)
        assert np.array_equal(img, r["u8"]), f
        assert totals[f] == (spp * W * H if smap is None else int((smap.astype(np.int64) ** 2).sum()))
        assert totals[f] <= spp * W * H
        state = ctx.temporal_accumulate(r["f32"], g, cam, state, guides, None if state is None else cam, max_history=32)
        assert np.array_equal(accum, state["u8"]), f
        guides = g
        smap = ctx.sample_plan(state, budget_spp=float(spp))["map"]
    assert [f for f, _, _ in got] == frames
