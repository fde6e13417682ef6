"""Rendering with a per-pixel sample count (wgt_render_tile_sampled and its async, G-buffer forms)
against the CPU oracle, bit for bit: pixel (x, y) of a sample map with side k is invocation (x, y)
of compute_sample with camera.spp = k * k.  The frames are partitioned into rectangles of one side
each, so the oracle renders each rectangle at that side's spp (OracleScene.render takes a
sub-rectangle) and its counters add up to the frame's.
"""
import numpy as np
import pytest

from test_gpu_parity import assert_radiance

pytestmark = pytest.mark.gpu

# (x0, y0, w, h, side): disjoint, covering the frame.  Cornell 40 x 24 (partial 8 x 8 blocks; no
# triangles: the traversal-free kernel): 8-aligned and unaligned rectangles; sides 2 and 16 take
# end_sample's multiplying path, 3, 5 and 255 the dividing one, 0 is the empty pixel, and the single
# pixel at 255 reaches the 8-bit limits of the packed sample counters.
CORNELL_W, CORNELL_H, CORNELL_SEED = 40, 24, 5
CORNELL_RECTS = [(0, 0, 16, 8, 2), (16, 0, 24, 8, 1), (0, 8, 13, 16, 3), (13, 8, 16, 11, 5), (29, 8, 11, 16, 0),
                 (13, 19, 15, 5, 16), (28, 19, 1, 1, 255), (28, 20, 1, 4, 1)]
# the 2000-triangle bunny stand-in at 48 x 27, the scene of tests/golden/bunny2000_48x27_spp1_seed3.npz
BUNNY_W, BUNNY_H, BUNNY_SEED = 48, 27, 3
BUNNY_RECTS = [(0, 0, 16, 8, 4), (16, 0, 32, 8, 1), (0, 8, 21, 19, 2), (21, 8, 16, 19, 7), (37, 8, 11, 19, 0)]


def rect_map(W, H, rects):
    m = np.full((H, W), 0xEE, np.uint8)
    seen = np.zeros((H, W), np.int32)
    for x0, y0, w, h, k in rects:
        m[y0:y0 + h, x0:x0 + w] = k
        seen[y0:y0 + h, x0:x0 + w] += 1
    assert (seen == 1).all(), "the rectangles partition the frame"
    return m


def oracle_frame(oracle, osc, W, H, seed, rects):
    """The frame the rectangles' sides ask for, rendered rectangle by rectangle at spp = side^2, and the
    sums of the oracle's counters."""
    ref = {"f32": np.zeros((H, W, 4), np.float32), "u8": np.zeros((H, W, 4), np.uint8),
           "hit": np.zeros((H, W), np.uint32), "counters": np.zeros(8, np.uint64)}
    for x0, y0, w, h, k in rects:
        r = osc.render(oracle.camera_param(W / H, k * k, seed), W, H, x0, y0, w, h)
        for f in ("f32", "u8", "hit"):
            ref[f][y0:y0 + h, x0:x0 + w] = r[f]
        ref["counters"] += r["counters"]
    return ref


def assert_frame(g, ref, oracle=None, smap=None):
    assert_radiance(g["f32"], ref["f32"])
    assert np.array_equal(g["u8"], ref["u8"])
    assert np.array_equal(g["hit"], ref["hit"])
    if oracle is not None:
        st, cnt = g["stats"], ref["counters"]
        assert st["samples"] == int((smap.astype(np.int64) ** 2).sum()) == int(cnt[oracle.CNT_SAMPLES])
        assert st["queries"] == int(cnt[oracle.CNT_QUERIES])
        assert st["traced_rays"] == int(cnt[oracle.CNT_TRACED])
        assert st["nan_rays"] == int(cnt[oracle.CNT_NAN_RAYS])
        assert st["pixels"] == smap.size
        assert st["stack_overflows"] == 0


@pytest.fixture(scope="module")
def cornell(wgt, oracle):
    L, Q, S = wgt.cornell_scene()
    osc = oracle.OracleScene(L, Q, S)
    ref = oracle_frame(oracle, osc, CORNELL_W, CORNELL_H, CORNELL_SEED, CORNELL_RECTS)
    return (L, Q, S), osc, rect_map(CORNELL_W, CORNELL_H, CORNELL_RECTS), ref


@pytest.fixture(scope="module")
def bunny(wgt, oracle):
    L, Q, S, T = wgt.mesh_scene("bunny", target_tris=2000)
    osc = oracle.OracleScene(L, Q, S, T)
    ref = oracle_frame(oracle, osc, BUNNY_W, BUNNY_H, BUNNY_SEED, BUNNY_RECTS)
    return (L, Q, S, T), osc, rect_map(BUNNY_W, BUNNY_H, BUNNY_RECTS), ref


def _scene(request, name):
    scene, osc, smap, ref = request.getfixturevalue(name)
    W, H, seed = (CORNELL_W, CORNELL_H, CORNELL_SEED) if name == "cornell" else (BUNNY_W, BUNNY_H, BUNNY_SEED)
    return scene, smap, ref, W, H, seed


def test_cornell_sampled_parity(ctx, wgt, oracle, cornell):
    scene, _, smap, ref = cornell
    ctx.upload_scene(*scene)
    # cam's spp is ignored: 9 here, and none of the map's
    g = ctx.render_tile(wgt.camera_param(CORNELL_W / CORNELL_H, 9, CORNELL_SEED), CORNELL_W, CORNELL_H, stats=True,
                        sample_map=smap)
    assert_frame(g, ref, oracle, smap)
    empty = smap == 0
    assert np.all(g["f32"][empty][:, :3] == 0) and np.all(g["hit"][empty] == 0xFFFFFFFF)


# the schedules of test_gpu_parity.test_ps_schedule_invariance, the simple kernel, and the pre-pass at
# sides below some of the map's and above others (WGT_PQ_LPT 1, 2, 3 against sides 0, 1, 2, 4, 7), with
# its cost weighted by k^2 (the default) and not
SCHEDULES = [{}, {"WGT_KERNEL": "1"}, {"WGT_PQ_LPT": "0"}, {"WGT_PQ_LPT": "1"}, {"WGT_PQ_LPT": "2"}, {"WGT_PQ_LPT": "3"},
             {"WGT_PQ_LPT": "3", "WGT_PQ_LPT_WEIGHT": "0"}, {"WGT_PQ_LPT_WEIGHT": "0"}, {"WGT_PQ_LPT": "200"},
             {"WGT_PQ_REFILL": "1"}, {"WGT_PQ_REFILL": "64"}, {"WGT_PS_TO_TRAV": "1", "WGT_PS_TO_SERVICE": "63"},
             {"WGT_PQ_LPT_ALL": "0"}, {"WGT_PS_SVC_FRAC": "0"}, {"WGT_PS_SVC_FRAC": "1"}, {"WGT_PQ_DEPTH": "1"},
             {"WGT_PQ_DEPTH": "50"}, {"WGT_CNODE": "0"}, {"WGT_CNODE": "0", "WGT_PQ_LPT": "0"}, {"WGT_PS_WAVES": "5"},
             {"WGT_PS_WAVES": "5", "WGT_CNODE": "0"}, {"WGT_NARROW": "1"}, {"WGT_STACK_LIMIT": "20"},
             {"WGT_PARK": "1"}, {"WGT_PARK": "1", "WGT_CNODE": "0"}, {"WGT_PARK": "1", "WGT_PS_CAP": "8"},
             {"WGT_PARK": "1", "WGT_PS_CAP": "8", "WGT_CNODE": "0"},
             {"WGT_PARK": "1", "WGT_PS_CAP": "8", "WGT_PS_WAVES": "5"},
             {"WGT_PARK": "1", "WGT_PS_CAP": "8", "WGT_PS_WAVES": "5", "WGT_CNODE": "0"},
             {"WGT_PARK": "1", "WGT_PS_CAP": "9", "WGT_PQ_LPT": "0"}, {"WGT_TRI_RATIO": "1"},
             {"WGT_TRI_RATIO": "1000000"}, {"WGT_TRI_RATIO": "1", "WGT_CNODE": "0"}]


@pytest.mark.parametrize("env", SCHEDULES, ids=lambda e: ",".join(f"{k[4:]}={v}" for k, v in e.items()) or "default")
def test_bunny_sampled_schedules(ctx, wgt, oracle, bunny, env, monkeypatch):
    """Every schedule variant gives the oracle's words (so all of them identical ones): both kernels, the
    5- and 6-wave forms, both node forms, the parked form, and the LPT pre-pass off and on."""
    scene, _, smap, ref = bunny
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx.upload_scene(*scene)
    g = ctx.render_tile(wgt.camera_param(BUNNY_W / BUNNY_H, 1, BUNNY_SEED), BUNNY_W, BUNNY_H, stats=True, sample_map=smap)
    assert_frame(g, ref, oracle, smap)


@pytest.mark.parametrize("env", [{}, {"WGT_KERNEL": "1"}, {"WGT_PQ_LPT": "0"}, {"WGT_PQ_LPT": "3"}],
                         ids=["default", "simple", "no-lpt", "lpt3"])
def test_cornell_sampled_schedules(ctx, wgt, oracle, cornell, env, monkeypatch):
    """The traversal-free instantiation under both kernels and the pre-pass off and on."""
    scene, _, smap, ref = cornell
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ctx.upload_scene(*scene)
    g = ctx.render_tile(wgt.camera_param(CORNELL_W / CORNELL_H, 1, CORNELL_SEED), CORNELL_W, CORNELL_H, stats=True,
                        sample_map=smap)
    assert_frame(g, ref, oracle, smap)


@pytest.mark.parametrize("name", ["cornell", "bunny"])
@pytest.mark.parametrize("k", [1, 3, 4])
def test_uniform_map_equals_plain_render(ctx, wgt, request, name, k):
    scene, _, _, W, H, seed = _scene(request, name)
    ctx.upload_scene(*scene)
    plain = ctx.render_tile(wgt.camera_param(W / H, k * k, seed), W, H, stats=True)
    g = ctx.render_tile(wgt.camera_param(W / H, 77, seed), W, H, stats=True, sample_map=np.full((H, W), k, np.uint8))
    for f in ("f32", "u8", "hit"):
        assert np.array_equal(g[f].view(np.uint8), plain[f].view(np.uint8)), f
    for f in ("samples", "queries", "traced_rays", "nan_rays", "pixels"):
        assert g["stats"][f] == plain["stats"][f], f


@pytest.mark.parametrize("name", ["cornell", "bunny"])
def test_sampled_tiles_reassemble_full_frame(ctx, wgt, request, name):
    """The map is indexed by global pixel coordinates: five uneven tiles reproduce the frame, and a
    tile past the frame edge behaves as the plain call's."""
    scene, smap, ref, W, H, seed = _scene(request, name)
    ctx.upload_scene(*scene)
    cam = wgt.camera_param(W / H, 1, seed)
    out = {f: np.zeros_like(ref[f]) for f in ("f32", "u8", "hit")}
    ax, bx, ay, by = W // 2 - 3, W - 11, H // 2 + 1, H - 5
    for (x0, y0, tw, th) in [(0, 0, ax, ay), (ax, 0, W - ax, ay), (0, ay, W, by - ay), (0, by, bx, H - by),
                             (bx, by, W - bx, H - by)]:
        t = ctx.render_tile(cam, W, H, x0, y0, tw, th, sample_map=smap)
        for f in out:
            out[f][y0:y0 + th, x0:x0 + tw] = t[f]
    assert_frame(out, ref)
    g = ctx.render_tile(cam, W, H, W - 10, H - 10, 16, 16, sample_map=smap)
    assert_radiance(g["f32"][:10, :10], ref["f32"][H - 10:, W - 10:])
    assert np.array_equal(g["hit"][:10, :10], ref["hit"][H - 10:, W - 10:])
    assert np.all(g["f32"][10:] == 0) and np.all(g["f32"][:, 10:] == 0)
    assert np.all(g["hit"][10:] == 0xFFFFFFFF) and np.all(g["hit"][:, 10:] == 0xFFFFFFFF)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("name", ["cornell", "bunny"])
def test_sampled_gbuffer(ctx, wgt, request, name):
    """prim equals the sampled render's hit everywhere; each rectangle equals the plain G-buffer at
    spp = side^2 in every field and in the ray; a pixel of side 0 has the miss record and a zero ray."""
    scene, smap, ref, W, H, seed = _scene(request, name)
    rects = CORNELL_RECTS if name == "cornell" else BUNNY_RECTS
    ctx.upload_scene(*scene)
    gb = ctx.render_gbuffer(wgt.camera_param(W / H, 5, seed), W, H, rays=True, sample_map=smap)
    assert np.array_equal(gb["prim"], ref["hit"])
    for x0, y0, w, h, k in rects:
        plain = ctx.render_gbuffer(wgt.camera_param(W / H, k * k, seed), W, H, x0, y0, w, h, rays=True)
        for f, a in plain.items():
            assert np.array_equal(_bits(gb[f][y0:y0 + h, x0:x0 + w]), _bits(a)), (f, k)
    empty = smap == 0
    assert np.all(gb["origin"][empty] == 0) and np.all(gb["direction"][empty] == 0)
    assert np.all(gb["prim"][empty] == 0xFFFFFFFF) and np.all(gb["pos"][empty] == 0) and np.all(gb["flags"][empty] == 0)
    # a tile past the frame edge: defined contents outside, the frame's records inside
    t = ctx.render_gbuffer(wgt.camera_param(W / H, 5, seed), W, H, W - 6, H - 6, 9, 9, want=("prim", "dist"), rays=True,
                           sample_map=smap)
    assert np.array_equal(t["prim"][:6, :6], ref["hit"][H - 6:, W - 6:])
    assert np.all(t["prim"][6:] == 0xFFFFFFFF) and np.all(t["dist"][:, 6:] == 0) and np.all(t["direction"][6:] == 0)


def test_sampled_async_equals_sync(ctx, wgt, bunny, cornell):
    """The async forms with device maps equal the sync forms, and two frames with different maps in
    flight on two pipeline streams do not disturb each other."""
    import torch

    scene, _, smap, ref = bunny
    W, H, seed = BUNNY_W, BUNNY_H, BUNNY_SEED
    ctx.upload_scene(*scene)
    dev = torch.device("cuda", 0)
    cam = wgt.camera_param(W / H, 1, 0)  # per-tile seeds
    maps = [smap, np.ascontiguousarray(smap[::-1, ::-1])]
    want = [ctx.render_tile(wgt.camera_param(W / H, 1, seed), W, H, sample_map=m) for m in maps]
    want_gb = ctx.render_gbuffer(wgt.camera_param(W / H, 1, seed), W, H, rays=True, sample_map=maps[0])
    assert_frame(want[0], ref)
    from webgputracer_amd._lib import TILE_DTYPE

    tiles = np.zeros(1, TILE_DTYPE)
    tiles["seed"] = seed
    d_tiles = torch.from_numpy(tiles.view(np.uint8).copy()).to(dev)
    n = W * H
    bufs = []
    for i, m in enumerate(maps):
        d_map = torch.from_numpy(m.copy()).to(dev)
        b = {"map": d_map, "u8": torch.full((n, 4), 0x5A, dtype=torch.uint8, device=dev),
             "f32": torch.full((n, 4), 7.0, dtype=torch.float32, device=dev),
             "hit": torch.full((n,), 5, dtype=torch.int32, device=dev)}
        bufs.append(b)
    gprim = torch.full((n,), 5, dtype=torch.int32, device=dev)
    gpos = torch.full((3, n), 7.0, dtype=torch.float32, device=dev)
    grays = torch.full((6, n), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    for i, b in enumerate(bufs):
        ctx.render_tiles_async(cam, W, H, W, H, d_tiles.data_ptr(), 1, d_u8=b["u8"].data_ptr(), d_f32=b["f32"].data_ptr(),
                               d_hit=b["hit"].data_ptr(), stream=ctx.pipeline_stream(i), d_sample_map=b["map"].data_ptr())
    ctx.render_gbuffer_async(cam, W, H, W, H, d_tiles.data_ptr(), 1, prim=gprim.data_ptr(), pos=gpos.data_ptr(),
                             d_rays=grays.data_ptr(), stream=ctx.pipeline_stream(0), d_sample_map=bufs[0]["map"].data_ptr())
    torch.cuda.synchronize()
    for b, w in zip(bufs, want):
        assert np.array_equal(b["f32"].cpu().numpy().reshape(H, W, 4).view(np.uint32), w["f32"].view(np.uint32))
        assert np.array_equal(b["u8"].cpu().numpy().reshape(H, W, 4), w["u8"])
        assert np.array_equal(b["hit"].cpu().numpy().view(np.uint32).reshape(H, W), w["hit"])
    assert np.array_equal(gprim.cpu().numpy().view(np.uint32).reshape(H, W), want_gb["prim"])
    assert np.array_equal(_bits(np.moveaxis(gpos.cpu().numpy().reshape(3, H, W), 0, -1)), _bits(want_gb["pos"]))
    r = grays.cpu().numpy().reshape(6, H, W)
    assert np.array_equal(_bits(np.moveaxis(r[:3], 0, -1)), _bits(want_gb["origin"]))
    assert np.array_equal(_bits(np.moveaxis(r[3:], 0, -1)), _bits(want_gb["direction"]))
