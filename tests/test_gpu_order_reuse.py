"""The pixel queue's order shared by the launches of one view: the first launch
of a view orders itself (TODAY), the second consecutive one makes the kept order (REFINE), later ones
read it (REUSE).  The order shapes the schedule only, so every output is compared bit for bit
(rgba8, rgba32f, hit id) with a context that runs under WGT_PQ_REUSE=0, where every launch orders
itself as before; no tolerance is involved.  The knobs are read per launch, so the reference context's
calls run inside `no_reuse()`."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def no_reuse():
    old = os.environ.get("WGT_PQ_REUSE")
    os.environ["WGT_PQ_REUSE"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["WGT_PQ_REUSE"]
        else:
            os.environ["WGT_PQ_REUSE"] = old


@pytest.fixture(scope="module")
def scene(wgt):
    return wgt.mesh_scene("bunny", target_tris=2000)


@pytest.fixture()
def pair(wgt, scene, monkeypatch):
    """(context under test, reference context), the scene uploaded to both; the refine side pinned."""
    monkeypatch.setenv("WGT_PQ_REUSE", "1")
    monkeypatch.setenv("WGT_PQ_REFINE", "2")
    c, r = wgt.Context(0), wgt.Context(0)
    c.upload_scene(*scene)
    r.upload_scene(*scene)
    yield c, r
    c.close()
    r.close()


def same(a, b):
    return (np.array_equal(a["u8"], b["u8"]) and np.array_equal(a["f32"].view(np.uint32), b["f32"].view(np.uint32))
            and np.array_equal(a["hit"], b["hit"]))


def ref_tile(r, *args, **kw):
    with no_reuse():
        return r.render_tile(*args, **kw)


def counts(c):
    i = c.order_info()
    return i["today"], i["refine"], i["reuse"]


@pytest.mark.parametrize("spp", [16, 4, 1])
def test_three_launches_of_one_view(wgt, pair, spp):
    """52 x 28 has partial 8 x 8 blocks (7 x 4 of them).  16 spp: refine side 2; 4 spp: the side clamps to
    sqrt_spp - 1 = 1; 1 spp: LPT is off and every launch is TODAY."""
    c, r = pair
    W, H = 52, 28
    cam = wgt.camera_param(W / H, spp, 5)
    ref = ref_tile(r, cam, W, H)
    for i in range(3):
        assert same(c.render_tile(cam, W, H), ref), i
    info = c.order_info()
    if spp == 1:
        assert counts(c) == (3, 0, 0) and info["nb"] == 0 and len(c.order_read()) == 0
    else:
        assert counts(c) == (1, 1, 1)
        assert info["nb"] == 28 and info["refine_side"] == (2 if spp == 16 else 1)
        assert np.array_equal(np.sort(c.order_read()), np.arange(28, dtype=np.uint32))
    assert counts(r) == (1, 0, 0) and r.order_info()["nb"] == 0  # the reference: every launch on its own
    assert info["invalidations"] == 0


def test_seeds_are_not_in_the_key_everything_else_is(wgt, pair, scene):
    c, r = pair
    L, Q, S, T = scene
    W, H, spp = 52, 28, 16

    def view(seed=5, origin=(278.0, 278.0, -800.0), W=W, H=H, tw=None, th=None, spp=spp):
        cam = wgt.camera_param(W / H, spp, seed, origin=origin)
        return (cam, W, H), dict(tw=tw, th=th)

    def both(v):
        a, kw = v
        g = c.render_tile(*a, **kw)
        assert same(g, ref_tile(r, *a, **kw))

    base = view()
    for _ in range(3):
        both(base)
    assert counts(c) == (1, 1, 1)
    # another seed: the same view, its own pixels
    both(view(seed=77))
    assert counts(c) == (1, 1, 2)
    assert not same(c.render_tile(*view(seed=78)[0]), ref_tile(r, *base[0]))  # the seeds do differ
    assert counts(c) == (1, 1, 3)
    # each change of view alone: the next launch is TODAY, and the kept order stays the base view's
    today, reuse = 1, 3
    for v in (view(origin=(300.0, 278.0, -800.0)), view(W=53), view(tw=32, th=24), view(spp=4)):
        both(v)
        today += 1
        assert counts(c) == (today, 1, reuse)
        both(base)
        reuse += 1
        assert counts(c) == (today, 1, reuse)
    # each change of the scene alone invalidates: TODAY, then REFINE and REUSE again
    moved = T.copy()
    moved["v0"][:, 0] += 3.0
    refine = 1
    for n, change in enumerate((lambda x: x.upload_scene(L, Q, S, T), lambda x: x.update_triangles(moved),
                                lambda x: x.rebuild_triangles(T))):
        change(c)
        change(r)
        assert c.order_info()["invalidations"] == n + 1 and c.order_info()["nb"] == 0
        both(base)
        today += 1
        assert counts(c) == (today, refine, reuse)
        both(base)
        both(base)
        refine += 1
        reuse += 1
        assert counts(c) == (today, refine, reuse)


def _device_set(torch, dev, n, tw, th):
    return {"u8": torch.zeros((n, th, tw, 4), dtype=torch.uint8, device=dev),
            "f32": torch.zeros((n, th, tw, 4), dtype=torch.float32, device=dev),
            "hit": torch.zeros((n, th, tw), dtype=torch.int32, device=dev)}


def _launch(x, cam, W, H, T, d_t, n, out, stream=0):
    x.render_tiles_async(cam, W, H, T, T, d_t.data_ptr(), n, d_u8=out["u8"].data_ptr(), d_f32=out["f32"].data_ptr(),
                         d_hit=out["hit"].data_ptr(), stream=stream)


def _host(out):
    return {"u8": out["u8"].cpu().numpy(), "f32": out["f32"].cpu().numpy(), "hit": out["hit"].cpu().numpy().view(np.uint32)}


def test_tile_lists(wgt, pair):
    """A resident device tile list is identified by its address: rewriting the origins behind it keeps a
    stale order, which is still a permutation of the same blocks, so the frame is still right."""
    import torch

    c, r = pair
    W, H, T, spp = 64, 48, 16, 16
    dev = torch.device("cuda", 0)
    cam = wgt.camera_param(W / H, spp, 0)
    tiles = wgt.tile_grid(W, H, T, seed=9)
    n = len(tiles)
    assert n == 12
    d_t = torch.from_numpy(tiles.view(np.uint8).copy()).to(dev)
    got, want = _device_set(torch, dev, n, T, T), _device_set(torch, dev, n, T, T)
    torch.cuda.synchronize()

    def reference():
        with no_reuse():
            _launch(r, cam, W, H, T, d_t, n, want)
        r.sync()
        return _host(want)

    ref = reference()
    for i in range(4):
        _launch(c, cam, W, H, T, d_t, n, got)
        c.sync()
        assert same(_host(got), ref), i
    assert counts(c) == (1, 1, 2)
    assert np.array_equal(np.sort(c.order_read()), np.arange(n * 4, dtype=np.uint32))
    # other origins behind the same pointer: a stale, valid order
    d_t.copy_(torch.from_numpy(tiles[::-1].copy().view(np.uint8)).to(dev))
    torch.cuda.synchronize()
    ref2 = reference()
    assert not same(ref2, ref)
    _launch(c, cam, W, H, T, d_t, n, got)
    c.sync()
    assert same(_host(got), ref2)
    assert counts(c) == (1, 1, 3)
    c.order_reset()
    assert c.order_info()["nb"] == 0 and c.order_info()["invalidations"] == 1
    _launch(c, cam, W, H, T, d_t, n, got)
    c.sync()
    assert same(_host(got), ref2)
    assert counts(c) == (2, 1, 3)


def test_more_blocks_than_resident_waves(wgt, pair):
    """The smallest square frame whose 8 x 8 blocks outnumber the persistent grid's waves: the queue's
    refills, not only each wave's first block, then go through the shared order."""
    c, r = pair
    resident = c.scene_info()["ps_resident"]
    side = 8
    while ((side + 7) // 8) ** 2 <= resident:
        side += 1
    nb = ((side + 7) // 8) ** 2
    assert nb > resident and side < 1024
    cam = wgt.camera_param(1.0, 4, 3)
    ref = ref_tile(r, cam, side, side)
    for i in range(3):
        assert same(c.render_tile(cam, side, side), ref), i
    assert counts(c) == (1, 1, 1) and c.order_info()["nb"] == nb
    assert np.array_equal(np.sort(c.order_read()), np.arange(nb, dtype=np.uint32))


def test_frames_in_flight(wgt, pair, scene):
    """bench.py's step loop: step k on pipeline stream k % 2 into output set k % 4, nine steps, with one
    update_triangles in the middle while launches are queued.  A step's output is copied on its own
    stream right after its launch, so no step waits for the host."""
    import torch

    c, r = pair
    L, Q, S, T = scene
    W, H, TS, spp = 96, 64, 16, 16
    dev = torch.device("cuda", 0)
    cam = wgt.camera_param(W / H, spp, 0)
    tiles = wgt.tile_grid(W, H, TS, seed=4)
    n = len(tiles)
    d_t = torch.from_numpy(tiles.view(np.uint8).copy()).to(dev)
    sets = [_device_set(torch, dev, n, TS, TS) for _ in range(4)]
    want = _device_set(torch, dev, n, TS, TS)
    moved = T.copy()
    moved["v0"][:, 1] += 5.0
    torch.cuda.synchronize()
    refs = []
    for version in range(2):
        if version:
            r.update_triangles(moved)
        with no_reuse():
            _launch(r, cam, W, H, TS, d_t, n, want)
        r.sync()
        refs.append(_host(want))
    assert not same(refs[0], refs[1])
    streams = [torch.cuda.ExternalStream(c.pipeline_stream(i), device=dev) for i in range(2)]
    snaps, version_of, before = [], [], None
    for k in range(9):
        if k == 4:
            before = c.order_info()
            c.update_triangles(moved)  # waits for the queued launches, then invalidates
        s = streams[k % 2]
        _launch(c, cam, W, H, TS, d_t, n, sets[k % 4], stream=s.cuda_stream)
        with torch.cuda.stream(s):
            snaps.append({key: v.clone() for key, v in sets[k % 4].items()})
        version_of.append(1 if k >= 4 else 0)
    torch.cuda.synchronize()
    for k in range(9):
        assert same(_host(snaps[k]), refs[version_of[k]]), k
    info = c.order_info()
    assert info["invalidations"] >= 1
    assert before["reuse"] >= 1 and info["reuse"] > before["reuse"]
    assert info["today"] + info["refine"] + info["reuse"] == 9


def test_three_views_in_turn_while_launches_are_queued(wgt, pair):
    """A, A, A, B, B, C, C on the two pipeline streams with no wait in between: the host plans every
    launch while the first ones still run, so when C's second launch asks for a buffer, A's and B's
    readers have not ended and the planner's queries of the slots' events answer "not ready".  That
    launch then orders itself, and no query's answer is taken for an error of the launch.  Which
    launches had ended when they were asked about is a matter of timing, so only what holds either way
    is asserted: every output, A's and B's plans, and that no order was dropped."""
    import torch

    c, r = pair
    W, H, TS, spp = 512, 512, 32, 64
    dev = torch.device("cuda", 0)
    tiles = wgt.tile_grid(W, H, TS, seed=2)
    n = len(tiles)
    d_t = torch.from_numpy(tiles.view(np.uint8).copy()).to(dev)
    cams = {v: wgt.camera_param(W / H, spp, 0, origin=(278.0 + 40.0 * i, 278.0, -800.0)) for i, v in enumerate("ABC")}
    turn = "AAABBCC"
    sets = [_device_set(torch, dev, n, TS, TS) for _ in turn]
    want = _device_set(torch, dev, n, TS, TS)
    torch.cuda.synchronize()
    refs = {}
    for v, cam in cams.items():
        with no_reuse():
            _launch(r, cam, W, H, TS, d_t, n, want)
        r.sync()
        refs[v] = _host(want)
    streams = [c.pipeline_stream(i) for i in range(2)]
    seen = []
    for k, v in enumerate(turn):
        _launch(c, cams[v], W, H, TS, d_t, n, sets[k], stream=streams[k % 2])
        seen.append(counts(c))
    torch.cuda.synchronize()
    for k, v in enumerate(turn):
        assert same(_host(sets[k]), refs[v]), (k, v)
    # A: its own order, the kept one (both buffers unread), reuse; B: its own, then the other buffer
    assert seen[:5] == [(1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1)]
    assert seen[5] == (3, 2, 1) and seen[6] in ((4, 2, 1), (3, 3, 1))
    assert c.order_info()["invalidations"] == 0
