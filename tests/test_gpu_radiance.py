"""The radiance queries (wgt_trace_radiance and its forms) on the GPU.  Every comparison
is bit for bit.  The oracle stays as it is and still pins the feature: a frame at spp = 1 is, per pixel, one
path along the ray the G-buffer pass exports, from the state two rand() past the pixel's seed.  Rays no
camera produces are pinned to the numpy restatement (tests/radiance_restatement.py, itself pinned to the
oracle on the CPU), the launch forms to one another and to the flat kernel."""
import os

import numpy as np
import pytest

import adversarial_meshes as am
import radiance_restatement as rr
import refit_cases as rc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NO_HIT = 0xFFFFFFFF
KNOBS = ("WGT_CNODE", "WGT_KERNEL", "WGT_PS_WAVES", "WGT_PARK", "WGT_PS_CAP", "WGT_NARROW")
FORMS = {"default": {}, "128B": {"WGT_CNODE": "0"}, "simple": {"WGT_KERNEL": "1"}, "5waves": {"WGT_PS_WAVES": "5"}}
FIELDS = ("rgb", "prim", "seed")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same(got, want, what=""):
    for k in want:
        bad = np.flatnonzero((bits(got[k]) != bits(want[k])).reshape(len(want[k]), -1).any(axis=1))
        assert bad.size == 0, f"{what}: {k} differs on {bad.size} of {len(want[k])} rays; first: ray {bad[0]}: " \
                              f"{got[k][bad[0]]} != {want[k][bad[0]]}"


def _set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def pixel_seeds(W, H, seed):
    x, y = np.meshgrid(np.arange(W, dtype=np.uint32), np.arange(H, dtype=np.uint32))
    with np.errstate(over="ignore"):
        return x + y * np.uint32(W) + np.uint32(seed) * np.uint32(W) * np.uint32(H)


def frame_by_query(ctx, cam, W, H, seed, **kw):
    """The frame of `cam` at one sample per pixel through the query: the G-buffer's rays, the state two
    draws past each pixel's seed."""
    g = ctx.render_gbuffer(cam, W, H, want=("prim",), rays=True)
    r = ctx.trace_radiance(g["origin"].reshape(-1, 3), g["direction"].reshape(-1, 3),
                           seeds=rr.advance(pixel_seeds(W, H, seed), 2).ravel(), samples=1, **kw)
    return g, r


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    t = torch.from_numpy(a.copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def _dev_words(n_words, fill=0x5A5A5A5A):
    import torch

    return torch.full((n_words,), fill, dtype=torch.int64, device=torch.device("cuda", 0)).to(torch.int32)


def _host_words(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def bunny():
    d = np.load(os.path.join(HERE, "golden", "bunny2000_48x27_spp1_seed3.npz"))
    return (d["lights"], d["quads"], d["spheres"], d["tris"]), d["f32"], d["hit"]


def test_oracle_pin_on_a_mesh(ctx, wgt, bunny, monkeypatch):
    """1. The golden bunny frame (the oracle's, 48 x 27, spp 1, seed 3): rgb and prim of the query on the
    G-buffer's rays equal it, and ctx.render_tile's frame.  Fails without the feature."""
    _set_env(monkeypatch, {})
    scene, f32, hit = bunny
    ctx.upload_scene(*scene)
    cam = wgt.camera_param(48 / 27, 1, 3)
    g, r = frame_by_query(ctx, cam, 48, 27, 3)
    assert np.array_equal(bits(r["rgb"]).reshape(27, 48, 3), bits(f32[..., :3]))
    assert np.array_equal(r["prim"].reshape(27, 48), hit) and np.array_equal(g["prim"], hit)
    t = ctx.render_tile(cam, 48, 27)
    assert np.array_equal(bits(r["rgb"]).reshape(27, 48, 3), bits(t["f32"][..., :3]))
    assert np.array_equal(r["prim"].reshape(27, 48), t["hit"])


@pytest.mark.parametrize("emissive", [False, True])
def test_oracle_pin_without_triangles(ctx, wgt, oracle, emissive, monkeypatch):
    """2. The Cornell box at 16 x 16, as uploaded and with an emissive last sphere (NaN rays are then
    shaded, not skipped): the frame and the stats form's four counts equal the oracle's."""
    _set_env(monkeypatch, {})
    L, Q, S = wgt.cornell_scene()
    if emissive:  # the scene of test_gpu_parity.test_emissive_last_sphere_no_skip
        S = np.concatenate([S, S])
        S[1]["center"] = (278.0, 100.0, 278.0)
        S[1]["radius"] = 60.0
        S[1]["col"] = (2.0, 1.0, 0.5)
        S[1]["emissive"] = 1.0
    W = H = 16
    ctx.upload_scene(L, Q, S)
    ref = oracle.OracleScene(L, Q, S).render(oracle.camera_param(1.0, 1, 5), W, H)
    g, r = frame_by_query(ctx, wgt.camera_param(1.0, 1, 5), W, H, 5)
    assert np.array_equal(bits(r["rgb"]).reshape(H, W, 3), bits(ref["f32"][..., :3]))
    assert np.array_equal(r["prim"].reshape(H, W), ref["hit"])
    assert int(ref["counters"][oracle.CNT_NAN_RAYS]) > 0
    soa = np.concatenate([g["origin"].reshape(-1, 3).T, g["direction"].reshape(-1, 3).T])
    d_rays, d_seeds, d_rgb = _dev(soa), _dev(rr.advance(pixel_seeds(W, H, 5), 2).ravel()), _dev_words(3 * W * H)
    counts = ctx.trace_radiance_stats(d_rays.data_ptr(), W * H, d_seeds=d_seeds.data_ptr(), samples=1, rgb=d_rgb.data_ptr())
    assert list(counts) == [int(ref["counters"][k]) for k in
                            (oracle.CNT_QUERIES, oracle.CNT_TRACED, oracle.CNT_SAMPLES, oracle.CNT_NAN_RAYS)]
    assert np.array_equal(_host_words(d_rgb).reshape(3, -1).T, bits(r["rgb"]))  # the counting kernel's answers


def hard_rays():
    """3. 257 rays no pinhole camera produces, in the Cornell box: origins inside it, directions over the
    whole sphere, every eighth with a length from 2^-20 to 2^20, three with a NaN component, three that
    miss everything (from in front of the open side, away from it)."""
    rng = np.random.default_rng(14)
    n = 257
    o = rng.uniform(1.0, 554.0, (n, 3)).astype(np.float32)
    d = rng.normal(0.0, 1.0, (n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    k = np.arange(0, n, 8)
    d[k] *= (2.0 ** np.linspace(-20, 20, len(k))).astype(np.float32)[:, None]
    o[3, 0] = d[100, 1] = d[200, 2] = np.nan
    o[5:8] = (278.0, 278.0, -100.0)
    d[5:8] = ((0.0, 0.0, -1.0), (0.3, 0.2, -2.0), (-1e-3, 0.0, -1e-3))
    return o, d, rng.integers(0, 2 ** 32, n, dtype=np.uint32)


@pytest.fixture(scope="module")
def hard_paths(wgt):
    """The restatement's four paths per hard ray, computed once: every sample count combines them."""
    L, Q, S = wgt.cornell_scene()
    o, d, seeds = hard_rays()
    return (L, Q, S), (o, d, seeds), rr.trace_paths(L, Q, S, o, d, seeds, 4)


@pytest.mark.parametrize("samples", [1, 2, 3, 4, 0])
def test_restatement_pin(ctx, hard_paths, samples, monkeypatch):
    """3. rgb, prim and the final seed equal the restatement for 1 to 4 samples (3: the division, f32(3) is
    no power of two) and for none (zero colour, no primitive, the seed unchanged)."""
    _set_env(monkeypatch, {})
    scene, (o, d, seeds), (cols, prim, states) = hard_paths
    ctx.upload_scene(*scene)
    got = ctx.trace_radiance(o, d, seeds=seeds, samples=samples)
    want = {"rgb": rr.combine(cols, samples, len(o)), "prim": prim if samples else np.full(len(o), NO_HIT, np.uint32),
            "seed": states[samples]}
    assert_same(got, want, f"{samples} samples")
    if samples == 1:
        assert (prim[5:8] == NO_HIT).all() and (prim[[3, 100, 200]] == len(scene[0]) + len(scene[1])).all()
        assert not np.isnan(got["rgb"]).any()


def test_composition(ctx, wgt, bunny, monkeypatch):
    """4. 4,097 rays on the bunny (the G-buffer's, tiled): one call with three samples equals three chained
    one-sample calls summed on the host in fp32 in order; seeds = NULL with seed0 = 7 is seeds 7 + i."""
    _set_env(monkeypatch, {})
    scene, _, _ = bunny
    ctx.upload_scene(*scene)
    g = ctx.render_gbuffer(wgt.camera_param(48 / 27, 1, 3), 48, 27, want=("prim",), rays=True)
    n = 4097
    k = np.arange(n) % (48 * 27)
    o, d = g["origin"].reshape(-1, 3)[k], g["direction"].reshape(-1, 3)[k]
    seeds = np.random.default_rng(15).integers(0, 2 ** 32, n, dtype=np.uint32)
    once = ctx.trace_radiance(o, d, seeds=seeds, samples=3)
    acc, s = np.zeros((n, 3), np.float32), seeds
    for j in range(3):
        c = ctx.trace_radiance(o, d, seeds=s, samples=1)
        acc, s = acc + c["rgb"] / np.float32(3), c["seed"]
        assert j or np.array_equal(c["prim"], once["prim"])
    assert_same({"rgb": acc, "seed": s}, {"rgb": once["rgb"], "seed": once["seed"]}, "chained")
    assert (once["seed"] != seeds).any() and once["rgb"].any()
    assert_same(ctx.trace_radiance(o, d, seed0=7, samples=2),
                ctx.trace_radiance(o, d, seeds=(np.uint32(7) + np.arange(n, dtype=np.uint32)), samples=2), "seed0")
    top = ctx.trace_radiance(o[:3], d[:3], seed0=0xFFFFFFFE, samples=1)  # seed0 + i wraps around
    assert_same(top, ctx.trace_radiance(o[:3], d[:3], seeds=np.array([0xFFFFFFFE, 0xFFFFFFFF, 0], np.uint32), samples=1), "wrap")


def form_rays(name):
    if name == "nodes_65536":
        o, d = am.limit_rays(name)
    else:
        o, d = am.aimed_rays(am.small_mesh(name), 1000, 3)
    return o, d, np.random.default_rng(16).integers(0, 2 ** 32, len(o), dtype=np.uint32)


@pytest.mark.parametrize("name", ["nodes_65536", "geometric_up"])
def test_every_launch_form_agrees(ctx, name, monkeypatch):
    """5. 1,000 rays, two samples, on the tree whose refs need the 4-byte stack entry (65,536 nodes: 5 waves)
    and on the one at the builder's depth and stack limits: the persistent kernel on 80-B and 128-B nodes,
    at 6 and at 5 waves, and the flat kernel give identical outputs; the first hits are trace_rays'."""
    L, Q, S = am.scene_parts(name)
    T = am.limit_mesh(name) if name in am.LIMITS else am.small_mesh(name)
    o, d, seeds = form_rays(name)
    got = {}
    for form in ("simple", "default", "128B", "5waves"):
        _set_env(monkeypatch, FORMS[form])
        if form in ("simple", "5waves"):  # the waves per SIMD are the upload's decision
            ctx.upload_scene(L, Q, S, T)
            waves = ctx.scene_info()["ps_waves"]
            assert waves == (5 if form == "5waves" or name == "nodes_65536" else 6)
        got[form] = ctx.trace_radiance(o, d, seeds=seeds, samples=2)
    for form in ("default", "128B", "5waves"):
        assert_same(got[form], got["simple"], f"{name}: {form} against the flat kernel")
    prim, _ = ctx.trace_rays(o, d)
    assert np.array_equal(got["simple"]["prim"], prim)
    nlq = len(L) + len(Q)
    assert np.mean((prim >= nlq) & (prim < nlq + len(T))) > 0.3 and (got["simple"]["seed"] != seeds).any()


def test_a_form_with_a_short_lds_stack_is_refused(ctx, wgt, monkeypatch):
    """5d. The radiance kernel has no parked form: on a scene uploaded with WGT_PARK and an LDS stack shorter
    than the tree's, the persistent launch is refused with a status and never queued; the flat kernel answers."""
    name = "geometric_up"
    L, Q, S = am.scene_parts(name)
    o, d, seeds = form_rays(name)
    _set_env(monkeypatch, {"WGT_PARK": "1", "WGT_PS_CAP": "8"})
    ctx.upload_scene(L, Q, S, am.small_mesh(name))
    info = ctx.scene_info()
    assert info["ps_park"] and info["ps_stack"] == 8 < info["bvh_stack"]
    with pytest.raises(wgt.tracer.WgtError) as e:
        ctx.trace_radiance(o, d, seeds=seeds, samples=2)
    assert "no parked form" in str(e.value)
    monkeypatch.setenv("WGT_KERNEL", "1")
    flat = ctx.trace_radiance(o, d, seeds=seeds, samples=2)
    _set_env(monkeypatch, {})
    ctx.upload_scene(L, Q, S, am.small_mesh(name))
    assert_same(ctx.trace_radiance(o, d, seeds=seeds, samples=2), flat, "unparked upload")


def test_origins_beyond_the_compact_bound(ctx, wgt, bunny, monkeypatch):
    """5b. The 80-B records hold for ray origins within the scene's bound; a batch with an origin beyond it
    runs on the 128-B nodes, decided on the device: identical to the flat kernel, batch by batch."""
    scene, _, _ = bunny
    _set_env(monkeypatch, {})
    ctx.upload_scene(*scene)
    g = ctx.render_gbuffer(wgt.camera_param(48 / 27, 1, 3), 48, 27, want=("prim",), rays=True)
    o, d = g["origin"].reshape(-1, 3).copy(), g["direction"].reshape(-1, 3)
    far = o.copy()
    far[::7] += d[::7] * np.float32(-1000.0)  # the same lines of sight from 1000 times further back: |z| ~ 1e6
    assert np.abs(far).max() > 1e5
    for name, org in (("near", o), ("far", far)):
        _set_env(monkeypatch, {})
        a = ctx.trace_radiance(org, d, seed0=3, samples=2)
        _set_env(monkeypatch, FORMS["simple"])
        assert_same(a, ctx.trace_radiance(org, d, seed0=3, samples=2), name)
        assert np.array_equal(a["prim"], ctx.trace_rays(org, d)[0])


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_batches_leave_the_guard_words(ctx, wgt, bunny, n, monkeypatch):
    """5c. n around the wave size on the default form, device buffers with 64 guard words behind each:
    the first n rays' answers, nothing written past them."""
    _set_env(monkeypatch, {})
    scene, _, _ = bunny
    ctx.upload_scene(*scene)
    g = ctx.render_gbuffer(wgt.camera_param(48 / 27, 1, 3), 48, 27, want=("prim",), rays=True)
    o, d = g["origin"].reshape(-1, 3)[500:500 + n], g["direction"].reshape(-1, 3)[500:500 + n]
    want = ctx.trace_radiance(o, d, seed0=11, samples=2)
    d_rays = _dev(np.concatenate([o.T, d.T]))
    out = {"rgb": _dev_words(3 * n + 64), "prim": _dev_words(n + 64), "seed": _dev_words(n + 64)}
    ctx.trace_radiance_async(d_rays.data_ptr(), n, seed0=11, samples=2, **{k: t.data_ptr() for k, t in out.items()})
    import torch

    torch.cuda.synchronize()
    host = {k: _host_words(t) for k, t in out.items()}
    for k, words in (("rgb", 3 * n), ("prim", n), ("seed", n)):
        assert (host[k][words:] == 0x5A5A5A5A).all(), k
    assert np.array_equal(host["rgb"][:3 * n].reshape(3, n).T, bits(want["rgb"]))
    assert np.array_equal(host["prim"][:n], want["prim"]) and np.array_equal(host["seed"][:n], want["seed"])


def test_follows_the_scene(ctx, wgt, monkeypatch):
    """6. After update_triangles and after rebuild_triangles the answers equal a fresh upload's."""
    _set_env(monkeypatch, {})
    L, Q, S, _ = wgt.mesh_scene("bunny", 2000)
    A = rc.mesh("bunny2000")
    B = rc.moved("bunny2000", "jitter5")
    o, d = am.aimed_rays(A, 1500, 5)

    def ask():
        return ctx.trace_radiance(o, d, seed0=21, samples=2)

    ctx.upload_scene(L, Q, S, B)
    fresh_b = ask()
    ctx.upload_scene(L, Q, S, A[::4])
    fresh_c = ask()
    ctx.upload_scene(L, Q, S, A)
    fresh_a = ask()
    ctx.update_triangles(B)
    assert_same(ask(), fresh_b, "after update_triangles")
    ctx.rebuild_triangles(A[::4])
    assert_same(ask(), fresh_c, "after rebuild_triangles")
    assert (bits(fresh_a["rgb"]) != bits(fresh_b["rgb"])).any() and (fresh_a["prim"] != fresh_c["prim"]).any()


def test_async_on_a_caller_stream_with_any_subset_of_outputs(ctx, wgt, bunny, monkeypatch):
    """7. Device pointers on a pipeline stream; every non-empty subset of the three outputs: the fields
    asked for equal the synchronous call's, the others keep their fill pattern."""
    import torch

    _set_env(monkeypatch, {})
    scene, _, _ = bunny
    ctx.upload_scene(*scene)
    g = ctx.render_gbuffer(wgt.camera_param(48 / 27, 1, 3), 48, 27, want=("prim",), rays=True)
    o, d = g["origin"].reshape(-1, 3), g["direction"].reshape(-1, 3)
    n = len(o)
    seeds = np.random.default_rng(17).integers(0, 2 ** 32, n, dtype=np.uint32)
    want = ctx.trace_radiance(o, d, seeds=seeds, samples=2)
    want = {"rgb": bits(want["rgb"]).T.ravel(), "prim": want["prim"], "seed": want["seed"]}
    d_rays, d_seeds = _dev(np.concatenate([o.T, d.T])), _dev(seeds)
    s = ctx.pipeline_stream(1)
    for mask in range(1, 8):
        out = {"rgb": _dev_words(3 * n), "prim": _dev_words(n), "seed": _dev_words(n)}
        asked = [k for i, k in enumerate(FIELDS) if mask >> i & 1]
        ctx.trace_radiance_async(d_rays.data_ptr(), n, d_seeds=d_seeds.data_ptr(), samples=2, stream=s,
                                 **{k: out[k].data_ptr() for k in asked})
        torch.cuda.synchronize()
        for k in FIELDS:
            h = _host_words(out[k])
            assert np.array_equal(h, want[k]) if k in asked else (h == 0x5A5A5A5A).all(), (mask, k)


def test_refusals_in_order(ctx, wgt, monkeypatch):
    """The entry points' refusals behind the scene check: n == 0 succeeds whatever else is passed; then
    each refusal names its argument and nothing is written."""
    import ctypes

    from webgputracer_amd import _lib

    _set_env(monkeypatch, {})
    ctx.upload_scene(*wgt.cornell_scene())
    L = _lib.lib()
    rays = np.zeros((6, 2), np.float32)
    prim = np.full(2, 123, np.uint32)
    some, none = _lib.WgtRadianceBuffers(prim=prim.ctypes.data), _lib.WgtRadianceBuffers()
    p = _lib.ptr
    assert L.wgt_trace_radiance(ctx.h, None, None, 0, 1 << 20, 0, None) == _lib.WGT_OK
    for args, text in (((None, None, 0, 1 << 20, 2, None), b"null rays"),
                       ((p(rays), None, 0, 1 << 20, 2, None), b"null output buffers"),
                       ((p(rays), None, 0, 1 << 20, 2, ctypes.byref(none)), b"no radiance field"),
                       ((p(rays), None, 0, 65537, 2, ctypes.byref(some)), b"too many samples")):
        assert L.wgt_trace_radiance(ctx.h, *args) == _lib.WGT_E_INVALID
        assert text in L.wgt_last_error(ctx.h), L.wgt_last_error(ctx.h)
        assert (prim == 123).all()
    assert L.wgt_trace_radiance_stats(ctx.h, p(rays), None, 0, 1, 2, ctypes.byref(some), None) == _lib.WGT_E_INVALID
    assert b"null counts" in L.wgt_last_error(ctx.h)
    with pytest.raises(ValueError):
        ctx.trace_radiance(rays.T[:, :3], rays.T[:, 3:], want=("dist",))


def test_panorama_cli(ctx, wgt, tmp_path, monkeypatch):
    """8. `frames --panorama` at 64 x 32 with --spp 4 writes NNN_pano.png, which decodes to the unorm8 store
    of trace_radiance on the same rays and seeds."""
    from PIL import Image

    from webgputracer_amd import frames

    _set_env(monkeypatch, {})
    obj = tmp_path / "mesh.obj"
    wgt.write_obj(str(obj), wgt.procedural_mesh("bunny", 2000))
    frames.main(["--frame", "2", "2", "--width", "64", "--spp", "4", "--scene", f"obj:{obj}", "--panorama",
                 "--out", str(tmp_path)])
    assert sorted(p.name for p in tmp_path.glob("*.png")) == ["001_pano.png"]
    img = np.asarray(Image.open(tmp_path / "001_pano.png").convert("RGBA"))
    ctx.upload_scene(*wgt.mesh_scene("bunny", obj_path=str(obj)))
    W, H = 64, 32
    d = frames.panorama_directions(W, H).reshape(-1, 3)
    o = np.broadcast_to(np.array([278.0, 278.0, -800.0], np.float32), d.shape)
    rgb = ctx.trace_radiance(o, d, seeds=pixel_seeds(W, H, 1).ravel(), samples=4, want=("rgb",))["rgb"]
    assert img.shape == (H, W, 4) and (img[..., 3] == 255).all()
    assert np.array_equal(img[..., :3], frames.unorm8(rgb).reshape(H, W, 3))
    assert len(np.unique(img[..., :3])) > 16  # an image, not a constant
