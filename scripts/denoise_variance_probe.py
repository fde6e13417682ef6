"""The variance-guided denoiser (wgt_denoise_variance_async) on device-resident buffers, timed with
device events, with the plain filter (wgt_denoise_async) on the same frame as the baseline.  Needs a GPU.
Workload: 1920x1080 frames of a mesh stand-in at default size (sponza) under one camera, radiance from
render_tiles_async at `spp` samples and guides from render_gbuffer_async, accumulated on the device by
temporal_accumulate_async: the state after `frames` frames (a long history: every accumulated pixel
takes its variance from its own moments) and the state after the first frame alone (the 7 x 7 spatial
estimate runs on every accumulated pixel).
Sides: the whole call (rgba32f, rgba8 and variance outputs) at iterations = 1 .. 5; on the long history
in three forms of the passes chosen per call by WGT_DENOISE_TILED_STEP: every pass a gather (0),
LDS-tiled passes up to a step of 16 (their tile's limit), and the default (tiled up to 8); on the
first frame in the default form; and wgt_denoise_async of the long history's radiance in its default
form.  The forms' outputs are checked equal first.  Each side runs `reps` (>= 10) alternating
repetitions of K back-to-back calls, K sized so that a side does >= 0.3 s of work in all; the figure is
the median repetition, with the minimum and maximum beside it.  The floor is the call's compulsory
traffic at 4 TB/s, per pixel: the pack pass reads the state (28 B) and the guides (41 B) and writes
48 B, the spatial pass reads a record's tag (16 B), each a-trous pass reads 48 B and writes 16 B, the
last one also reads the albedo and the input's alpha (28 B) and writes rgba8 and the variance (8 B); on
the first frame the spatial pass reads 60 B and writes 4 B.  Prints one JSON line per side.
  python scripts/denoise_variance_probe.py [scene=sponza] [reps=10] [spp=4] [frames=8]"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import webgputracer_amd as w  # noqa: E402
from webgputracer_amd._lib import TILE_DTYPE  # noqa: E402

scene = sys.argv[1] if len(sys.argv) > 1 else "sponza"
reps = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 10
spp = int(sys.argv[3]) if len(sys.argv) > 3 else 4
frames = int(sys.argv[4]) if len(sys.argv) > 4 else 8
W, H = 1920, 1080


def floor_ms(kind, iters):
    per_pixel = {"long": 69 + 48 + 16 + 64 * iters + 28 + 8, "first": 69 + 48 + 60 + 4 + 64 * iters + 28 + 8,
                 "plain": 57 + 48 + 64 * iters + 16}[kind]
    return per_pixel * W * H / 4e12 * 1e3


if w.device_count() < 1:
    sys.exit("denoise_variance_probe: no HIP device")
dev = torch.device("cuda", 0)


def timed(stream, launch, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(k):
        launch()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / k  # ms per call


with w.Context(0) as ctx:
    ctx.upload_scene(*w.mesh_scene(scene))
    n = W * H
    cam = w.camera_param(W / H, spp, 0)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream

    def guide_set():
        t = {"prim": torch.zeros(n, dtype=torch.int32, device=dev), "flags": torch.zeros(n, dtype=torch.uint8, device=dev)}
        t.update({k: torch.zeros((3, n), dtype=torch.float32, device=dev) for k in ("pos", "norm", "col")})
        return t, {k: b.data_ptr() for k, b in t.items()}

    def state():
        t = {"f32": torch.zeros((H, W, 4), dtype=torch.float32, device=dev),
             "len": torch.zeros(n, dtype=torch.float32, device=dev),
             "moments": torch.zeros((2, n), dtype=torch.float32, device=dev)}
        return t, {k: b.data_ptr() for k, b in t.items()}

    # the sequence: two guide sets and two states alternate, the first frame's state is kept aside
    gsets, states = [guide_set(), guide_set()], [state(), state()]
    first_t, first = state()
    d_color = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    for f in range(frames):
        tile = np.zeros(1, TILE_DTYPE)
        tile["seed"] = f
        d_tile = torch.from_numpy(tile.view(np.uint8).copy()).to(dev)
        q = f % 2
        torch.cuda.synchronize()
        ctx.render_tiles_async(cam, W, H, W, H, d_tile.data_ptr(), 1, d_f32=d_color.data_ptr(), stream=s)
        ctx.render_gbuffer_async(cam, W, H, W, H, d_tile.data_ptr(), 1, stream=s, **gsets[q][1])
        ctx.temporal_accumulate_async(W, H, cam, d_color.data_ptr(), gsets[q][1], states[q][1],
                                      states[1 - q][1] if f else None, gsets[1 - q][1] if f else None, cam if f else None,
                                      max_history=65536, stream=s)
        stream.synchronize()
        if f == 0:
            for key in first_t:
                first_t[key].copy_(states[0][0][key])
            g_first_t, g_first = guide_set()
            for key in g_first_t:
                g_first_t[key].copy_(gsets[0][0][key])
    last = (frames - 1) % 2
    long_t, long = states[last]
    g_long = gsets[last][1]
    ws_bytes = max(w.denoise_variance_workspace_bytes(W, H), w.denoise_workspace_bytes(W, H))
    d_ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    d_f32 = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    d_u8 = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    d_var = torch.zeros(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def side(kind, form, iters):
        def go():
            os.environ["WGT_DENOISE_TILED_STEP"] = form  # read per call: the largest LDS-tiled step
            if kind == "plain":
                ctx.denoise_async(W, H, long["f32"], d_ws.data_ptr(), ws_bytes, d_f32_out=d_f32.data_ptr(),
                                  d_u8_out=d_u8.data_ptr(), iterations=iters, stream=s, **g_long)
            else:
                ctx.denoise_variance_async(W, H, long if kind == "long" else first, d_ws.data_ptr(), ws_bytes,
                                           d_f32_out=d_f32.data_ptr(), d_u8_out=d_u8.data_ptr(),
                                           d_var_out=d_var.data_ptr(), iterations=iters, stream=s,
                                           **(g_long if kind == "long" else g_first))
        return go

    FORMS = {"0": "gather", "16": "lds_tiled_to_16", "8": "default_tiled_to_8"}
    keys = [("long", f, i) for i in range(1, 6) for f in FORMS]
    keys += [(kind, "8", i) for i in range(1, 6) for kind in ("first", "plain")]
    sides = [(key, side(*key)) for key in keys]
    k, result = {}, {}
    for key, go in sides:  # warm-up, and K per side from one timed run
        timed(stream, go, 2)
        k[key] = max(1, math.ceil(300.0 / (reps * timed(stream, go, 3))))
        result[key] = (d_f32.clone(), d_u8.clone(), d_var.clone())
    for i in range(1, 6):  # the forms compute the same bits
        for f in ("16", "8"):
            for a, b in zip(result[("long", "0", i)], result[("long", f, i)]):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), (f, i)
    ms = {key: [] for key in keys}
    for _ in range(reps):  # alternating
        for key, go in sides:
            ms[key].append(timed(stream, go, k[key]))
    med = {key: float(np.median(v)) for key, v in ms.items()}
    lens = {"long": long_t["len"], "first": first_t["len"], "plain": long_t["len"]}
    for key in keys:
        kind, f, i = key
        ln = lens[kind]
        line = {"scene": scene, "spp": spp, "call": "wgt_denoise_async" if kind == "plain" else "wgt_denoise_variance_async",
                "history": "first" if kind == "first" else "long", "frames": 1 if kind == "first" else frames,
                "form": FORMS[f], "side": f"iterations_{i}", "pixels": n, "accumulated": int((ln > 0).sum().item()),
                "short_history": int(((ln > 0) & (ln < 4)).sum().item()) if kind != "plain" else None,
                "ms": round(med[key], 4), "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4),
                "plain_ms": round(med[("plain", "8", i)], 4),
                "ratio_to_plain": round(med[key] / med[("plain", "8", i)], 3),
                "floor_ms": round(floor_ms(kind, i), 4), "floor_fraction": round(floor_ms(kind, i) / med[key], 3),
                "reps": reps, "calls_per_rep": k[key], "build_id": w.build_id()}
        print(json.dumps(line), flush=True)
