"""Temporal accumulation (wgt_temporal_accumulate_async) on device-resident buffers, timed with device
events.  Needs a GPU.
Workload: 1920x1080 frames of a mesh stand-in at default size (sponza), radiance from
render_tiles_async at `spp` samples and guides from render_gbuffer_async, all left on the device:
frame A (the reference camera, seed 0), frame A' (the same camera, seed 1) and frame B (the origin
moved by a few units, seed 1).  Sides, each one call with moments and the rgba8 output:
  static : A' over the state of A, identical cameras: every pixel reads its own pixel, one live tap
  moving : B over the state of A: fractional history coordinates, four live taps
  first  : the first-frame form on A
The probe first checks that a second run of each side gives equal bits.  Each side runs `reps` (>= 10)
alternating repetitions of K back-to-back calls, K sized so that a side does >= 0.5 s of work in all;
the figure is the median repetition, with the minimum and maximum beside it.  The floor is the call's
compulsory traffic at 4 TB/s, per pixel: the colour (16 B) and the guides' prim, flags, pos and norm
(29 B) read, rgba32f, len, two moments and rgba8 (32 B) written: 77 B for the first frame; with a
history also its rgba32f, len and moments (28 B) and its guides (29 B): 134 B.  Prints one JSON line
per side.
  python scripts/temporal_probe.py [scene=sponza] [reps=10] [spp=4]"""
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
W, H = 1920, 1080
BYTES = {"static": 134, "moving": 134, "first": 77}  # compulsory traffic per pixel

if w.device_count() < 1:
    sys.exit("temporal_probe: no HIP device")
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
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream

    def frame(cam, seed):
        """A rendered frame on the device: its colour tensor, its guide tensors and their addresses."""
        tile = np.zeros(1, TILE_DTYPE)
        tile["seed"] = seed
        d_tile = torch.from_numpy(tile.view(np.uint8).copy()).to(dev)
        color = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
        guides = {"prim": torch.zeros(n, dtype=torch.int32, device=dev), "flags": torch.zeros(n, dtype=torch.uint8, device=dev)}
        guides.update({k: torch.zeros((3, n), dtype=torch.float32, device=dev) for k in ("pos", "norm")})
        g = {k: b.data_ptr() for k, b in guides.items()}
        torch.cuda.synchronize()
        ctx.render_tiles_async(cam, W, H, W, H, d_tile.data_ptr(), 1, d_f32=color.data_ptr(), stream=s)
        ctx.render_gbuffer_async(cam, W, H, W, H, d_tile.data_ptr(), 1, stream=s, **g)
        stream.synchronize()
        return color, guides, g

    def state():
        t = {"f32": torch.zeros((H, W, 4), dtype=torch.float32, device=dev),
             "len": torch.zeros(n, dtype=torch.float32, device=dev),
             "moments": torch.zeros((2, n), dtype=torch.float32, device=dev)}
        return t, {k: b.data_ptr() for k, b in t.items()}

    cam_a = w.camera_param(W / H, spp, 0)
    cam_b = w.camera_param(W / H, spp, 0, origin=(278.0 + 4.3, 278.0 - 2.9, -800.0 + 1.7))
    A, A1, B = frame(cam_a, 0), frame(cam_a, 1), frame(cam_b, 1)
    (hist_t, hist), (out_t, out) = state(), state()
    d_u8 = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.temporal_accumulate_async(W, H, cam_a, A[0].data_ptr(), A[2], hist, stream=s)
    stream.synchronize()

    def side(cur, cam, first):
        def go():
            ctx.temporal_accumulate_async(W, H, cam, cur[0].data_ptr(), cur[2], out, None if first else hist,
                                          None if first else A[2], None if first else cam_a, d_u8_out=d_u8.data_ptr(),
                                          max_history=65536, stream=s)
        return go

    sides = [("static", side(A1, cam_a, False)), ("moving", side(B, cam_b, False)), ("first", side(A, cam_a, True))]
    k, lens = {}, {}
    for key, go in sides:  # warm-up, equal bits of two runs, and K per side from one timed run
        timed(stream, go, 2)
        first_run = [t.clone() for t in out_t.values()] + [d_u8.clone()]
        out_t["f32"].fill_(-1.0)
        torch.cuda.synchronize()
        k[key] = max(1, math.ceil(500.0 / (reps * timed(stream, go, 3))))
        for a, b in zip(first_run, list(out_t.values()) + [d_u8]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), key
        ln = out_t["len"]
        lens[key] = {"accumulated": int((ln > 0).sum().item()), "with_history": int((ln > 1).sum().item())}
    ms = {key: [] for key, _ in sides}
    for _ in range(reps):  # alternating
        for key, go in sides:
            ms[key].append(timed(stream, go, k[key]))
    for key, _ in sides:
        med = float(np.median(ms[key]))
        floor = BYTES[key] * n / 4e12 * 1e3
        print(json.dumps({"scene": scene, "spp": spp, "side": key, "pixels": n, **lens[key], "ms": round(med, 4),
                          "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4),
                          "bytes_per_pixel": BYTES[key], "floor_ms": round(floor, 4),
                          "floor_fraction": round(floor / med, 3), "reps": reps, "calls_per_rep": k[key],
                          "build_id": w.build_id()}), flush=True)
