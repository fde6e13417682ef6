"""The denoiser (wgt_denoise_async) on device-resident buffers, timed with device events.  Needs a GPU.
Workload: one 1920x1080 frame of a mesh stand-in at default size (sponza), radiance from
render_tiles_async at `spp` samples and guides from render_gbuffer_async, both left on the device.
Sides: the whole call at iterations = 1 .. 5 (the pack pass, then that many a-trous passes, the last
of which writes the rgba32f and rgba8 outputs), in three forms of the passes chosen per call by
WGT_DENOISE_TILED_STEP: every pass a gather (0), LDS-tiled passes up to a step of 16 (their tile's
limit), and the default (tiled up to 8).  The forms' outputs are checked equal first.  Pass i's own
time is the difference of the sides i + 1 and i of a form (approximate: the two differ in which pass
carries the output's writes; the pack pass is not separable this way and is reported with pass 0).  Each side runs `reps` (>= 10) alternating repetitions of K back-to-back calls, K sized so
that a side does >= 0.5 s of work in all; the figure is the median repetition, with the minimum and
maximum beside it.  The floor of a pass is its compulsory traffic, 48 B read and 16 B written per
pixel (133 MB at 1080p), at 4 TB/s: 33 us.  Prints one JSON line per side, then one per pass.
  python scripts/denoise_probe.py [scene=sponza] [reps=10] [spp=4]"""
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
PASS_BYTES = 64 * W * H         # 3 float4 read, 1 written per pixel
FLOOR_MS = PASS_BYTES / 4e12 * 1e3


def call_floor_ms(iters):
    """The whole call's compulsory traffic at 4 TB/s: the pack pass reads the image and the five guide
    planes (57 B per pixel) and writes 48 B; the last pass also reads the albedo (12 B) and writes rgba8."""
    return (57 + 48 + 64 * iters + 16) * W * H / 4e12 * 1e3

if w.device_count() < 1:
    sys.exit("denoise_probe: no HIP device")
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
    d_tile = torch.from_numpy(np.zeros(1, TILE_DTYPE).view(np.uint8).copy()).to(dev)
    d_color = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    guides = {"prim": torch.zeros(n, dtype=torch.int32, device=dev), "flags": torch.zeros(n, dtype=torch.uint8, device=dev)}
    guides.update({k: torch.zeros((3, n), dtype=torch.float32, device=dev) for k in ("pos", "norm", "col")})
    g = {k: b.data_ptr() for k, b in guides.items()}
    ws_bytes = w.denoise_workspace_bytes(W, H)
    d_ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
    d_f32 = torch.zeros((H, W, 4), dtype=torch.float32, device=dev)
    d_u8 = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    torch.cuda.synchronize()
    ctx.render_tiles_async(cam, W, H, W, H, d_tile.data_ptr(), 1, d_f32=d_color.data_ptr(), stream=s)
    ctx.render_gbuffer_async(cam, W, H, W, H, d_tile.data_ptr(), 1, stream=s, **g)
    stream.synchronize()

    def side(form, iters):
        def go():
            os.environ["WGT_DENOISE_TILED_STEP"] = form  # read per call: the largest LDS-tiled step
            ctx.denoise_async(W, H, d_color.data_ptr(), d_ws.data_ptr(), ws_bytes, d_f32_out=d_f32.data_ptr(),
                              d_u8_out=d_u8.data_ptr(), iterations=iters, stream=s, **g)
        return go

    FORMS = {"0": "gather", "16": "lds_tiled_to_16", "8": "default_tiled_to_8"}
    sides = [((f, i), side(f, i)) for i in range(1, 6) for f in FORMS]
    k, result = {}, {}
    for key, go in sides:  # warm-up, and K per side from one timed run
        timed(stream, go, 2)
        k[key] = max(1, math.ceil(500.0 / (reps * timed(stream, go, 3))))
        result[key] = (d_f32.clone(), d_u8.clone())
    for i in range(1, 6):  # the forms compute the same bits
        for f in ("16", "8"):
            assert torch.equal(result[("0", i)][0].view(torch.int32), result[(f, i)][0].view(torch.int32))
            assert torch.equal(result[("0", i)][1], result[(f, i)][1])
    ms = {key: [] for key, _ in sides}
    for _ in range(reps):  # alternating
        for key, go in sides:
            ms[key].append(timed(stream, go, k[key]))
    valid = int((guides["prim"] != -1).sum().item())
    med = {key: float(np.median(v)) for key, v in ms.items()}
    for (f, i), _ in sides:
        key = (f, i)
        print(json.dumps({"scene": scene, "spp": spp, "form": FORMS[f], "side": f"iterations_{i}", "pixels": n,
                          "hit_pixels": valid, "ms": round(med[key], 4), "ms_min": round(min(ms[key]), 4),
                          "ms_max": round(max(ms[key]), 4), "floor_ms": round(call_floor_ms(i), 4),
                          "floor_fraction": round(call_floor_ms(i) / med[key], 3), "reps": reps,
                          "calls_per_rep": k[key], "build_id": w.build_id()}), flush=True)
    for f in FORMS:
        for i in range(1, 5):  # pass i (step 2^i), by difference, repetition by repetition
            diff = [b - a for a, b in zip(ms[(f, i)], ms[(f, i + 1)])]
            m = float(np.median(diff))
            print(json.dumps({"scene": scene, "form": FORMS[f], "pass": i, "step": 1 << i, "ms": round(m, 4),
                              "ms_min": round(min(diff), 4), "ms_max": round(max(diff), 4), "floor_ms": round(FLOOR_MS, 4),
                              "floor_fraction": round(FLOOR_MS / m, 3) if m > 0 else None}), flush=True)
        print(json.dumps({"scene": scene, "form": FORMS[f], "pass": "pack + pass 0 (step 1)", "ms": round(med[(f, 1)], 4),
                          "ms_min": round(min(ms[(f, 1)]), 4), "ms_max": round(max(ms[(f, 1)]), 4)}), flush=True)
