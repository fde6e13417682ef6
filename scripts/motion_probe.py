"""The motion passes (wgt_motion_snapshot, wgt_motion_reproject_async,
wgt_temporal_accumulate_motion_async) on device-resident buffers, timed with device events.  Needs a GPU.
Workload: 1920x1080 frames of a mesh stand-in at default size (sponza) whose every vertex is jittered
by a seeded 5 % of the mesh's size per frame through wgt_update_vertices_device (scripts/refit_probe.py's
motion): the previous frame (mesh 0, seed 0) with its first-frame state, a snapshot, the update to mesh
1, the current frame (seed 1) and its reprojection, all left on the device.  Sides:
  snapshot          : wgt_motion_snapshot of the resident mesh
  reproject         : wgt_motion_reproject_async of the current frame's G-buffer
  accumulate_motion : wgt_temporal_accumulate_motion_async over the previous state, moments and rgba8
  accumulate_plain  : wgt_temporal_accumulate_async of the same frame over the same state
The probe first checks that a second run of each side gives equal bits.  Each side runs `reps` (>= 10)
alternating repetitions of K back-to-back calls, K sized so that a side does >= 0.25 s of work in all;
the figure is the median repetition, with the minimum and maximum beside it.  The floor is each
call's compulsory traffic at 4 TB/s: the snapshot reads 64 + 16 B and writes 52 B per triangle; the
reprojection reads 29 B and writes 24 B per pixel, and 112 B more per pixel that hit a moved triangle
(its record, shading record, snapshot and slot); the accumulation 134 B per pixel and
24 B more in the motion form.  Prints one JSON line per side and appends them to `out`.
  python scripts/motion_probe.py [scene=sponza] [reps=10] [spp=4] [out=profiles/motion/probe.jsonl]"""
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
out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "motion", "probe.jsonl")
W, H = 1920, 1080

if w.device_count() < 1:
    sys.exit("motion_probe: no HIP device")
dev = torch.device("cuda", 0)


def vertices(tris):
    v0 = tris["v0"][:, :3].astype(np.float64)
    return np.stack([v0, v0 + tris["e1"][:, :3], v0 + tris["e2"][:, :3]], axis=1)


def jittered(tris, seed):
    v = vertices(tris)
    size = np.linalg.norm(v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0))
    rng = np.random.default_rng(seed)
    return (v + rng.uniform(-1.0, 1.0, v.shape) * 0.05 * size).astype(np.float32)


def timed(stream, launch, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(k):
        launch()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / k  # ms per call


with w.Context(0) as ctx:
    L, Q, S, T = w.mesh_scene(scene)
    ctx.upload_scene(L, Q, S, T)
    n, n_tris, nlq = W * H, len(T), len(L) + len(Q)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    d_verts = [torch.from_numpy(jittered(T, k)).to(dev) for k in range(2)]
    torch.cuda.synchronize()

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

    cam = w.camera_param(W / H, spp, 0)
    ctx.update_vertices_device(d_verts[0].data_ptr(), 3 * n_tris, n_tris)
    P = frame(cam, 0)
    (hist_t, hist), (out_t, out) = state(), state()
    ctx.temporal_accumulate_async(W, H, cam, P[0].data_ptr(), P[2], hist, stream=s)
    ctx.motion_snapshot(stream=s)
    stream.synchronize()
    ctx.update_vertices_device(d_verts[1].data_ptr(), 3 * n_tris, n_tris)
    host_ms, refit_ms = ctx.update_timing()
    C = frame(cam, 1)
    motion_t = {k: torch.zeros((3, n), dtype=torch.float32, device=dev) for k in ("pos_prev", "norm_prev")}
    motion = {k: b.data_ptr() for k, b in motion_t.items()}
    d_u8 = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    ctx.motion_reproject_async(n, C[2], motion["pos_prev"], motion["norm_prev"], stream=s)
    stream.synchronize()
    prim = C[1]["prim"].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    tri_px = int(((prim >= nlq) & (prim < nlq + n_tris)).sum().item())

    def accumulate(with_motion):
        def go():
            f = ctx.temporal_accumulate_motion_async if with_motion else ctx.temporal_accumulate_async
            kw = {"motion": motion} if with_motion else {}
            f(W, H, cam, C[0].data_ptr(), C[2], out, prev=hist, guides_prev=P[2], cam_prev=cam, d_u8_out=d_u8.data_ptr(),
              max_history=65536, stream=s, **kw)
        return go

    # the snapshot of the resident mesh (mesh 1) replaces the one the reprojection above read: it is timed last
    sides = [("reproject", lambda: ctx.motion_reproject_async(n, C[2], motion["pos_prev"], motion["norm_prev"], stream=s),
              list(motion_t.values()), (29 + 24) * n + 112 * tri_px),
             ("accumulate_motion", accumulate(True), list(out_t.values()) + [d_u8], (134 + 24) * n),
             ("accumulate_plain", accumulate(False), list(out_t.values()) + [d_u8], 134 * n),
             ("snapshot", lambda: ctx.motion_snapshot(stream=s), [], (64 + 16 + 52) * n_tris)]
    k, lens = {}, {}
    for key, go, outs, _ in sides[:3]:  # warm-up, equal bits of two runs, and K per side from one timed run
        timed(stream, go, 2)
        first_run = [t.clone() for t in outs]
        for t in outs:
            t.view(torch.uint8).fill_(0x5A)
        torch.cuda.synchronize()
        k[key] = max(1, math.ceil(250.0 / (reps * timed(stream, go, 3))))
        for a, b in zip(first_run, outs):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), key
        if key != "reproject":
            ln = out_t["len"]
            lens[key] = {"accumulated": int((ln > 0).sum().item()), "with_history": int((ln > 1).sum().item())}
    ms = {key: [] for key, *_ in sides}
    for _ in range(reps):  # alternating
        for key, go, _, _ in sides[:3]:
            ms[key].append(timed(stream, go, k[key]))
    key, go = sides[3][:2]
    timed(stream, go, 2)
    first_run = ctx.motion_snapshot_read()
    k[key] = max(1, math.ceil(250.0 / (reps * timed(stream, go, 3))))
    assert np.array_equal(first_run.view(np.uint32), ctx.motion_snapshot_read().view(np.uint32)), key
    for _ in range(reps):
        ms[key].append(timed(stream, go, k[key]))
    lines = []
    for key, _, _, nbytes in sides:
        med = float(np.median(ms[key]))
        floor = nbytes / 4e12 * 1e3
        lines.append(json.dumps({"scene": scene, "spp": spp, "side": key, "pixels": n, "triangles": n_tris,
                                 "triangle_pixels": tri_px, **lens.get(key, {}), "ms": round(med, 4),
                                 "ms_min": round(min(ms[key]), 4), "ms_max": round(max(ms[key]), 4), "bytes": nbytes,
                                 "floor_ms": round(floor, 4), "floor_fraction": round(floor / med, 3), "reps": reps,
                                 "calls_per_rep": k[key], "update_device_ms": round(refit_ms, 4),
                                 "build_id": w.build_id()}))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
