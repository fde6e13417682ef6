"""Hit-record queries (wgt_trace_hits_async, wgt_render_gbuffer_async) against the closest-hit query
(wgt_trace_rays_async: k_trace_hits with two fields), on device-resident buffers, timed with device events.  Needs a GPU.
Workload, per mesh stand-in at default size: the ambient-occlusion rays of scripts/occlusion_probe.py
(origins = the first hits of a 1920x1080 camera frame, cosine-hemisphere directions, seeded numpy).
Sides:
  baseline       wgt_trace_rays_async (k_trace_hits with prim and dist only)
  hits_prim_dist wgt_trace_hits_async with prim and dist only: the same launch through the other entry
                 point (until k_trace was retired the baseline was that kernel)
  hits_all       wgt_trace_hits_async with all six fields (41 bytes more written per ray, 24 read)
  gbuffer_1080p  wgt_render_gbuffer_async, one 1920x1080 tile, 1 spp, all fields and the rays (its own
                 rays: the camera's, so its time compares with the others only per ray)
Each side runs `reps` (>= 10) alternating repetitions of K back-to-back launches, K sized so that a
side does >= 0.5 s of work in all; the figure is the median repetition, with the minimum and maximum
beside it (the baseline's spread is the noise band).  Prints one JSON line per scene and side.
  python scripts/hits_probe.py [scenes=sponza,bunny] [reps=10]"""
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

scenes = (sys.argv[1] if len(sys.argv) > 1 else "sponza,bunny").split(",")
reps = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 10
W, H = 1920, 1080

if w.device_count() < 1:
    sys.exit("hits_probe: no HIP device")
dev = torch.device("cuda", 0)


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def camera_rays():
    """Pixel-centre rays of the reference camera (origin (278, 278, -800), looking down +z, fovy 40)."""
    o = np.array([278.0, 278.0, -800.0])
    half = math.tan(math.radians(40.0) / 2.0)
    ys, xs = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    d = np.stack([(2 * xs - 1) * half * W / H, (1 - 2 * ys) * half, np.ones_like(xs)], axis=-1).reshape(-1, 3)
    return np.broadcast_to(o, d.shape).astype(np.float32), unit(d).astype(np.float32)


def ao_rays(ctx, L, Q, S, T):
    """scripts/occlusion_probe.py's rays: origins on the first hits of the camera frame,
    cosine-hemisphere directions about the hit normal."""
    o, d = camera_rays()
    prim, dist = ctx.trace_rays(o, d)
    nlq = len(L) + len(Q)
    keep = prim < nlq + len(T)  # a hit on a quad or a triangle (their records carry a normal)
    o, d, prim, dist = o[keep], d[keep], prim[keep], dist[keep]
    normals = np.concatenate([L["norm"][:, :3], Q["norm"][:, :3], T["face_norm"][:, :3]]).astype(np.float64)
    nrm = unit(normals[prim])
    nrm *= -np.sign(np.sum(nrm * d, axis=1, keepdims=True))  # towards the camera ray's side
    p = o.astype(np.float64) + dist[:, None].astype(np.float64) * d + 1e-2 * nrm
    rng = np.random.default_rng(0)
    u1, u2 = rng.random(len(p)), rng.random(len(p))
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    a = np.where(np.abs(nrm[:, :1]) > 0.9, [[0.0, 1.0, 0.0]], [[1.0, 0.0, 0.0]])
    t1 = unit(np.cross(a, nrm))
    t2 = np.cross(nrm, t1)
    v = (r * np.cos(phi))[:, None] * t1 + (r * np.sin(phi))[:, None] * t2 + np.sqrt(1 - u1)[:, None] * nrm
    return p.astype(np.float32), v.astype(np.float32)


def timed(stream, launch, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(k):
        launch()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / k  # ms per launch


def record_buffers(n):
    return {"prim": torch.zeros(n, dtype=torch.int32, device=dev), "dist": torch.zeros(n, dtype=torch.float32, device=dev),
            "pos": torch.zeros((3, n), dtype=torch.float32, device=dev),
            "norm": torch.zeros((3, n), dtype=torch.float32, device=dev),
            "col": torch.zeros((3, n), dtype=torch.float32, device=dev),
            "flags": torch.zeros(n, dtype=torch.uint8, device=dev)}


def measure(ctx, scene, o, d):
    n = len(o)
    d_rays = torch.from_numpy(np.concatenate([o.T, d.T], axis=0).astype(np.float32)).to(dev)
    d_prim = torch.zeros(n, dtype=torch.int32, device=dev)
    d_dist = torch.zeros(n, dtype=torch.float32, device=dev)
    pd = record_buffers(n)
    full = record_buffers(n)
    npx = W * H
    gb = record_buffers(npx)
    gb_rays = torch.zeros((6, npx), dtype=torch.float32, device=dev)
    d_tile = torch.from_numpy(np.zeros(1, TILE_DTYPE).view(np.uint8).copy()).to(dev)
    cam = w.camera_param(W / H, 1, 0)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    torch.cuda.synchronize()

    def base():
        ctx.trace_rays_async(d_rays.data_ptr(), n, d_prim.data_ptr(), d_dist.data_ptr(), stream=s)

    def hits_pd():
        ctx.trace_hits_async(d_rays.data_ptr(), n, prim=pd["prim"].data_ptr(), dist=pd["dist"].data_ptr(), stream=s)

    def hits_all():
        ctx.trace_hits_async(d_rays.data_ptr(), n, stream=s, **{k: b.data_ptr() for k, b in full.items()})

    def gbuffer():
        ctx.render_gbuffer_async(cam, W, H, W, H, d_tile.data_ptr(), 1, d_rays=gb_rays.data_ptr(), stream=s,
                                 **{k: b.data_ptr() for k, b in gb.items()})

    sides = [("baseline", base, n), ("hits_prim_dist", hits_pd, n), ("hits_all", hits_all, n),
             ("gbuffer_1080p", gbuffer, npx)]
    k = {}
    for side, go, _ in sides:  # warm-up, and K per side from one timed launch
        timed(stream, go, 2)
        k[side] = max(1, math.ceil(500.0 / (reps * timed(stream, go, 3))))
    for b in (pd, full):  # every side's prim and dist are the closest-hit query's
        assert torch.equal(b["prim"], d_prim) and torch.equal(b["dist"].view(torch.int32), d_dist.view(torch.int32))
    ms = {side: [] for side, _, _ in sides}
    for _ in range(reps):  # alternating
        for side, go, _ in sides:
            ms[side].append(timed(stream, go, k[side]))
    med = {side: float(np.median(v)) for side, v in ms.items()}
    for side, _, rays in sides:
        per_ray = {x: med[x] / m for x, _, m in sides}
        print(json.dumps({"scene": scene, "side": side, "rays": rays, "ms": round(med[side], 4),
                          "ms_min": round(min(ms[side]), 4), "ms_max": round(max(ms[side]), 4),
                          "rays_per_s": round(rays / (med[side] * 1e-3)),
                          "vs_baseline_per_ray": round(per_ray["baseline"] / per_ray[side], 3), "reps": reps,
                          "launches_per_rep": k[side], "build_id": w.build_id()}), flush=True)


with w.Context(0) as ctx:
    for scene in scenes:
        L, Q, S, T = w.mesh_scene(scene)
        ctx.upload_scene(L, Q, S, T)
        measure(ctx, scene, *ao_rays(ctx, L, Q, S, T))
