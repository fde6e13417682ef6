"""Occlusion queries (wgt_occluded_rays_async) against today's only other way to get the answer,
the closest-hit query (wgt_trace_rays_async: k_trace_hits with two fields) followed by a compare, on device-resident
buffers, timed with device events.  Needs a GPU.  Workloads, per mesh stand-in at default size:
  A  ambient occlusion: origins = the first hits of a 1920x1080 camera frame (trace_rays),
     cosine-hemisphere directions (seeded numpy), max_dist = 50
  B  the same rays, max_dist = +inf
  C  point-to-point visibility between random pairs of points in the box, max_dist = |b - a|
Each side runs `reps` (>= 10) alternating repetitions of K back-to-back launches, K sized so that a
side does >= 0.5 s of work in all; the figure is the median repetition, with the minimum and maximum
beside it (the baseline's spread is the noise band).  Prints one JSON line per workload and side
(baseline, occluded): rays/s, the ratio to the baseline's rays/s and the share of occluded rays.
  python scripts/occlusion_probe.py [scenes=sponza,bunny] [reps=10]"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import webgputracer_amd as w  # noqa: E402

scenes = (sys.argv[1] if len(sys.argv) > 1 else "sponza,bunny").split(",")
reps = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 10
W, H = 1920, 1080
NO_HIT = 0xFFFFFFFF

if w.device_count() < 1:
    sys.exit("occlusion_probe: no HIP device")
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
    """Origins on the first hits of the camera frame, cosine-hemisphere directions about the hit normal."""
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


def pair_rays(n):
    rng = np.random.default_rng(1)
    a, b = rng.uniform(5, 550, size=(n, 3)), rng.uniform(5, 550, size=(n, 3))
    d = (b - a).astype(np.float32)
    return a.astype(np.float32), d, np.linalg.norm(d.astype(np.float64), axis=1).astype(np.float32)


def to_dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(dev)


def timed(stream, launch, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(k):
        launch()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / k  # ms per launch


def measure(ctx, scene, name, o, d, lim):
    n = len(o)
    d_rays = to_dev(np.concatenate([o.T, d.T], axis=0).astype(np.float32))
    d_lim = to_dev(np.broadcast_to(np.asarray(lim, np.float32), (n,)))
    d_out = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_prim = torch.zeros(n, dtype=torch.int32, device=dev)
    d_dist = torch.zeros(n, dtype=torch.float32, device=dev)
    stream = torch.cuda.Stream(device=dev)
    s = stream.cuda_stream
    torch.cuda.synchronize()

    def occ():
        ctx.occluded_async(d_rays.data_ptr(), d_lim.data_ptr(), n, d_out.data_ptr(), stream=s)

    def base():
        ctx.trace_rays_async(d_rays.data_ptr(), n, d_prim.data_ptr(), d_dist.data_ptr(), stream=s)

    sides = [("baseline", base), ("occluded", occ)]
    # warm-up, the answers' agreement, and K per side from one timed launch
    k = {}
    answers = {}
    for side, go in sides:
        timed(stream, go, 2)
        ms = timed(stream, go, 3)
        k[side] = max(1, math.ceil(500.0 / (reps * ms)))
        if side == "baseline":
            answers[side] = ((d_prim != -1) & (d_dist < d_lim)).to(torch.uint8)
        else:
            answers[side] = d_out.clone()
    for side in answers:
        assert torch.equal(answers[side], answers["baseline"]), f"{scene} {name}: {side} differs from the baseline"
    share = float(answers["baseline"].float().mean())
    ms = {side: [] for side, _ in sides}
    for _ in range(reps):  # alternating
        for side, go in sides:
            ms[side].append(timed(stream, go, k[side]))
    med = {side: float(np.median(v)) for side, v in ms.items()}
    for side, _ in sides:
        print(json.dumps({"scene": scene, "workload": name, "side": side, "rays": n, "ms": round(med[side], 4),
                          "ms_min": round(min(ms[side]), 4), "ms_max": round(max(ms[side]), 4),
                          "rays_per_s": round(n / (med[side] * 1e-3)), "vs_baseline": round(med["baseline"] / med[side], 3),
                          "occluded_share": round(share, 4), "reps": reps, "launches_per_rep": k[side],
                          "build_id": w.build_id()}), flush=True)


with w.Context(0) as ctx:
    for scene in scenes:
        L, Q, S, T = w.mesh_scene(scene)
        ctx.upload_scene(L, Q, S, T)
        o, d = ao_rays(ctx, L, Q, S, T)
        measure(ctx, scene, "A_ao_50", o, d, 50.0)
        measure(ctx, scene, "B_ao_inf", o, d, np.inf)
        po, pd, plen = pair_rays(len(o))
        measure(ctx, scene, "C_visibility", po, pd, plen)
