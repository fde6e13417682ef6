"""Multi-hit queries (wgt_trace_multi_hits_async) against the closest-hit query (wgt_trace_rays_async) on the
same device-resident rays in the same run, timed with device events.  Needs a GPU.  Per mesh stand-in at
default size the rays are occlusion_probe's workload A: origins on the first hits of a 1920x1080 camera
frame, cosine-hemisphere directions (seeded numpy).  Sides:
  baseline             wgt_trace_rays_async
  cull_k{1,4,8,32}     prim and dist only, no limit: the bound shrinks to the k-th distance
  count_50, count_inf  count only, max_dist = 50 and +inf: every hit below the limit is visited
Each side runs `reps` (>= 10) alternating repetitions of K back-to-back launches, K sized so that a side does
>= 0.5 s of work in all; the figure is the median repetition, with the minimum and maximum beside it (the
baseline's spread is the noise band).  Before timing, each cull side's first entry is compared with the
baseline's distance bit for bit, and the counting kernel reports its visits.
Writes one JSON document (default profiles/multihit/probe.json) and prints one line per side.
  python scripts/multihit_probe.py [scenes=bunny,sponza] [reps=10] [out=profiles/multihit/probe.json]"""
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import webgputracer_amd as w  # noqa: E402

scenes = (sys.argv[1] if len(sys.argv) > 1 else "bunny,sponza").split(",")
reps = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 10
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "multihit", "probe.json")
W, H = 1920, 1080

if w.device_count() < 1:
    sys.exit("multihit_probe: no HIP device")
dev = torch.device("cuda", 0)


def unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def first_hit_rays(ctx, L, Q, S, T):
    """scripts/occlusion_probe.py's ao_rays: origins on the first hits of the reference camera's frame
    (pixel centres), cosine-hemisphere directions about the hit normal."""
    half = math.tan(math.radians(40.0) / 2.0)
    ys, xs = np.meshgrid((np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W, indexing="ij")
    d = unit(np.stack([(2 * xs - 1) * half * W / H, (1 - 2 * ys) * half, np.ones_like(xs)], axis=-1).reshape(-1, 3))
    o = np.broadcast_to(np.array([278.0, 278.0, -800.0]), d.shape).astype(np.float32)
    d = d.astype(np.float32)
    prim, dist = ctx.trace_rays(o, d)
    keep = prim < len(L) + len(Q) + len(T)  # a hit on a quad or a triangle (their records carry a normal)
    o, d, prim, dist = o[keep], d[keep], prim[keep], dist[keep]
    normals = np.concatenate([L["norm"][:, :3], Q["norm"][:, :3], T["face_norm"][:, :3]]).astype(np.float64)
    nrm = unit(normals[prim])
    nrm *= -np.sign(np.sum(nrm * d, axis=1, keepdims=True))
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


rows = []
with w.Context(0) as ctx:
    for scene in scenes:
        L, Q, S, T = w.mesh_scene(scene)
        ctx.upload_scene(L, Q, S, T)
        o, d = first_hit_rays(ctx, L, Q, S, T)
        n = len(o)
        d_rays = torch.from_numpy(np.ascontiguousarray(np.concatenate([o.T, d.T], axis=0), np.float32)).to(dev)
        d_lim50 = torch.full((n,), 50.0, dtype=torch.float32, device=dev)
        d_count = torch.zeros(n, dtype=torch.int32, device=dev)
        d_prim = torch.zeros((32, n), dtype=torch.int32, device=dev)
        d_dist = torch.zeros((32, n), dtype=torch.float32, device=dev)
        d_bprim = torch.zeros(n, dtype=torch.int32, device=dev)
        d_bdist = torch.zeros(n, dtype=torch.float32, device=dev)
        stream = torch.cuda.Stream(device=dev)
        s = stream.cuda_stream
        torch.cuda.synchronize()

        def base():
            ctx.trace_rays_async(d_rays.data_ptr(), n, d_bprim.data_ptr(), d_bdist.data_ptr(), stream=s)

        def cull(k):
            def go():
                ctx.trace_multi_hits_async(d_rays.data_ptr(), n, k, prim=d_prim.data_ptr(), dist=d_dist.data_ptr(), stream=s)
            return go

        def count(lim):
            def go():
                ctx.trace_multi_hits_async(d_rays.data_ptr(), n, 0, d_max_dist=lim, count=d_count.data_ptr(), stream=s)
            return go

        sides = [("baseline", base, None)] + [(f"cull_k{k}", cull(k), dict(k=k)) for k in (1, 4, 8, 32)]
        sides += [("count_50", count(d_lim50.data_ptr()), dict(lim=d_lim50.data_ptr())), ("count_inf", count(0), dict(lim=0))]
        # warm-up, the answers' agreement with the baseline, the visits, and K per side from one timed launch
        kk, visits, extra = {}, {}, {}
        timed(stream, base, 2)
        hit = (d_bprim != -1) & ~torch.isnan(d_bdist)
        for side, go, what in sides:
            timed(stream, go, 2)
            kk[side] = max(1, math.ceil(500.0 / (reps * timed(stream, go, 3))))
            if side.startswith("cull"):
                assert torch.equal(d_dist[0][hit].view(torch.int32), d_bdist[hit].view(torch.int32)), f"{scene} {side}: first entry"
                visits[side] = ctx.trace_multi_hits_stats(d_rays.data_ptr(), n, what["k"], prim=d_prim.data_ptr(),
                                                          dist=d_dist.data_ptr())
            elif side.startswith("count"):
                assert torch.equal(d_count > 0, (d_bprim != -1) & (d_bdist < (50.0 if what["lim"] else math.inf))), f"{scene} {side}"
                extra[side] = {"mean_count": round(float(d_count.float().mean()), 3), "max_count": int(d_count.max())}
                visits[side] = ctx.trace_multi_hits_stats(d_rays.data_ptr(), n, 0, d_max_dist=what["lim"], count=d_count.data_ptr())
        ms = {side: [] for side, _, _ in sides}
        for _ in range(reps):  # alternating
            for side, go, _ in sides:
                ms[side].append(timed(stream, go, kk[side]))
        med = {side: float(np.median(v)) for side, v in ms.items()}
        info = ctx.scene_info()
        for side, _, _ in sides:
            row = {"scene": scene, "n_tris": int(len(T)), "bvh_stack": info["bvh_stack"], "side": side, "rays": n,
                   "ms": round(med[side], 4), "ms_min": round(min(ms[side]), 4), "ms_max": round(max(ms[side]), 4),
                   "rays_per_s": round(n / (med[side] * 1e-3)), "vs_baseline": round(med["baseline"] / med[side], 3),
                   "reps": reps, "launches_per_rep": kk[side], "build_id": w.build_id(), **extra.get(side, {})}
            if side in visits:
                row["node_visits_per_ray"] = round(visits[side][0] / n, 2)
                row["tri_tests_per_ray"] = round(visits[side][1] / n, 2)
            print(json.dumps(row), flush=True)
            rows.append(row)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump({"command": "python scripts/multihit_probe.py " + " ".join(sys.argv[1:3]), "rows": rows}, f, indent=1)
    f.write("\n")
