"""Closest-point queries (wgt_nearest_points_async) on device-resident points, timed with device events, and
the counting kernel's visits (wgt_nearest_points_stats), in one process.  Needs a GPU.  Per mesh stand-in
at default size, on the uploaded tree (the SAH build) and on the rebuilt one (wgt_rebuild_triangles, the
Morton build), two point sets of 2^20 points:
  surface  within 1 % of the mesh's size (its bounding box's diagonal) of the surface: random centroids
           moved along their face normal
  box      uniform in the Cornell box, [5, 550]^3
The figure is the median of `reps` (>= 10) repetitions of K back-to-back launches, K sized so that the
repetitions do >= 0.5 s of work in all, with the minimum and maximum beside it.  The first 2,048 points of
each set are also answered by the host brute force (wgt_nearest_points_spec) on 16 threads: its rate is
what the device's is held against, and its answers are compared with the device's bit for bit.
Writes one JSON document (default profiles/nearest/probe.json) and prints one line per measurement.
  python scripts/nearest_probe.py [scenes=bunny,sponza] [reps=10] [out=profiles/nearest/probe.json]"""
import json
import math
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import webgputracer_amd as w  # noqa: E402

scenes = (sys.argv[1] if len(sys.argv) > 1 else "bunny,sponza").split(",")
reps = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 10
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "nearest", "probe.json")
N, N_HOST, THREADS = 1 << 20, 2048, 16

if w.device_count() < 1:
    sys.exit("nearest_probe: no HIP device")
dev = torch.device("cuda", 0)


def point_sets(T):
    rng = np.random.default_rng(0)
    v0, e1, e2 = (T[k][:, :3].astype(np.float64) for k in ("v0", "e1", "e2"))
    verts = np.concatenate([v0, v0 + e1, v0 + e2])
    size = float(np.linalg.norm(verts.max(0) - verts.min(0)))
    nrm = np.cross(e1, e2)
    area = np.linalg.norm(nrm, axis=1)
    ok = np.flatnonzero(area > 0.0)
    idx = ok[rng.integers(0, len(ok), N)]
    c = v0[idx] + (e1[idx] + e2[idx]) / 3.0
    surface = c + rng.uniform(-0.01 * size, 0.01 * size, (N, 1)) * (nrm[idx] / area[idx, None])
    box = rng.uniform(5.0, 550.0, (N, 3))
    return size, {"surface": surface.astype(np.float32), "box": box.astype(np.float32)}


def timed(stream, launch, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(k):
        launch()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / k  # ms per launch


def host_rate(T, P, first_prim):
    """(queries per second, answers) of the brute force on THREADS threads (ctypes releases the GIL)."""
    parts = np.array_split(np.arange(len(P)), THREADS)
    t0 = time.perf_counter()
    with ThreadPoolExecutor(THREADS) as ex:
        res = list(ex.map(lambda ix: w.nearest_points_spec(T, P[ix], first_prim=first_prim), parts))
    dt = time.perf_counter() - t0
    return len(P) / dt, {k: np.concatenate([r[k] for r in res]) for k in res[0]}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


results = []
with w.Context(0) as ctx:
    for scene in scenes:
        L, Q, S, T = w.mesh_scene(scene)
        size, sets = point_sets(T)
        host = {}
        for tree in ("uploaded", "rebuilt"):
            if tree == "uploaded":
                ctx.upload_scene(L, Q, S, T)
            else:
                ctx.rebuild_triangles(T)
            info = ctx.scene_info()
            first_prim = info["n_lights"] + info["n_quads"]
            for name, P in sets.items():
                d_pts = torch.from_numpy(np.ascontiguousarray(P.T)).to(dev)
                d_prim = torch.zeros(N, dtype=torch.int32, device=dev)
                d_dist = torch.zeros(N, dtype=torch.float32, device=dev)
                d_pos = torch.zeros((3, N), dtype=torch.float32, device=dev)
                d_uv = torch.zeros((2, N), dtype=torch.float32, device=dev)
                stream = torch.cuda.Stream(device=dev)
                torch.cuda.synchronize()
                ptrs = dict(prim=d_prim.data_ptr(), dist=d_dist.data_ptr(), pos=d_pos.data_ptr(), uv=d_uv.data_ptr())

                def go():
                    ctx.nearest_points_async(d_pts.data_ptr(), N, stream=stream.cuda_stream, **ptrs)

                timed(stream, go, 2)
                k = max(1, math.ceil(500.0 / (reps * timed(stream, go, 3))))
                ms = [timed(stream, go, k) for _ in range(reps)]
                med = float(np.median(ms))
                nodes, tests = ctx.nearest_points_stats(d_pts.data_ptr(), N, **ptrs)
                if name not in host:  # the resident values are the caller's for either tree: once per set
                    host[name] = host_rate(T, P[:N_HOST], first_prim)
                rate, want = host[name]
                got = {"prim": d_prim[:N_HOST].cpu().numpy().view(np.uint32), "dist": d_dist[:N_HOST].cpu().numpy(),
                       "pos": d_pos[:, :N_HOST].cpu().numpy().T, "uv": d_uv[:, :N_HOST].cpu().numpy().T}
                agree = all(np.array_equal(bits(got[f]), bits(want[f])) for f in got)
                row = {"scene": scene, "n_tris": int(len(T)), "mesh_size": round(size, 2), "tree": tree,
                       "bvh_nodes": info["bvh_nodes"], "bvh_stack": info["bvh_stack"], "points": name, "n": N,
                       "ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                       "queries_per_s": round(N / (med * 1e-3)), "node_visits_per_query": round(nodes / N, 2),
                       "tri_tests_per_query": round(tests / N, 2), "reps": reps, "launches_per_rep": k,
                       "host_threads": THREADS, "host_points": N_HOST, "host_queries_per_s": round(rate, 1),
                       "equal_to_host_bits": bool(agree), "build_id": w.build_id()}
                print(json.dumps(row), flush=True)
                results.append(row)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump({"command": "python scripts/nearest_probe.py " + " ".join(sys.argv[1:3]), "rows": results}, f, indent=1)
    f.write("\n")
