"""Refit probe: what moving a mesh costs, against the only other way to move one, a full upload.
For the Sponza and bunny stand-ins at the benchmark's sizes, one JSON line with the milliseconds of
wgt_upload_scene (host SAH build, collapse, packing, copy) and the median of 10
wgt_update_triangles calls to the mesh with every vertex moved by a seeded 5 % jitter, each update
split into its host part (checks, staging copy) and its device part (the refit kernels and their
two small readbacks, by hipEvents; wgt_update_timing).  The first update, which also prepares the
level lists, is reported apart.
  python scripts/refit_probe.py [scene ...]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import webgputracer_amd as w  # noqa: E402


def jittered(tris, seed):
    v0 = tris["v0"][:, :3].astype(np.float64)
    v = np.stack([v0, v0 + tris["e1"][:, :3], v0 + tris["e2"][:, :3]], axis=1)
    size = np.linalg.norm(v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0))
    rng = np.random.default_rng(seed)
    return w.make_triangles((v + rng.uniform(-1.0, 1.0, v.shape) * 0.05 * size).astype(np.float32))


def ms(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


out = {}
with w.Context(0) as ctx:
    for scene in sys.argv[1:] or ["sponza", "bunny"]:
        L, Q, S, T = w.mesh_scene(scene)
        ctx.upload_scene(L, Q, S, T)  # the device's first use is not an upload's cost
        upload_ms = [ms(lambda: ctx.upload_scene(L, Q, S, T)) for _ in range(3)]
        moved = [jittered(T, k) for k in range(2)]
        first_ms = ms(lambda: ctx.update_triangles(moved[0]))
        total, host, device = [], [], []
        for k in range(10):
            total.append(ms(lambda: ctx.update_triangles(moved[(k + 1) % 2])))
            h, d = ctx.update_timing()
            host.append(h)
            device.append(d)
        info = ctx.scene_info()
        med = statistics.median
        out[scene] = {"n_tris": len(T), "bvh_nodes": info["bvh_nodes"], "upload_ms": round(med(upload_ms), 2),
                      "first_update_ms": round(first_ms, 3), "update_ms": round(med(total), 3),
                      "update_host_ms": round(med(host), 3), "update_device_ms": round(med(device), 3),
                      "upload_over_update": round(med(upload_ms) / med(total), 1)}
print(json.dumps(out), flush=True)
