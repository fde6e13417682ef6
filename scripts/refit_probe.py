"""Refit probe: what moving a mesh costs, against the only other way to move one, a full upload.
For the Sponza and bunny stand-ins at the benchmark's sizes, one JSON line with the milliseconds of
wgt_upload_scene (host SAH build, collapse, packing, copy) and the median of 10 updates of each
input form to the mesh with every vertex moved by a seeded 5 % jitter: wgt_update_triangles from a
host array, wgt_update_triangles_device and wgt_update_vertices_device (unindexed) from resident
torch tensors.  The three forms alternate in one process.  Each update is split into its host part
(everything before the first refit kernel: checks, the staging copy or the device check pass and
its readback) and its device part (the refit kernels and their two small readbacks, by hipEvents;
wgt_update_timing).  The first update, which also prepares the level lists, is reported apart.
  python scripts/refit_probe.py [scene ...]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import webgputracer_amd as w  # noqa: E402


def vertices(tris):
    v0 = tris["v0"][:, :3].astype(np.float64)
    return np.stack([v0, v0 + tris["e1"][:, :3], v0 + tris["e2"][:, :3]], axis=1)


def jittered(tris, seed):
    v = vertices(tris)
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
        dev = torch.device("cuda", 0)
        d_tris = [torch.from_numpy(m.view(np.uint8).copy()).to(dev) for m in moved]
        d_verts = [torch.from_numpy(vertices(m).astype(np.float32)).to(dev) for m in moved]
        torch.cuda.synchronize()
        n = len(T)
        forms = {"": lambda j: ctx.update_triangles(moved[j]),
                 "device_records_": lambda j: ctx.update_triangles_device(d_tris[j].data_ptr(), n),
                 "device_vertices_": lambda j: ctx.update_vertices_device(d_verts[j].data_ptr(), 3 * n, n)}
        times = {f: ([], [], []) for f in forms}
        for k in range(10):
            for f, update in forms.items():
                times[f][0].append(ms(lambda: update((k + 1) % 2)))
                h, d = ctx.update_timing()
                times[f][1].append(h)
                times[f][2].append(d)
        info = ctx.scene_info()
        med = statistics.median
        out[scene] = {"n_tris": n, "bvh_nodes": info["bvh_nodes"], "upload_ms": round(med(upload_ms), 2),
                      "first_update_ms": round(first_ms, 3),
                      "upload_over_update": round(med(upload_ms) / med(times[""][0]), 1)}
        for f, (total, host, device) in times.items():
            out[scene].update({f"update_{f}ms": round(med(total), 3), f"update_{f}host_ms": round(med(host), 3),
                               f"update_{f}device_ms": round(med(device), 3)})
print(json.dumps(out), flush=True)
