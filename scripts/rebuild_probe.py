"""Rebuild probe: what making a new tree on the device costs and what the tree is worth, against the
two other ways to follow a changed mesh: a full upload (the host SAH build) and a refit of the old tree.
For the Sponza and bunny stand-ins at the benchmark's sizes and the leaf targets 4 and 8, one JSON line:
  * wgt_upload_scene's milliseconds, re-measured here, and the median of 10 wgt_rebuild_triangles_device
    calls on resident records, split into host and device part (wgt_update_timing), beside the device
    refit's (wgt_update_triangles_device);
  * node visits and triangle tests per traced ray and the 1080p / 16 spp frame time (device events,
    wgt_render_tiles_profile) on the rebuilt tree against the uploaded SAH tree of the same mesh, two
    contexts alternating in one process after a warm-up, with each tree's ps_waves and node_form;
  * for the mesh deformed by a seeded 5 % jitter and with its triangles' positions permuted among the
    indices: the frame time on the refit tree and on a rebuilt one, and the frames after which a
    rebuild has paid for itself.  The permuted mesh, whose refit tree makes every ray visit most of the
    nodes, is rendered at 160 x 90 / 4 spp, 3 rounds, leaf target 4 only: its figures are per such frame.
  python scripts/rebuild_probe.py [scene ...]"""
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
from webgputracer_amd._lib import TILE_DTYPE  # noqa: E402

W, H, SPP, ROUNDS = 1920, 1080, 16, 10
med = statistics.median


def vertices(tris):
    v0 = tris["v0"][:, :3].astype(np.float64)
    return np.stack([v0, v0 + tris["e1"][:, :3], v0 + tris["e2"][:, :3]], axis=1)


def jittered(tris, seed):
    v = vertices(tris)
    size = np.linalg.norm(v.reshape(-1, 3).max(0) - v.reshape(-1, 3).min(0))
    rng = np.random.default_rng(seed)
    out = w.make_triangles((v + rng.uniform(-1.0, 1.0, v.shape) * 0.05 * size).astype(np.float32))
    out["col"], out["emissive"] = tris["col"], tris["emissive"]
    return out


def permuted(tris, seed):
    return tris[np.random.default_rng(seed).permutation(len(tris))].copy()


def ms(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def resident(a):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


def frames(ctxs, cam, d_tile, W=W, H=H, rounds=ROUNDS):
    """Median frame milliseconds of each context, alternating, after one warm-up frame each; and each one's
    counters per traced ray."""
    for c in ctxs:
        c.render_tiles_profile(cam, W, H, W, H, d_tile.data_ptr(), 1)
    t = [[] for _ in ctxs]
    for _ in range(rounds):
        for k, c in enumerate(ctxs):
            t[k].append(c.render_tiles_profile(cam, W, H, W, H, d_tile.data_ptr(), 1)["kernel_ms"])
    out = []
    for k, c in enumerate(ctxs):
        st = c.render_tiles_stats(cam, W, H, W, H, d_tile.data_ptr(), 1)
        info = c.scene_info()
        out.append({"frame_ms": round(med(t[k]), 3), "node_visits_per_ray": round(st["node_visits"] / st["traced_rays"], 3),
                    "tri_tests_per_ray": round(st["tri_tests"] / st["traced_rays"], 3), "bvh_nodes": info["bvh_nodes"],
                    "bvh_stack": info["bvh_stack"], "ps_waves": info["ps_waves"], "node_form": info["node_form"]})
    return out


out = {}
with w.Context(0) as up, w.Context(0) as rb:
    tile = np.zeros(1, TILE_DTYPE)
    tile["seed"] = 7
    d_tile = resident(tile)
    cam = w.camera_param(W / H, SPP, 7)
    for scene in sys.argv[1:] or ["sponza", "bunny"]:
        L, Q, S, T = w.mesh_scene(scene)
        n = len(T)
        up.upload_scene(L, Q, S, T)  # the device's first use is not an upload's cost
        upload_ms = med([ms(lambda: up.upload_scene(L, Q, S, T)) for _ in range(3)])
        rb.upload_scene(L, Q, S, T)
        deformed = {"jitter5": jittered(T, 5), "permuted": permuted(T, 12)}
        d_T = resident(T)
        d_def = {k: resident(v) for k, v in deformed.items()}
        res = {"n_tris": n, "upload_ms": round(upload_ms, 2)}
        for leaf in (4, 8):
            os.environ["WGT_REBUILD_LEAF"] = str(leaf)
            rb.rebuild_triangles_device(d_T.data_ptr(), n)  # the first one allocates
            total, host, device = [], [], []
            for _ in range(ROUNDS):
                total.append(ms(lambda: rb.rebuild_triangles_device(d_T.data_ptr(), n)))
                h, d = rb.update_timing()
                host.append(h)
                device.append(d)
            sah, lbvh = frames((up, rb), cam, d_tile)
            refit = []
            for _ in range(ROUNDS):
                rb.update_triangles_device(d_T.data_ptr(), n)
                refit.append(rb.update_timing()[1])
            r = {"rebuild_ms": round(med(total), 3), "rebuild_host_ms": round(med(host), 3),
                 "rebuild_device_ms": round(med(device), 3), "refit_device_ms": round(med(refit), 3),
                 "upload_over_rebuild": round(upload_ms / med(total), 1), "uploaded": sah, "rebuilt": lbvh,
                 "frame_rebuilt_over_uploaded": round(lbvh["frame_ms"] / sah["frame_ms"], 3)}
            for name, d_m in d_def.items():
                if name == "permuted" and leaf != 4:
                    continue
                small = name == "permuted"
                up.upload_scene(L, Q, S, T)
                up.update_triangles_device(d_m.data_ptr(), n)  # the upload's tree, refit to the deformed mesh
                rb.rebuild_triangles_device(d_m.data_ptr(), n)
                a, b = (frames((up, rb), w.camera_param(160 / 90, 4, 7), d_tile, 160, 90, 3) if small else
                        frames((up, rb), cam, d_tile))
                gain = a["frame_ms"] - b["frame_ms"]
                r[name] = {"refit": a, "rebuilt": b,
                           "break_even_frames": round(med(total) / gain, 2) if gain > 0 else None}
            res[f"leaf{leaf}"] = r
            up.upload_scene(L, Q, S, T)
        out[scene] = res
os.environ.pop("WGT_REBUILD_LEAF", None)
print(json.dumps(out), flush=True)
