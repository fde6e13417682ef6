"""Triangle overlap queries (wgt_overlap_triangles_async) on device-resident query triangles, timed with device
events against what a caller could do before them: three wgt_occluded_rays_async edge rays per query, on the
same queries in the same process (that covers half the definition: it misses every resident edge that goes
through a query's face, and it cannot name the triangles).  Also the counting kernel's visits
(wgt_overlap_triangles_stats).  Needs a GPU.  Per mesh stand-in at default size, on the uploaded tree (the SAH
build) and on the rebuilt one (wgt_rebuild_triangles, the Morton build), two query sets of 2^20 triangles each:
  copy   the mesh's own triangles moved by 1 % of its size, so nearly every query overlaps a few
  box    random triangles of the mesh's median edge length, uniform in the Cornell box
and these forms:
  edge rays     3 x 2^20 occlusion rays along the queries' edges, each limited to its edge: the rate every
                other row is a ratio to
  hit           hit alone (the traversal ends at the first overlapping triangle)
  count         count alone
  count k=8     count and prim at k = 8
The figure is the median of `reps` (>= 10) repetitions of K back-to-back launches, K sized so that the
repetitions do >= 0.5 s of work in all, with the minimum and maximum beside it.  The first 2,048 answers of
every overlap row are compared with the host brute force (wgt_overlap_triangles_spec) bit for bit.
Writes one JSON document (default profiles/overlap/probe.json) and prints one line per measurement.
  python scripts/overlap_probe.py [scenes=bunny,sponza] [reps=10] [out=profiles/overlap/probe.json]"""
import json
import math
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import webgputracer_amd as w  # noqa: E402

scenes = (sys.argv[1] if len(sys.argv) > 1 else "bunny,sponza").split(",")
reps = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 10
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "overlap", "probe.json")
N, N_HOST, THREADS, K = 1 << 20, 2048, 16, 8
FIELDS = ("hit", "count", "prim")

if w.device_count() < 1:
    sys.exit("overlap_probe: no HIP device")
dev = torch.device("cuda", 0)


def query_sets(T):
    rng = np.random.default_rng(0)
    v0, e1, e2 = (T[k][:, :3].astype(np.float64) for k in ("v0", "e1", "e2"))
    verts = np.concatenate([v0, v0 + e1, v0 + e2])
    size = float(np.linalg.norm(verts.max(0) - verts.min(0)))
    ok = np.flatnonzero(np.linalg.norm(np.cross(e1, e2), axis=1) > 0.0)
    idx = ok[rng.integers(0, len(ok), N)]
    shift = 0.01 * size * np.array([0.5377, 0.3183, 0.7807]) / np.linalg.norm([0.5377, 0.3183, 0.7807])
    copy = np.stack([v0[idx], v0[idx] + e1[idx], v0[idx] + e2[idx]], 1) + shift
    edge = float(np.median(np.concatenate([np.linalg.norm(e, axis=1) for e in (e1[ok], e2[ok], (e2 - e1)[ok])])))
    u = rng.normal(size=(N, 2, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    a0 = rng.uniform(5.0, 550.0, (N, 1, 3))
    box = np.concatenate([a0, a0 + edge * u], 1)
    return size, edge, {"copy": copy.astype(np.float32), "box": box.astype(np.float32)}


def edge_rays(Q):
    """The three edges of each query as rays: six planes of 3 n floats (origins, unit directions) and the limits."""
    o = np.concatenate([Q[:, 0], Q[:, 1], Q[:, 2]]).astype(np.float64)
    d = np.concatenate([Q[:, 1] - Q[:, 0], Q[:, 2] - Q[:, 1], Q[:, 0] - Q[:, 2]]).astype(np.float64)
    length = np.linalg.norm(d, axis=1)
    rays = np.concatenate([o, d / length[:, None]], 1).astype(np.float32)
    return np.ascontiguousarray(rays.T), length.astype(np.float32)


def timed(stream, launch, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(k):
        launch()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1) / k  # ms per launch


def measure(stream, go):
    timed(stream, go, 2)
    k = max(1, math.ceil(500.0 / (reps * timed(stream, go, 3))))
    ms = [timed(stream, go, k) for _ in range(reps)]
    return float(np.median(ms)), min(ms), max(ms), k


def host_spec(T, Q, first_prim):
    """The brute force on THREADS threads (ctypes releases the GIL)."""
    parts = np.array_split(np.arange(len(Q)), THREADS)
    with ThreadPoolExecutor(THREADS) as ex:
        res = list(ex.map(lambda ix: w.overlap_triangles_spec(T, Q[ix], K, first_prim=first_prim), parts))
    return {f: np.concatenate([r[f] for r in res]) for f in res[0]}


def head(buf, f, k):
    """The first N_HOST answers of device field f as the Python face shapes them."""
    if f == "hit":
        return buf[f][:N_HOST].cpu().numpy() != 0
    a = buf[f][:(k if f == "prim" else 1), :N_HOST].cpu().numpy().view(np.uint32)
    return a.T if f == "prim" else a.reshape(-1)


results = []
with w.Context(0) as ctx:
    for scene in scenes:
        L, Qd, S, T = w.mesh_scene(scene)
        size, edge, sets = query_sets(T)
        host = {}
        for tree in ("uploaded", "rebuilt"):
            if tree == "uploaded":
                ctx.upload_scene(L, Qd, S, T)
            else:
                ctx.rebuild_triangles(T)
            info = ctx.scene_info()
            first_prim = info["n_lights"] + info["n_quads"]
            for name, Q in sets.items():
                d_q = torch.from_numpy(np.ascontiguousarray(Q.reshape(N, 9).T)).to(dev)
                rays, limits = edge_rays(Q)
                d_rays, d_lim = torch.from_numpy(rays).to(dev), torch.from_numpy(limits).to(dev)
                d_occ = torch.zeros(3 * N, dtype=torch.uint8, device=dev)
                buf = {"hit": torch.zeros(N, dtype=torch.uint8, device=dev), "count": torch.zeros((1, N), dtype=torch.int32, device=dev),
                       "prim": torch.zeros((K, N), dtype=torch.int32, device=dev)}
                stream = torch.cuda.Stream(device=dev)
                torch.cuda.synchronize()
                if name not in host:  # the resident values are the caller's for either tree: once per set
                    host[name] = host_spec(T, Q[:N_HOST], first_prim)
                want = host[name]

                def base():
                    ctx.occluded_async(d_rays.data_ptr(), d_lim.data_ptr(), 3 * N, d_occ.data_ptr(), stream=stream.cuda_stream)

                base_ms, base_min, base_max, launches = measure(stream, base)
                torch.cuda.synchronize()
                occ = d_occ.cpu().numpy().reshape(3, N).any(0)
                common = {"scene": scene, "n_tris": int(len(T)), "mesh_size": round(size, 2), "median_edge": round(edge, 3),
                          "tree": tree, "bvh_nodes": info["bvh_nodes"], "bvh_stack": info["bvh_stack"], "queries": name, "n": N,
                          "reps": reps}
                rows = [dict(common, form="edge rays", k=0, ms=round(base_ms, 4), ms_min=round(base_min, 4), ms_max=round(base_max, 4),
                             queries_per_s=round(N / (base_ms * 1e-3)), ratio_to_edge_rays=1.0, launches_per_rep=launches,
                             share_with_an_occluded_edge=round(float(occ.mean()), 4))]
                for form, k, fields in (("hit", 0, ("hit",)), ("count", 0, ("count",)), ("count k=8", K, ("count", "prim"))):
                    ptrs = {f: buf[f].data_ptr() for f in fields}

                    def go():
                        ctx.overlap_triangles_async(d_q.data_ptr(), N, k, stream=stream.cuda_stream, **ptrs)

                    med, lo, hi, launches = measure(stream, go)
                    nodes, tests = ctx.overlap_triangles_stats(d_q.data_ptr(), N, k, **ptrs)
                    agree = all(np.array_equal(head(buf, f, k), want[f][:, :k] if f == "prim" else want[f]) for f in fields)
                    hits = float(buf["hit"].float().mean()) if form == "hit" else float((buf["count"] != 0).float().mean())
                    rows.append(dict(common, form=form, k=k, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                                     queries_per_s=round(N / (med * 1e-3)), ratio_to_edge_rays=round(base_ms / med, 4),
                                     node_visits_per_query=round(nodes / N, 2), tri_tests_per_query=round(tests / N, 2),
                                     launches_per_rep=launches, lds_bytes_per_wave=256 * (info["bvh_stack"] + k),
                                     share_overlapping=round(hits, 4),
                                     mean_count=(round(float(buf["count"].float().mean()), 3) if form != "hit" else None),
                                     equal_to_host_bits=bool(agree), build_id=w.build_id()))
                for row in rows:
                    print(json.dumps(row), flush=True)
                results += rows
                del buf

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump({"command": "python scripts/overlap_probe.py " + " ".join(sys.argv[1:3]), "rows": results}, f, indent=1)
    f.write("\n")
