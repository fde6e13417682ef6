"""k-nearest and within-radius closest-point queries (wgt_nearest_k_points_async) on device-resident points,
timed with device events against wgt_nearest_points_async on the same points in the same process, and the
counting kernels' visits (wgt_nearest_k_points_stats).  Needs a GPU.  Per mesh stand-in at default size, on
the uploaded tree (the SAH build) and on the rebuilt one (wgt_rebuild_triangles, the Morton build), the two
point sets of scripts/nearest_probe.py (2^20 points each: "surface" within 1 % of the mesh's size of the
surface, "box" uniform in the Cornell box), these forms:
  nearest          wgt_nearest_points, all four fields: the rate every other row is a ratio to
  cull k=1, 8, 32  no count, no radius, all four list fields
  count            the count alone at a radius of 1 % of the mesh's size
  count k=8        the count and all four list fields at k = 8, at that radius
The two count rows are measured with the node step in slot order (WGT_NEAREST_K_SORT=0, the default of the
count alone) and nearest first (WGT_NEAREST_K_SORT=1, the default with a list).  The figure is the median of `reps` (>= 10) repetitions of K back-to-back launches, K
sized so that the repetitions do >= 0.5 s of work in all, with the minimum and maximum beside it.  The first
2,048 answers of every row are compared with the host brute force (wgt_nearest_k_points_spec) bit for bit.
Writes one JSON document (default profiles/nearest_k/probe.json) and prints one line per measurement.
  python scripts/nearest_k_probe.py [scenes=bunny,sponza] [reps=10] [out=profiles/nearest_k/probe.json]"""
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "nearest_k", "probe.json")
N, N_HOST, THREADS, K_MAX = 1 << 20, 2048, 16, 32
LISTS = ("prim", "dist", "pos", "uv")
PLANES = {"count": 1, "prim": 1, "dist": 1, "pos": 3, "uv": 2}

if w.device_count() < 1:
    sys.exit("nearest_k_probe: no HIP device")
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


def measure(stream, go):
    timed(stream, go, 2)
    k = max(1, math.ceil(500.0 / (reps * timed(stream, go, 3))))
    ms = [timed(stream, go, k) for _ in range(reps)]
    return float(np.median(ms)), min(ms), max(ms), k


def host_spec(T, P, k, max_dist, first_prim):
    """The brute force on THREADS threads (ctypes releases the GIL)."""
    parts = np.array_split(np.arange(len(P)), THREADS)
    with ThreadPoolExecutor(THREADS) as ex:
        res = list(ex.map(lambda ix: w.nearest_k_points_spec(T, P[ix], k, max_dist=max_dist, first_prim=first_prim), parts))
    return {f: np.concatenate([r[f] for r in res]) for f in res[0]}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def head(buf, f, k):
    """The first N_HOST answers of device field f (k planes per component) as the Python face shapes them."""
    a = buf[f][:(1 if f == "count" else k) * PLANES[f], :N_HOST].cpu().numpy()
    a = a.view(np.uint32) if f in ("count", "prim") else a
    if f == "count":
        return a.reshape(-1)
    return a.T if f in ("prim", "dist") else a.reshape(k, PLANES[f], -1).transpose(2, 0, 1)


results = []
with w.Context(0) as ctx:
    for scene in scenes:
        L, Q, S, T = w.mesh_scene(scene)
        size, sets = point_sets(T)
        radius = np.float32(0.01 * size)
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
                d_lim = torch.full((N,), float(radius), dtype=torch.float32, device=dev)
                buf = {f: torch.zeros(((1 if f == "count" else K_MAX) * p, N), dtype=torch.int32 if f in ("count", "prim") else torch.float32,
                                      device=dev) for f, p in PLANES.items()}
                stream = torch.cuda.Stream(device=dev)
                torch.cuda.synchronize()
                if name not in host:  # the resident values are the caller's for either tree: once per set
                    host[name] = (host_spec(T, P[:N_HOST], K_MAX, None, first_prim), host_spec(T, P[:N_HOST], 8, radius, first_prim))
                free, near = host[name]
                one = {f: buf[f].data_ptr() for f in LISTS}

                def base():
                    ctx.nearest_points_async(d_pts.data_ptr(), N, stream=stream.cuda_stream, **one)

                base_ms, base_min, base_max, launches = measure(stream, base)
                nodes, tests = ctx.nearest_points_stats(d_pts.data_ptr(), N, **one)
                common = {"scene": scene, "n_tris": int(len(T)), "mesh_size": round(size, 2), "tree": tree,
                          "bvh_nodes": info["bvh_nodes"], "bvh_stack": info["bvh_stack"], "points": name, "n": N, "reps": reps}
                rows = [dict(common, form="nearest", k=1, radius=None, ms=round(base_ms, 4), ms_min=round(base_min, 4),
                             ms_max=round(base_max, 4), queries_per_s=round(N / (base_ms * 1e-3)), ratio_to_nearest=1.0,
                             node_visits_per_query=round(nodes / N, 2), tri_tests_per_query=round(tests / N, 2),
                             launches_per_rep=launches)]
                forms = [("cull", k, None, LISTS, "0") for k in (1, 8, 32)]
                for sort in ("0", "1"):
                    forms += [("count", 0, radius, ("count",), sort), ("count", 8, radius, ("count",) + LISTS, sort)]
                for form, k, rad, fields, sort in forms:
                    os.environ["WGT_NEAREST_K_SORT"] = sort
                    ptrs = {f: buf[f].data_ptr() for f in fields}
                    lim = d_lim.data_ptr() if rad is not None else 0

                    def go():
                        ctx.nearest_k_points_async(d_pts.data_ptr(), N, k, d_max_dist=lim, stream=stream.cuda_stream, **ptrs)

                    med, lo, hi, launches = measure(stream, go)
                    nodes, tests = ctx.nearest_k_points_stats(d_pts.data_ptr(), N, k, d_max_dist=lim, **ptrs)
                    want = free if rad is None else near
                    agree = all(np.array_equal(bits(head(buf, f, k)), bits(want[f] if f == "count" else want[f][:, :k])) for f in fields)
                    rows.append(dict(common, form=form, k=k, radius=None if rad is None else round(float(rad), 4),
                                     node_step=("nearest first" if form == "cull" or sort == "1" else "slot order"),
                                     ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                                     queries_per_s=round(N / (med * 1e-3)), ratio_to_nearest=round(base_ms / med, 4),
                                     node_visits_per_query=round(nodes / N, 2), tri_tests_per_query=round(tests / N, 2),
                                     launches_per_rep=launches, lds_bytes_per_wave=256 * (info["bvh_stack"] + (3 if k else 2) * k),
                                     mean_count=(round(float(near["count"].mean()), 2) if rad is not None else None),
                                     equal_to_host_bits=bool(agree), build_id=w.build_id()))
                os.environ.pop("WGT_NEAREST_K_SORT", None)
                for row in rows:
                    print(json.dumps(row), flush=True)
                results += rows
                del buf

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump({"command": "python scripts/nearest_k_probe.py " + " ".join(sys.argv[1:3]), "rows": results}, f, indent=1)
    f.write("\n")
