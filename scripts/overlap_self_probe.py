"""Self-intersection queries (wgt_overlap_self_async) on the resident mesh, timed with device events against the
only route there was before them: wgt_overlap_triangles_async at k = 32 on the resident triangles' own corners,
fed back in leaf order, plus a host filter that drops each triangle itself and its neighbours by label.  Also
the counting kernel's visits (wgt_overlap_self_stats).  Needs a GPU.  Per mesh stand-in at default size, on the
uploaded tree, with labels welded on the host by position (for the probe only: the library never sees
positions as topology):
  workaround    overlap_triangles, count and prim at k = 32, n_tris queries in leaf order; the host filter's
                time (numpy, on the fetched lists) is reported beside it, not in it
  hit           hit alone (the traversal ends at the first member)
  count         count alone
  count k=8     count and prim at k = 8
  count k=32    count and prim at k = 32
  bare k=32     the same without an index buffer: what the workaround's kernel computes, but for the roles by id
The figure is the median of `reps` (>= 10) repetitions of K back-to-back launches, K sized so that the
repetitions do >= 0.5 s of work in all, with the minimum and maximum beside it.  Every list row is checked for
symmetry on the triangles whose lists are complete (t in s's list iff s in t's); bit equality with the host
brute force is the tests' business (tests/test_gpu_overlap_self.py), the brute force being O(n^2).
Writes one JSON document (default profiles/overlap_self/probe.json) and prints one line per measurement.
  python scripts/overlap_self_probe.py [scenes=bunny,sponza] [reps=10] [out=profiles/overlap_self/probe.json]"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import webgputracer_amd as w  # noqa: E402

scenes = (sys.argv[1] if len(sys.argv) > 1 else "bunny,sponza").split(",")
reps = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 10
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "overlap_self", "probe.json")
KMAX = 32
NO_HIT = 0xFFFFFFFF

if w.device_count() < 1:
    sys.exit("overlap_self_probe: no HIP device")
dev = torch.device("cuda", 0)


def corners(v0, e1, e2):
    v0, e1, e2 = (np.ascontiguousarray(x, np.float32) for x in (v0, e1, e2))
    return np.stack([v0, v0 + e1, v0 + e2], 1)


def weld(T):
    """(n, 3) uint32 labels: equal corner positions (bit for bit, after one rounding) get one label."""
    C = corners(T["v0"][:, :3], T["e1"][:, :3], T["e2"][:, :3]).reshape(-1, 3)
    _, inverse = np.unique(C.view(np.uint32), axis=0, return_inverse=True)
    return np.ascontiguousarray(inverse.reshape(-1, 3).astype(np.uint32)), int(inverse.max()) + 1


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


def host_filter(ids, count, prim, labels, first_prim):
    """The workaround's second half: per query (resident triangle ids[i]) drop itself and every listed triangle
    that shares a label.  -> kept (n, 32) bool."""
    valid = prim != NO_HIT
    t = np.where(valid, prim - first_prim, 0).astype(np.int64)
    mine, theirs = labels[ids][:, None, :, None], labels[t][:, :, None, :]
    return valid & (t != ids[:, None]) & ~(mine == theirs).any((2, 3))


def symmetric(count, prim, first_prim, k):
    """On the triangles with complete lists: t in s's list iff s in t's."""
    full = count <= k
    s, j = np.nonzero((prim != NO_HIT) & full[:, None])
    t = prim[s, j].astype(np.int64) - first_prim
    both = full[t]
    s, t = s[both].astype(np.int64), t[both]
    n = len(count)
    return bool(np.isin(t * n + s, s * n + t).all()), len(s) // 2


results = []
with w.Context(0) as ctx:
    for scene in scenes:
        L, Qd, S, T = w.mesh_scene(scene)
        n = len(T)
        labels, n_verts = weld(T)
        ctx.upload_scene(L, Qd, S, T)
        info = ctx.scene_info()
        first_prim = info["n_lights"] + info["n_quads"]
        recs = ctx.bvh_read()[1]  # leaf order
        ids = np.ascontiguousarray(recs[:, 0, 3]).view(np.uint32).astype(np.int64)
        Q = corners(recs[:, 0, :3], recs[:, 1, :3], recs[:, 2, :3])
        d_q = torch.from_numpy(np.ascontiguousarray(Q.reshape(n, 9).T)).to(dev)
        d_idx = torch.from_numpy(labels.view(np.int32)).to(dev)
        buf = {"hit": torch.zeros(n, dtype=torch.uint8, device=dev), "count": torch.zeros((1, n), dtype=torch.int32, device=dev),
               "prim": torch.zeros((KMAX, n), dtype=torch.int32, device=dev)}
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        common = {"scene": scene, "n_tris": n, "n_welded_vertices": n_verts, "bvh_nodes": info["bvh_nodes"],
                  "bvh_stack": info["bvh_stack"], "reps": reps, "build_id": w.build_id()}

        # the parent's only route: the overlap query on the resident corners in leaf order, then the host filter
        def workaround():
            ctx.overlap_triangles_async(d_q.data_ptr(), n, KMAX, stream=stream.cuda_stream, count=buf["count"].data_ptr(),
                                        prim=buf["prim"].data_ptr())

        wa_ms, wa_min, wa_max, launches = measure(stream, workaround)
        wa_nodes, wa_tests = ctx.overlap_triangles_stats(d_q.data_ptr(), n, KMAX, count=buf["count"].data_ptr(),
                                                         prim=buf["prim"].data_ptr())
        count = buf["count"].cpu().numpy().view(np.uint32).reshape(-1)
        prim = np.ascontiguousarray(buf["prim"].cpu().numpy().view(np.uint32).T)
        filt = []
        for _ in range(5):
            t0 = time.perf_counter()
            kept = host_filter(ids, count, prim, labels, first_prim)
            filt.append((time.perf_counter() - t0) * 1e3)
        filter_ms = float(np.median(filt))
        rows = [dict(common, form="workaround", k=KMAX, indexed=False, ms=round(wa_ms, 4), ms_min=round(wa_min, 4),
                     ms_max=round(wa_max, 4), triangles_per_s=round(n / (wa_ms * 1e-3)), launches_per_rep=launches,
                     node_visits_per_triangle=round(wa_nodes / n, 2), tri_tests_per_triangle=round(wa_tests / n, 2),
                     host_filter_ms=round(filter_ms, 3), triangles_per_s_with_filter=round(n / ((wa_ms + filter_ms) * 1e-3)),
                     mean_listed=round(float(np.minimum(count, KMAX).mean()), 3), mean_kept=round(float(kept.sum(1).mean()), 4),
                     share_truncated=round(float((count > KMAX).mean()), 5),
                     share_with_a_kept_entry=round(float(kept.any(1).mean()), 5))]
        for form, k, fields, indexed in (("hit", 0, ("hit",), True), ("count", 0, ("count",), True),
                                         ("count k=8", 8, ("count", "prim"), True), ("count k=32", KMAX, ("count", "prim"), True),
                                         ("bare k=32", KMAX, ("count", "prim"), False)):
            ptrs = {f: buf[f].data_ptr() for f in fields}
            ip = d_idx.data_ptr() if indexed else 0

            def go():
                ctx.overlap_self_async(ip, k, stream=stream.cuda_stream, **ptrs)

            med, lo, hi, launches = measure(stream, go)
            nodes, tests = ctx.overlap_self_stats(ip, k, **ptrs)
            row = dict(common, form=form, k=k, indexed=indexed, ms=round(med, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                       triangles_per_s=round(n / (med * 1e-3)), ratio_to_workaround_kernel=round(wa_ms / med, 4),
                       ratio_to_workaround_with_filter=round((wa_ms + filter_ms) / med, 4), launches_per_rep=launches,
                       node_visits_per_triangle=round(nodes / n, 2), tri_tests_per_triangle=round(tests / n, 2),
                       lds_bytes_per_wave=256 * (info["bvh_stack"] + k))
            if form == "hit":
                row["share_cutting"] = round(float(buf["hit"].float().mean()), 5)
            else:
                c = buf["count"].cpu().numpy().view(np.uint32).reshape(-1)
                row.update(share_cutting=round(float((c > 0).mean()), 5), mean_count=round(float(c.mean()), 4),
                           max_count=int(c.max()), share_truncated=round(float((c > k).mean()), 5) if k else None)
                if k:
                    p = np.ascontiguousarray(buf["prim"][:k].cpu().numpy().view(np.uint32).T)
                    ok, pairs = symmetric(c, p, first_prim, k)
                    row.update(symmetric=bool(ok), pairs_between_complete_lists=pairs)
            rows.append(row)
        for row in rows:
            print(json.dumps(row), flush=True)
        results += rows
        del buf

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump({"command": "python scripts/overlap_self_probe.py " + " ".join(sys.argv[1:3]), "rows": results}, f, indent=1)
    f.write("\n")
