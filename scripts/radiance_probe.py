"""Radiance queries (wgt_trace_radiance_async) on device-resident rays, timed with device events, against the
renderer on the same view, in one process.  Needs a GPU.  Per mesh stand-in at default size: the 1080p
G-buffer's rays (wgt_render_gbuffer: sample 0's camera ray of every pixel), 16 samples each from the pixels'
seeds, through the flat kernel (WGT_KERNEL=1) and the persistent phase-split one (the default), and the
yardstick: wgt_render_tile of the same view at 16 spp, the same number of paths along nearly the same rays
(the render jitters each sample's ray within the pixel and orders its pixel queue by cost).
Rates are traced rays per second: the stats forms' traced-ray counts (wgt_trace_radiance_stats, wgt_stats of
the render's counting pass) over the median time of `reps` (>= 10) rounds; a round times one launch of each
of the three, alternating, after two warm-up rounds.  The two forms' outputs are compared bit for bit.
Writes one JSON document (default profiles/radiance/probe.json) and prints one line per measurement.
  python scripts/radiance_probe.py [scenes=bunny,sponza] [reps=10] [out=profiles/radiance/probe.json]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import webgputracer_amd as w  # noqa: E402

scenes = (sys.argv[1] if len(sys.argv) > 1 else "bunny,sponza").split(",")
reps = max(10, int(sys.argv[2])) if len(sys.argv) > 2 else 10
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "radiance", "probe.json")
W, H, SAMPLES, SEED = 1920, 1080, 16, 1
FORMS = {"flat": "1", "phase_split": None}  # WGT_KERNEL, read per launch

if w.device_count() < 1:
    sys.exit("radiance_probe: no HIP device")
dev = torch.device("cuda", 0)


def set_form(form):
    os.environ.pop("WGT_KERNEL", None)
    if FORMS[form]:
        os.environ["WGT_KERNEL"] = FORMS[form]


def timed(stream, launch):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    launch()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


results = []
with w.Context(0) as ctx:
    for scene in scenes:
        L, Q, S, T = w.mesh_scene(scene)
        ctx.upload_scene(L, Q, S, T)
        info = ctx.scene_info()
        cam = w.camera_param(W / H, SAMPLES, SEED)
        g = ctx.render_gbuffer(cam, W, H, want=("prim",), rays=True)
        n = W * H
        soa = np.concatenate([g["origin"].reshape(-1, 3).T, g["direction"].reshape(-1, 3).T])
        d_rays = torch.from_numpy(np.ascontiguousarray(soa)).to(dev)
        d_out = {f: {"rgb": torch.zeros((3, n), dtype=torch.float32, device=dev),
                     "prim": torch.zeros(n, dtype=torch.int32, device=dev),
                     "seed": torch.zeros(n, dtype=torch.int32, device=dev)} for f in FORMS}
        stream = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()

        def query(form):
            set_form(form)
            ctx.trace_radiance_async(d_rays.data_ptr(), n, seed0=SEED * n, samples=SAMPLES, stream=stream.cuda_stream,
                                     **{k: t.data_ptr() for k, t in d_out[form].items()})

        ms = {f: [] for f in list(FORMS) + ["render"]}
        for r in range(reps + 2):
            for f in FORMS:
                t = timed(stream, lambda: query(f))
                if r >= 2:
                    ms[f].append(t)
            set_form("phase_split")
            st = ctx.render_tile(cam, W, H, want=("f32",), stats=True)["stats"]
            if r >= 2:
                ms["render"].append(st["kernel_ms"])
        set_form("phase_split")
        counts = ctx.trace_radiance_stats(d_rays.data_ptr(), n, seed0=SEED * n, samples=SAMPLES,
                                          rgb=d_out["phase_split"]["rgb"].data_ptr())
        set_form("flat")
        counts_flat = ctx.trace_radiance_stats(d_rays.data_ptr(), n, seed0=SEED * n, samples=SAMPLES,
                                               rgb=d_out["flat"]["rgb"].data_ptr())
        set_form("phase_split")
        torch.cuda.synchronize()
        same = counts == counts_flat and all(torch.equal(d_out["flat"][k].view(torch.int32), d_out["phase_split"][k].view(torch.int32))
                                             for k in d_out["flat"])
        render_rate = st["traced_rays"] / (float(np.median(ms["render"])) * 1e-3)
        base = {"scene": scene, "n_tris": int(len(T)), "bvh_nodes": info["bvh_nodes"], "ps_waves": info["ps_waves"],
                "rays": n, "samples": SAMPLES, "reps": reps, "build_id": w.build_id()}
        rows = [dict(base, what="render_tile 16 spp", traced_rays=int(st["traced_rays"]), ms=round(float(np.median(ms["render"])), 3),
                     ms_min=round(min(ms["render"]), 3), ms_max=round(max(ms["render"]), 3),
                     traced_rays_per_s=round(render_rate), ratio_to_render=1.0)]
        for f in FORMS:
            med = float(np.median(ms[f]))
            rate = counts[1] / (med * 1e-3)
            rows.append(dict(base, what="trace_radiance " + f, traced_rays=int(counts[1]), queries=int(counts[0]),
                             paths=int(counts[2]), nan_queries=int(counts[3]), ms=round(med, 3), ms_min=round(min(ms[f]), 3),
                             ms_max=round(max(ms[f]), 3), traced_rays_per_s=round(rate),
                             ratio_to_render=round(rate / render_rate, 4), forms_equal_bits=bool(same)))
        for row in rows:
            print(json.dumps(row), flush=True)
        results += rows

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump({"command": "python scripts/radiance_probe.py " + " ".join(sys.argv[1:3]), "rows": results}, f, indent=1)
    f.write("\n")
