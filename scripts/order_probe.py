"""K frames of one view with seed = frame index, alternated over the context's two pipeline streams
(wgt_render_tiles_async), with the queue order made per launch (WGT_PQ_REUSE=0) and shared across the
launches of the view (WGT_PQ_REUSE=1).  Unlike bench.py's steps the frames
differ: every launch has its own seeds, and a launch reads its tile list while it runs, so two frames
in flight need two lists.
  lists = 2 (default): stream j's frames rewrite list j's seeds on stream j (behind their predecessor
                       there).  The two addresses alternate, which the planner takes for two views.
  lists = 1:           one list and fixed seeds, bench.py's case, as the upper bound.
Prints one JSON line per mode and repeat: wall ms per frame and how the launches got their order.
  python scripts/order_probe.py [scene] [W H spp] [K] [reps] [lists]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import webgputracer_amd as w  # noqa: E402

scene = sys.argv[1] if len(sys.argv) > 1 else "sponza"
W, H, spp = (int(v) for v in sys.argv[2:5]) if len(sys.argv) > 4 else (1920, 1080, 256)
K = int(sys.argv[5]) if len(sys.argv) > 5 else 12
REPS = int(sys.argv[6]) if len(sys.argv) > 6 else 3
LISTS = int(sys.argv[7]) if len(sys.argv) > 7 else 2
T = 32
dev = torch.device("cuda", 0)
ctx = w.Context(0)
ctx.upload_scene(*w.mesh_scene(scene))
cam = w.camera_param(W / H, spp, 0)
tiles = w.tile_grid(W, H, T, seed=0)
nt = len(tiles)
d_tiles = [torch.from_numpy(tiles.view(np.uint8).copy()).to(dev) for _ in range(LISTS)]
# the seed column of a list as a strided device view: one fill per frame rewrites it
seed_col = [d.view(torch.int32).view(nt, 4)[:, 2] for d in d_tiles]
outs = [torch.zeros((nt, T, T, 4), dtype=torch.uint8, device=dev) for _ in range(2)]
streams = [torch.cuda.ExternalStream(ctx.pipeline_stream(i), device=dev) for i in range(2)]
for rep in range(REPS):
    for reuse in (0, 1):
        os.environ["WGT_PQ_REUSE"] = str(reuse)
        ctx.order_reset()
        before = ctx.order_info()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(K):
            s, j = streams[k % 2], k % LISTS
            if LISTS == 2:
                with torch.cuda.stream(s):
                    seed_col[j].fill_(k)
            ctx.render_tiles_async(cam, W, H, T, T, d_tiles[j].data_ptr(), nt, d_u8=outs[k % 2].data_ptr(),
                                   stream=s.cuda_stream)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        after = ctx.order_info()
        print(json.dumps({"scene": scene, "W": W, "H": H, "spp": spp, "frames": K, "lists": LISTS, "reuse": reuse,
                          "rep": rep, "ms_per_frame": round(dt / K * 1e3, 3),
                          "today": after["today"] - before["today"], "refine": after["refine"] - before["refine"],
                          "reused": after["reuse"] - before["reuse"], "refine_side": after["refine_side"]}),
              flush=True)
ctx.close()
