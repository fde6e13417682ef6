"""One timed 1920x1080 frame of the simple render kernel (k_render, WGT_KERNEL=1) per mesh stand-in,
through the library's own timed path (wgt_render_tiles_profile: device events around the launch),
after one warm-up frame.  Needs a GPU.  Prints one JSON line per scene with the library's build id;
for an A/B of two builds run it once per build and repetition, alternating the builds:
  for i in $(seq 10); do for so in ab/parent.so ab/branch.so; do
    WGT_LIB_PATH=$PWD/$so python scripts/simple_frame_probe.py; done; done
  python scripts/simple_frame_probe.py [scenes=bunny,sponza] [spp=16]"""
import json
import os
import sys

os.environ["WGT_KERNEL"] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import webgputracer_amd as w  # noqa: E402

scenes = (sys.argv[1] if len(sys.argv) > 1 else "bunny,sponza").split(",")
spp = int(sys.argv[2]) if len(sys.argv) > 2 else 16
W, H = 1920, 1080
if w.device_count() < 1:
    sys.exit("simple_frame_probe: no HIP device")
tiles = w.tile_grid(W, H, W)
d_t = torch.from_numpy(tiles.view(np.uint8).copy()).to(torch.device("cuda", 0))
cam = w.camera_param(W / H, spp, 0)
with w.Context(0) as ctx:
    for scene in scenes:
        ctx.upload_scene(*w.mesh_scene(scene))
        ctx.render_tiles_profile(cam, W, H, W, H, d_t.data_ptr(), len(tiles))
        pr = ctx.render_tiles_profile(cam, W, H, W, H, d_t.data_ptr(), len(tiles))
        print(json.dumps({"scene": scene, "kernel": "k_render", "spp": spp, "ms": round(pr["kernel_ms"], 3),
                          "build_id": w.build_id()}), flush=True)
