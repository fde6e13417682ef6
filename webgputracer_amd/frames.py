"""Multi-frame launcher (BASELINE config C5): a frame range
rendered by one process per GPU, frames dealt round-robin, no collective.

Replaces the reference's machine split (settings/run.py:11-24: frames 1-320 on
one host, 321-600 on another, each running `WebGPUTracer --frame s e`,
main.cpp:17-33) inside one node.  `--frame s e` means the frames
i = s-1 ... e-1 written as "%03d.png" % i (Renderer::OnCompute's loop
`for (i = start_frame - 1; i < end_frame; ++i) OnRender(i)`, render.cpp:437-439,
and the file name of OnRender, render.cpp:493-497), so `--frame 1 600` writes
000.png ... 599.png; rank r of N renders the frames i with (i - (s-1)) % N == r.
The camera is static (Camera::Update ignores t, camera.cpp:64-70), so frames
differ only by their seed: seed = frame index i (the reference draws
std::random_device, util.h:43-47; the C++ CLI's --fixed-seed uses the same i).

Frames are rendered B per launch (one full-frame tile per frame, each with its
frame's seed), so the persistent kernel's end-of-launch drain is paid once per B
frames instead of once per frame, and consecutive launches alternate over the
context's two pipeline streams: batch k+1 starts in batch k's
drain, while the host encodes batch k-1's PNGs.  Every frame is bit-identical to a
single-frame render.

`--gbuffer` also writes NNN_gbuffer.npz next to each NNN.png: the first-hit G-buffer of the frame
(Context.render_gbuffer with the frame's camera and seed), the guides a denoiser asks for.
`--denoise` also writes NNN_denoised.png: the frame through wgt_denoise (an edge-avoiding a-trous
filter guided by that G-buffer), computed on the device on the batch's stream.
`--accumulate` also writes NNN_accum.png: the frames accumulated over time in frame order
(wgt_temporal_accumulate: each frame's history reprojected through its G-buffer, capped at
`--max-history` frames), and with `--denoise` NNN_accum_denoised.png; one process only, because the
ranks of a distributed run see no consecutive frames.
`--denoise-variance` (with `--accumulate`) also writes NNN_accum_vdenoised.png: the accumulated state
through wgt_denoise_variance, the filter whose luminance weight follows each pixel's variance.
`--adaptive` (with `--accumulate`) renders frame 0 uniformly at `--spp` and every later frame with the
sample map wgt_sample_plan makes of the previous frame's accumulated state, capped at `--budget-spp`
samples per pixel on average (default: `--spp`); one frame per launch, all on one stream.

`--panorama` writes NNN_pano.png instead: an equirectangular image, width x width/2, seen from the camera's
origin, a camera the reference's pinhole cannot express.  Pixel (x, y) looks along
panorama_directions(W, H)[y, x]; its `--spp` paths start from the state x + y*W + frame*W*H and go through
Context.trace_radiance (wgt_trace_radiance); the colour is stored as the renderer stores it (unorm8).
`--hit-count` writes NNN_hits.png instead: grey, the number of surfaces along each pixel's G-buffer ray
(Context.trace_multi_hits on the rays render_gbuffer exports, every primitive counted), clipped at 255.

  python -m webgputracer_amd.frames --frame 1 600 --spp 64 --scene bunny --batch 4 --out out/
  python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
      -m webgputracer_amd.frames --frame 1 600 --spp 64 --batch 4 --out out/
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .tracer import Context, camera_param, cornell_scene, mesh_scene, write_png


def frame_indices(start: int, end: int):
    """The frame indices `--frame start end` renders: start-1 ... end-1
    (render.cpp:437, `for (uint32_t i = start_frame - 1; i < end_frame; ++i)`)."""
    if start < 1 or end < start:
        return []
    return list(range(start - 1, end))


def frames_of_rank(start: int, end: int, rank: int, world: int):
    """Frame indices of `--frame start end` (frame_indices) dealt to `rank`:
    round-robin, as even as the range allows."""
    return [f for k, f in enumerate(frame_indices(start, end)) if k % world == rank]


def _cpu_share() -> int:
    """CPUs this process may use, capped by OMP_NUM_THREADS where the launcher sets it."""
    n = len(os.sched_getaffinity(0))
    omp = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    return min(n, omp) if omp > 0 else n


def batches(frames, batch: int):
    return [frames[i:i + batch] for i in range(0, len(frames), max(batch, 1))]


def panorama_directions(W: int, H: int):
    """(H, W, 3) float32 unit directions of an equirectangular image: pixel (x, y) has longitude
    (u - 1/2) 2 pi and latitude (1/2 - v) pi at its centre (u, v) = ((x + 1/2) / W, (y + 1/2) / H), and
    looks along (cos lat sin lon, sin lat, cos lat cos lon): the image's centre looks along +z (the
    reference camera's view), +x is a quarter to the right, -z the left and right edges, +y the top row."""
    lon = ((np.arange(W, dtype=np.float64) + 0.5) / W - 0.5) * (2.0 * np.pi)
    lat = (0.5 - (np.arange(H, dtype=np.float64) + 0.5) / H) * np.pi
    d = np.empty((H, W, 3), np.float64)
    d[..., 0] = np.cos(lat)[:, None] * np.sin(lon)[None, :]
    d[..., 1] = np.sin(lat)[:, None]
    d[..., 2] = np.cos(lat)[:, None] * np.cos(lon)[None, :]
    return d.astype(np.float32)


def panorama_seeds(W: int, H: int, frame: int):
    """(H, W) uint32: pixel (x, y) of frame `frame` starts from x + y*W + frame*W*H (32-bit wrap-around),
    the renderer's per-pixel seed (path_tracer.wgsl:378)."""
    x, y = np.meshgrid(np.arange(W, dtype=np.uint64), np.arange(H, dtype=np.uint64))
    return ((x + y * W + np.uint64(frame) * np.uint64(W * H)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def unorm8(x):
    """The renderer's rgba8unorm store of an fp32 value: floor(min(max(x, 0), 1) * 255 + 0.5) in fp32,
    a NaN as 0."""
    x = np.asarray(x, np.float32)
    c = np.where(x > 0, x, np.float32(0))
    c = np.where(c < 1, c, np.float32(1))
    return np.floor(c * np.float32(255) + np.float32(0.5)).astype(np.uint8)


def render_panorama(ctx: Context, W: int, spp: int, frame: int, origin=(278.0, 278.0, -800.0)):
    """(W/2, W, 4) uint8: frame `frame` of the equirectangular camera at `origin` (see --panorama)."""
    H = W // 2
    d = panorama_directions(W, H).reshape(-1, 3)
    o = np.broadcast_to(np.asarray(origin, np.float32), d.shape)
    rgb = ctx.trace_radiance(o, d, seeds=panorama_seeds(W, H, frame).reshape(-1), samples=spp, want=("rgb",))["rgb"]
    img = np.full((H, W, 4), 255, np.uint8)
    img[..., :3] = unorm8(rgb).reshape(H, W, 3)
    return img


def render_hit_count(ctx: Context, W: int, H: int, spp: int, frame: int):
    """(H, W, 4) uint8 grey image: the number of surfaces along each pixel's G-buffer ray (sample 0's primary
    ray of frame `frame`, as render_gbuffer exports it), every primitive the ray hits counted
    (Context.trace_multi_hits, count only), clipped at 255 (see --hit-count)."""
    g = ctx.render_gbuffer(camera_param(W / H, spp, frame), W, H, want=("prim",), rays=True)
    count = ctx.trace_multi_hits(g["origin"].reshape(-1, 3), g["direction"].reshape(-1, 3), 0, want=("count",))["count"]
    img = np.full((H, W, 4), 255, np.uint8)
    img[..., :3] = np.minimum(count, 255).astype(np.uint8).reshape(H, W, 1)
    return img


class FrameRenderer:
    """Renders batches of whole frames on one GPU: render() is one synchronous launch
    per batch (wgt_render_frames); stream() pipelines the batches (a launch per batch
    on the context's pipeline streams)."""

    def __init__(self, ctx: Context, W: int, H: int, spp: int):
        self.ctx, self.W, self.H, self.spp = ctx, W, H, spp
        self.cam = camera_param(W / H, spp, 0)  # per-frame seeds override cam.seed

    def render(self, frames):
        """{frame: (H, W, 4) uint8} for the batch `frames`, seed = frame index."""
        out = self.ctx.render_frames(self.cam, self.W, self.H, np.asarray(frames, np.uint32))
        return {f: out[j] for j, f in enumerate(frames)}

    def gbuffer(self, frame: int):
        """The frame's first-hit G-buffer (one render_gbuffer call with the frame's camera and
        seed) under a denoiser's names: prim, depth (the hit distance), pos, normal, albedo, flags."""
        g = self.ctx.render_gbuffer(camera_param(self.W / self.H, self.spp, frame), self.W, self.H)
        return {"prim": g["prim"], "depth": g["dist"], "pos": g["pos"], "normal": g["norm"], "albedo": g["col"],
                "flags": g["flags"]}

    def stream(self, frame_batches, depth: int = 2, denoised=None, accumulated=None, max_history=None,
               accumulated_denoised=None, accumulated_vdenoised=None):
        """Yield (batch, {frame: (H, W, 4) uint8}) for each batch of `frame_batches`, in
        order.  Batch k renders on pipeline stream k % depth into buffer set k % depth;
        it is issued before batch k-1 is handed out, so the device always has the next
        launch queued behind the running one.  Host copies are made on the batch's own
        stream once its launch is done (no pinned buffers: torch's host allocator would
        outlive the context's streams).

        denoised: a dict that receives {frame: (H, W, 4) uint8} of each batch as it is handed out,
        the frame through wgt_denoise with the default parameters.  The batch's launch then also
        fills a device rgba32f buffer, and each of its frames gets, on the batch's stream, its
        G-buffer (render_gbuffer_async with the frame's one tile) and denoise_async to a device
        rgba8 buffer; nothing leaves the device but the two rgba8 images.

        accumulated: a dict that receives {frame: (H, W, 4) uint8}, the frames accumulated over time in
        the order they are rendered (wgt_temporal_accumulate with `max_history`, the camera being
        static), each after its G-buffer on its batch's stream.  The history is one sequence: two
        state sets and two G-buffer sets that alternate frame by frame across batches and pipeline
        slots, and each slot's rgba8 outputs.  Frame k is accumulated after frame k - 1 also when
        the two belong to batches on different pipeline streams: a batch's stream waits, after its
        render launch and before its first G-buffer, for an event recorded behind the previous
        batch's last accumulation, so the renders still overlap and only the short accumulation
        passes are serialised.  accumulated_denoised: a dict that also receives the accumulated
        radiance through denoise_async.  accumulated_vdenoised: a dict that also receives the
        accumulated state through denoise_variance_async (default parameters), on the same stream
        right behind the accumulation."""
        import torch

        from ._lib import TILE_DTYPE
        from .tracer import denoise_variance_workspace_bytes, denoise_workspace_bytes

        dev = torch.device("cuda", self.ctx.device)
        W, H = self.W, self.H
        nmax = max((len(b) for b in frame_batches), default=0)
        if nmax == 0:
            return
        streams = [torch.cuda.ExternalStream(self.ctx.pipeline_stream(i), device=dev) for i in range(depth)]
        d_out = [torch.empty((nmax, H, W, 4), dtype=torch.uint8, device=dev) for _ in range(depth)]
        d_dn = d_acc = d_accdn = d_accvdn = None
        acc = accumulated is not None
        dn_acc = acc and accumulated_denoised is not None
        vdn_acc = acc and accumulated_vdenoised is not None
        n = W * H

        def u8_set():
            return [torch.empty((nmax, H, W, 4), dtype=torch.uint8, device=dev) for _ in range(depth)]

        if denoised is not None or acc:
            d_f32 = [torch.empty((nmax, H, W, 4), dtype=torch.float32, device=dev) for _ in range(depth)]
            # per set: one frame's guides (reused frame after frame in stream order).  Accumulating, the
            # sets are two for the whole sequence instead: a frame's guides are the next frame's history
            sets = 2 if acc else depth
            d_vec = [torch.empty((3, 3, n), dtype=torch.float32, device=dev) for _ in range(sets)]
            d_prim = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(sets)]
            d_flags = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(sets)]
        if denoised is not None or dn_acc or vdn_acc:
            ws_bytes = max(denoise_workspace_bytes(W, H), denoise_variance_workspace_bytes(W, H))  # one serves both
            d_ws = [torch.empty(ws_bytes, dtype=torch.uint8, device=dev) for _ in range(depth)]
        if denoised is not None:
            d_dn = u8_set()
        if acc:
            d_acc = u8_set()
            d_accdn = u8_set() if dn_acc else None
            d_accvdn = u8_set() if vdn_acc else None
            d_state = [{"f32": torch.empty((H, W, 4), dtype=torch.float32, device=dev),
                        "len": torch.empty(n, dtype=torch.float32, device=dev),
                        "moments": torch.empty((2, n), dtype=torch.float32, device=dev)} for _ in range(2)]
            history = 0       # frames accumulated so far
            last_acc = None   # recorded behind the previous batch's last accumulation
        copies = [(d_dn, denoised), (d_acc, accumulated), (d_accdn, accumulated_denoised),
                  (d_accvdn, accumulated_vdenoised)]
        pending = []
        for k, b in enumerate(frame_batches):
            j = k % depth
            if len(pending) == depth:  # the oldest batch in flight holds set j: hand it out first
                yield self._finish(pending.pop(0), streams, d_out, copies)
            s = streams[j]
            t = np.zeros(len(b), TILE_DTYPE)  # one full-frame tile per frame (wgt_render_frames' list)
            t["seed"] = np.asarray(b, np.uint32)
            t["frame"] = np.arange(len(b), dtype=np.uint32)
            with torch.cuda.stream(s):
                d_tiles = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
                self.ctx.render_tiles_async(self.cam, W, H, W, H, d_tiles.data_ptr(), len(b),
                                            d_u8=d_out[j].data_ptr(),
                                            d_f32=d_f32[j].data_ptr() if d_dn or acc else 0, stream=s.cuda_stream)
                if acc and last_acc is not None:
                    s.wait_event(last_acc)  # frame order across the pipeline streams
                for i in range(len(b) if d_dn or acc else 0):
                    q = history % 2 if acc else j
                    guides = {"prim": d_prim[q].data_ptr(), "pos": d_vec[q][0].data_ptr(),
                              "norm": d_vec[q][1].data_ptr(), "col": d_vec[q][2].data_ptr(),
                              "flags": d_flags[q].data_ptr()}
                    self.ctx.render_gbuffer_async(self.cam, W, H, W, H, d_tiles.data_ptr() + i * TILE_DTYPE.itemsize, 1,
                                                  stream=s.cuda_stream, **guides)
                    if d_dn:
                        self.ctx.denoise_async(W, H, d_f32[j][i].data_ptr(), d_ws[j].data_ptr(), ws_bytes,
                                               d_u8_out=d_dn[j][i].data_ptr(), stream=s.cuda_stream, **guides)
                    if acc:
                        p = 1 - q
                        before = {"prim": d_prim[p].data_ptr(), "pos": d_vec[p][0].data_ptr(),
                                  "norm": d_vec[p][1].data_ptr(), "flags": d_flags[p].data_ptr()}
                        out = {key: t.data_ptr() for key, t in d_state[q].items()}
                        prev = {key: t.data_ptr() for key, t in d_state[p].items()}
                        self.ctx.temporal_accumulate_async(
                            W, H, self.cam, d_f32[j][i].data_ptr(), guides, out, prev if history else None,
                            before if history else None, self.cam if history else None,
                            d_u8_out=d_acc[j][i].data_ptr(), max_history=max_history, stream=s.cuda_stream)
                        if dn_acc:
                            self.ctx.denoise_async(W, H, out["f32"], d_ws[j].data_ptr(), ws_bytes,
                                                   d_u8_out=d_accdn[j][i].data_ptr(), stream=s.cuda_stream, **guides)
                        if vdn_acc:
                            # the same workspace right behind the plain filter: one stream orders them
                            self.ctx.denoise_variance_async(W, H, out, d_ws[j].data_ptr(), ws_bytes,
                                                            d_u8_out=d_accvdn[j][i].data_ptr(), stream=s.cuda_stream,
                                                            **guides)
                        history += 1
                if acc:
                    last_acc = torch.cuda.Event()
                    last_acc.record(s)
                d_tiles.record_stream(s)
            pending.append((k, b))
        while pending:
            yield self._finish(pending.pop(0), streams, d_out, copies)

    def stream_adaptive(self, frames, max_history=None, budget_spp=None, totals=None, **plan_params):
        """Yield (frame, (H, W, 4) uint8 rendered, (H, W, 4) uint8 accumulated) for each of `frames`, in
        order, rendering adaptively: the first frame uniformly at this renderer's spp, every later
        frame with the sample map planned (wgt_sample_plan_async, `budget_spp` and `plan_params`) from
        the state the previous frame left, its G-buffer with the same map.  A frame needs the frame
        before it, so there is one frame per launch, and everything (render, G-buffer, accumulation,
        plan) is queued on one pipeline stream: nothing leaves the device but the two rgba8 images and
        the map's total.  budget_spp None: this renderer's spp, so no frame spends more than the plain
        run's.  totals: a dict that receives {frame: samples traced}."""
        import torch

        from ._lib import TILE_DTYPE
        from .tracer import sample_plan_workspace_bytes

        dev = torch.device("cuda", self.ctx.device)
        W, H = self.W, self.H
        n = W * H
        s = torch.cuda.ExternalStream(self.ctx.pipeline_stream(0), device=dev)
        budget = float(self.spp if budget_spp is None else budget_spp)
        side = int(np.sqrt(np.float32(self.spp)))  # the uniform frame's side: floor(sqrt(f32(spp))), as the kernels'
        with torch.cuda.stream(s):
            d_u8 = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
            d_acc = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
            d_f32 = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
            d_vec = [torch.empty((2, 3, n), dtype=torch.float32, device=dev) for _ in range(2)]
            d_prim = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2)]
            d_flags = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2)]
            d_state = [{"f32": torch.empty((H, W, 4), dtype=torch.float32, device=dev),
                        "len": torch.empty(n, dtype=torch.float32, device=dev),
                        "moments": torch.empty((2, n), dtype=torch.float32, device=dev)} for _ in range(2)]
            d_map = torch.empty(n, dtype=torch.uint8, device=dev)
            d_total = torch.zeros(1, dtype=torch.int64, device=dev)
            ws_bytes = sample_plan_workspace_bytes(W, H)
            d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        for history, f in enumerate(frames):
            with torch.cuda.stream(s):  # left before the frame is handed out: the caller's stream stays its own
                t = np.zeros(1, TILE_DTYPE)
                t["seed"] = f
                d_tile = torch.from_numpy(t.view(np.uint8).copy()).to(dev)
                q, p = history % 2, 1 - history % 2
                smap = d_map.data_ptr() if history else 0  # frame 0: uniform, cam's spp
                guides = {"prim": d_prim[q].data_ptr(), "pos": d_vec[q][0].data_ptr(), "norm": d_vec[q][1].data_ptr(),
                          "flags": d_flags[q].data_ptr()}
                before = {"prim": d_prim[p].data_ptr(), "pos": d_vec[p][0].data_ptr(), "norm": d_vec[p][1].data_ptr(),
                          "flags": d_flags[p].data_ptr()}
                out = {key: b.data_ptr() for key, b in d_state[q].items()}
                prev = {key: b.data_ptr() for key, b in d_state[p].items()}
                self.ctx.render_tiles_async(self.cam, W, H, W, H, d_tile.data_ptr(), 1, d_u8=d_u8.data_ptr(),
                                            d_f32=d_f32.data_ptr(), stream=s.cuda_stream, d_sample_map=smap)
                self.ctx.render_gbuffer_async(self.cam, W, H, W, H, d_tile.data_ptr(), 1, stream=s.cuda_stream,
                                              d_sample_map=smap, **guides)
                self.ctx.temporal_accumulate_async(W, H, self.cam, d_f32.data_ptr(), guides, out, prev if history else None,
                                                   before if history else None, self.cam if history else None,
                                                   d_u8_out=d_acc.data_ptr(), max_history=max_history,
                                                   stream=s.cuda_stream)
                spent = int(d_total.cpu()[0]) if history else side * side * n  # the total of the map just rendered with
                # the next frame's map, behind this frame's render on the stream (which has read the old one)
                self.ctx.sample_plan_async(W, H, out, d_ws.data_ptr(), ws_bytes, d_map.data_ptr(), d_total.data_ptr(),
                                           stream=s.cuda_stream, budget_spp=budget, **plan_params)
                img, accum = d_u8.cpu().numpy(), d_acc.cpu().numpy()
                d_tile.record_stream(s)
            if totals is not None:
                totals[f] = spent
            yield f, img, accum

    @staticmethod
    def _finish(kb, streams, d_out, copies=()):
        """Batch k's images on the host; copies: (per-slot device rgba8 buffers, the dict they go to)."""
        import torch

        k, b = kb
        j = k % len(streams)
        with torch.cuda.stream(streams[j]):  # ordered after batch k's launch on its stream
            imgs = d_out[j][:len(b)].cpu().numpy()
            for d_buf, into in copies:
                if d_buf is not None:
                    host = d_buf[j][:len(b)].cpu().numpy()
                    into.update({f: host[i] for i, f in enumerate(b)})
        return b, {f: imgs[i] for i, f in enumerate(b)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frame", nargs=2, type=int, default=[1, 1], metavar=("START", "END"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--scene", default="bunny", help="bunny | sponza | cornell | obj:<path>")
    ap.add_argument("--batch", type=int, default=4,
                    help="frames per launch (4 with 2 in flight: 33.0 frames/s, 31.6 at 8, 31.1 at 1; "
                         "profiles/configs/r02_c5_frames.jsonl)")
    ap.add_argument("--pipeline", type=int, default=2, help="batches in flight (1..4, DESIGN.md §4.2a)")
    ap.add_argument("--out", default=None, help="directory for NNN.png (none: render only)")
    ap.add_argument("--png-threads", type=int, default=0,
                    help="PNG encoder threads (0: this process's CPU share, capped by OMP_NUM_THREADS and 16)")
    ap.add_argument("--gbuffer", action="store_true",
                    help="also write NNN_gbuffer.npz next to each NNN.png: prim, depth, pos, normal, albedo, flags "
                         "of each pixel's first hit (guides for a denoiser)")
    ap.add_argument("--denoise", action="store_true",
                    help="also write NNN_denoised.png next to each NNN.png: the frame through the edge-avoiding "
                         "a-trous filter (wgt_denoise, default parameters), guided by its G-buffer on the device")
    ap.add_argument("--accumulate", action="store_true",
                    help="also write NNN_accum.png: the frames accumulated over time in frame order by reprojecting "
                         "the history (wgt_temporal_accumulate) on the device; with --denoise also "
                         "NNN_accum_denoised.png, the accumulated radiance through the filter")
    ap.add_argument("--denoise-variance", action="store_true",
                    help="with --accumulate, also write NNN_accum_vdenoised.png: the accumulated state through the "
                         "variance-guided filter (wgt_denoise_variance, default parameters) on the device")
    ap.add_argument("--adaptive", action="store_true",
                    help="with --accumulate: render frame 0 uniformly at --spp and every later frame with the sample "
                         "map planned from the previous frame's accumulated state (wgt_sample_plan, default "
                         "parameters), all on the device; one frame per launch, one process, without --denoise, "
                         "--denoise-variance and --gbuffer")
    ap.add_argument("--budget-spp", type=float, default=None,
                    help="--adaptive: the map's mean samples per pixel may not exceed this (default: --spp, so the "
                         "option never spends more than the plain run)")
    ap.add_argument("--panorama", action="store_true",
                    help="write NNN_pano.png instead of NNN.png: an equirectangular image, --width x --width/2, from "
                         "the camera's origin, --spp paths per pixel through wgt_trace_radiance; without the other "
                         "outputs")
    ap.add_argument("--hit-count", action="store_true",
                    help="write NNN_hits.png instead of NNN.png: the number of surfaces along each pixel's G-buffer "
                         "ray through wgt_trace_multi_hits, clipped at 255; without the other outputs")
    ap.add_argument("--max-history", type=int, default=32, help="--accumulate: the history length's cap (1..65536)")
    a = ap.parse_args(argv)
    if a.gbuffer and not a.out:
        ap.error("--gbuffer needs --out")
    if a.denoise and not a.out:
        ap.error("--denoise needs --out")
    if a.accumulate and not a.out:
        ap.error("--accumulate needs --out")
    if a.denoise_variance and not (a.accumulate and a.out):
        ap.error("--denoise-variance needs --accumulate and --out: it filters the accumulated state")
    if a.adaptive and not a.accumulate:
        ap.error("--adaptive needs --accumulate: the map is planned from the accumulated state")
    if a.adaptive and (a.denoise or a.denoise_variance or a.gbuffer):
        ap.error("--adaptive runs without --denoise, --denoise-variance and --gbuffer")
    if a.budget_spp is not None and not (a.adaptive and a.budget_spp > 0 and a.budget_spp < float("inf")):
        ap.error("--budget-spp needs --adaptive and a finite value > 0")
    if a.accumulate and not 1 <= a.max_history <= 65536:
        ap.error("--max-history must be 1..65536")
    if a.accumulate and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        ap.error("--accumulate needs consecutive frames: frames are dealt round-robin to the ranks, so run it "
                 "in one process (WORLD_SIZE = 1)")
    if a.panorama and (a.gbuffer or a.denoise or a.accumulate or a.denoise_variance or a.adaptive):
        ap.error("--panorama runs without --gbuffer, --denoise, --accumulate, --denoise-variance and --adaptive")
    if a.panorama and not (a.out and a.width >= 2 and 0 <= a.spp <= 65536):
        ap.error("--panorama needs --out, --width >= 2 and --spp within 0..65536")
    if a.hit_count and (a.panorama or a.gbuffer or a.denoise or a.accumulate or a.denoise_variance or a.adaptive):
        ap.error("--hit-count runs without --panorama, --gbuffer, --denoise, --accumulate, --denoise-variance and "
                 "--adaptive")
    if a.hit_count and not a.out:
        ap.error("--hit-count needs --out")
    if a.frame[0] < 1 or a.frame[1] < a.frame[0]:
        ap.error("bad frame range")  # the C++ CLI's check (csrc/main.cpp)
    if not 1 <= a.pipeline <= 4:
        ap.error("--pipeline must be 1..4 (the context has 4 pipeline streams)")
    if a.batch < 1:
        ap.error("--batch must be >= 1")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import torch

    # one process per GPU; ranks beyond the visible GPUs share them (rehearsals, tests)
    local = int(os.environ.get("LOCAL_RANK", "0")) % max(torch.cuda.device_count(), 1)
    if a.scene == "cornell":
        scene = cornell_scene()
    elif a.scene.startswith("obj:"):
        scene = mesh_scene("bunny", obj_path=a.scene[4:])
    else:
        scene = mesh_scene(a.scene)
    ctx = Context(local)
    ctx.upload_scene(*scene)
    fr = FrameRenderer(ctx, a.width, a.height, a.spp)
    mine = frames_of_rank(a.frame[0], a.frame[1], rank, world)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    # PNG encoding (zlib on the host, ~0.5 s per 1080p frame) runs on a thread pool while the GPU
    # renders the next batches (wgt_write_png is a ctypes call: it releases the GIL); at most
    # 4 frames per writer are held
    workers = max(1, a.png_threads or min(_cpu_share(), 16))
    pool = ThreadPoolExecutor(max_workers=workers) if a.out else None
    pending = collections.deque()
    t0 = time.perf_counter()
    denoised = {} if a.denoise else None
    accumulated = {} if a.accumulate else None
    accumulated_denoised = {} if a.accumulate and a.denoise else None
    accumulated_vdenoised = {} if a.accumulate and a.denoise_variance else None
    totals = {}
    if a.panorama:
        for f in mine:
            pending.append(pool.submit(write_png, os.path.join(a.out, f"{f:03d}_pano.png"),
                                       render_panorama(ctx, a.width, a.spp, f)))
    elif a.hit_count:
        for f in mine:
            pending.append(pool.submit(write_png, os.path.join(a.out, f"{f:03d}_hits.png"),
                                       render_hit_count(ctx, a.width, a.height, a.spp, f)))
    elif a.adaptive:
        for f, img, accum in fr.stream_adaptive(mine, max_history=a.max_history, budget_spp=a.budget_spp, totals=totals):
            pending.append(pool.submit(write_png, os.path.join(a.out, f"{f:03d}.png"), img))
            pending.append(pool.submit(write_png, os.path.join(a.out, f"{f:03d}_accum.png"), accum))
            while len(pending) > 4 * workers:
                pending.popleft().result()
    else:
        for b, imgs in fr.stream(batches(mine, a.batch), depth=a.pipeline, denoised=denoised, accumulated=accumulated,
                                 max_history=a.max_history, accumulated_denoised=accumulated_denoised,
                                 accumulated_vdenoised=accumulated_vdenoised):
            if a.out:
                for f in b:  # render.cpp:494-497
                    pending.append(pool.submit(write_png, os.path.join(a.out, f"{f:03d}.png"), imgs[f]))
                    for suffix, extra in (("denoised", denoised), ("accum", accumulated),
                                          ("accum_denoised", accumulated_denoised),
                                          ("accum_vdenoised", accumulated_vdenoised)):
                        if extra is not None:
                            pending.append(pool.submit(write_png, os.path.join(a.out, f"{f:03d}_{suffix}.png"),
                                                       extra.pop(f)))
                    if a.gbuffer:
                        np.savez(os.path.join(a.out, f"{f:03d}_gbuffer.npz"), **fr.gbuffer(f))
                while len(pending) > 4 * workers:
                    pending.popleft().result()
    while pending:
        pending.popleft().result()
    dt = time.perf_counter() - t0
    if pool:
        pool.shutdown()
    torch.cuda.synchronize()
    print(json.dumps({"rank": rank, "world": world, "frames": len(mine), "batch": a.batch, "pipeline": a.pipeline,
                      "seconds": round(dt, 3), **({"adaptive_samples": sum(totals.values())} if a.adaptive else {}),
                      "frames_per_s": round(len(mine) / dt, 3) if dt > 0 else None}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
