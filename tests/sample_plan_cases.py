"""States for the sample-map planner's tests (test infrastructure only), shared by
tests/test_sample_plan_restatement.py and tests/test_gpu_sample_plan.py: synthetic ones that take every
branch of the specification, and accumulated Cornell frames of the CPU oracle.
"""
import numpy as np

import hit_records as hr
import temporal_restatement as tr

f32 = np.float32
SIZES = [(37, 21), (64, 64)]  # W x H: no multiple of the 64 x 4 workgroup, and several workgroups


def synthetic(w, h, seed):
    """len: 0, below and at min_history, fractions, NaN, inf, -0, negative.  Moments: 0; m2 below m1^2
    (max0); 2^100 and the next float above it, either sign; inf and NaN; m1 = 0 under a huge m2
    (rel * gain far above 255, and inf through a denormal lum_floor); the four corners want the most."""
    rng = np.random.default_rng(seed)
    n = w * h
    length = rng.choice(np.array([0.0, 0.0, 0.5, 1.0, 2.0, 3.0, 3.5, 4.0, 4.0, 7.0, 7.0, 31.0, 64.0, 65536.0], f32), n)
    for bad in (np.nan, np.inf, -np.inf, -0.0, -3.0):
        length[rng.random(n) < 0.02] = bad
    m1 = rng.gamma(0.7, 0.5, n).astype(f32)
    m2 = (m1 * m1 + (rng.gamma(0.3, 0.2, n) * rng.choice([0.0, 0.01, 1.0, 30.0], n)).astype(f32)).astype(f32)
    k = rng.random(n) < 0.1
    m2[k] = (m1[k] * m1[k] * f32(0.9)).astype(f32)  # below m1^2
    for which in (m1, m2):
        which[rng.random(n) < 0.05] = 0.0
        for bad in (2.0 ** 100, np.nextafter(f32(2.0 ** 100), f32(np.inf)), -(2.0 ** 100), np.inf, -np.inf, np.nan, -0.0,
                    1e-40, 3e38):
            which[rng.random(n) < 0.01] = bad
    k = rng.random(n) < 0.03
    m1[k], m2[k] = 0.0, 1e30
    m1[rng.random(n) < 0.03] *= -1.0
    length, m1, m2 = length.reshape(h, w), m1.reshape(h, w), m2.reshape(h, w)
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        length[y, x], m1[y, x], m2[y, x] = 8.0, 0.0, 1e20
    return {"len": length, "moments": np.stack([m1, m2]).astype(f32)}


def quiet_corners(w, h):
    """Everything measured and converged but the four corners, which want the most: what dilation spreads."""
    st = {"len": np.full((h, w), 8.0, f32), "moments": np.stack([np.full((h, w), 0.5, f32), np.full((h, w), 0.25, f32)])}
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
        st["moments"][:, y, x] = (0.0, 1e20)
    return st


def cornell_frames(oracle, w, h, spp, seeds, ref_spp=None):
    """The oracle's Cornell frames at `spp` for `seeds` (one camera), the first-hit guides of seeds[0]'s
    camera rays, the scene, and a `ref_spp` frame when asked for."""
    from test_gpu_gbuffer import camera_rays

    L, Q, S = oracle.cornell_scene()
    scene = oracle.OracleScene(L, Q, S)
    cams = [oracle.camera_param(w / h, spp, s) for s in seeds]
    colors = [scene.render(c, w, h, want=("f32",))["f32"] for c in cams]
    o, d = camera_rays(cams[0], w, h)
    rec = hr.quad_sphere_records(o.reshape(-1, 3), d.reshape(-1, 3), L, Q, S)
    g = {k: rec[k].reshape((h, w) + rec[k].shape[1:]) for k in ("prim", "flags", "pos", "norm", "col")}
    ref = scene.render(oracle.camera_param(w / h, ref_spp, 77), w, h, want=("f32",))["f32"] if ref_spp else None
    return scene, cams, colors, g, ref


def cornell_states(oracle, w, h, spp=4, frames=5):
    """The states after 1..frames oracle frames chained through the numpy temporal restatement."""
    _, cams, colors, g, _ = cornell_frames(oracle, w, h, spp, range(frames))
    states, prev = [], None
    for c in colors:
        prev = tr.accumulate(c, g, cams[0], prev, None if prev is None else g, None if prev is None else cams[0])
        states.append(prev)
    return states


def render_with_map(oracle, scene, w, h, seed, smap):
    """The oracle's frame under a sample map: each distinct side's pixels from a frame at that side's spp
    (rows that hold none of them are not rendered)."""
    out = np.zeros((h, w, 4), f32)
    for k in np.unique(smap):
        rows = np.flatnonzero((smap == k).any(axis=1))
        y0, y1 = int(rows[0]), int(rows[-1]) + 1
        r = scene.render(oracle.camera_param(w / h, int(k) * int(k), seed), w, h, 0, y0, w, y1 - y0, want=("f32",))["f32"]
        sel = smap[y0:y1] == k
        out[y0:y1][sel] = r[sel]
    return out


def clamped_mse(img, ref):
    return float(np.mean((np.minimum(img[..., :3], 1) - np.minimum(ref[..., :3], 1)) ** 2, dtype=np.float64))
