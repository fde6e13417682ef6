"""The motion passes' specification restated in numpy float32 (test infrastructure only):
wgt_motion_reproject and wgt_temporal_accumulate_motion, operation by operation.
Every operation is an IEEE binary32 operation, none is fused, denormals are kept; the GPU results equal
reproject() and accumulate_motion() bit for bit.

Triangles are TRI_DTYPE record arrays in original order (v0, e1, e2, face_norm are read): `now` what
is resident, `before` what the snapshot holds.  Guides and states are shaped as in
tests/temporal_restatement.py.
"""
import numpy as np

import temporal_restatement as tr
from denoise_restatement import dot3, ok

f32 = np.float32
FRONT_FACE = 2  # WGT_HIT_FRONT_FACE


def cross(a, b):
    """include/wgt/vec.h cross: each product and each difference one rounded operation."""
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _xyz(tris, field, t, dtype):
    return np.ascontiguousarray(tris[field][t][:, :3]).astype(dtype)


def reproject(g, nlq, now, before, dtype=f32):
    """wgt_motion_reproject: {"pos_prev", "norm_prev"} shaped as g["pos"].  dtype=np.float64 evaluates
    the same formula in float64 from the same float32 inputs (the accuracy tests' reference)."""
    shape = np.asarray(g["pos"]).shape
    prim = np.asarray(g["prim"], np.uint32).reshape(-1).astype(np.int64)
    flags = np.asarray(g["flags"], np.uint8).reshape(-1)
    pos = np.asarray(g["pos"], f32).reshape(-1, 3)
    norm = np.asarray(g["norm"], f32).reshape(-1, 3)
    pp, npv = pos.astype(dtype), norm.astype(dtype)
    n_tris = len(now)
    assert len(before) == n_tris
    k = np.flatnonzero((prim >= nlq) & (prim < nlq + n_tris))  # every other id passes through, nothing indexed
    t = prim[k] - nlq
    with np.errstate(all="ignore"):
        v0, e1, e2, fn = (_xyz(now, f, t, dtype) for f in ("v0", "e1", "e2", "face_norm"))
        pv0, pe1, pe2, pfn = (_xyz(before, f, t, dtype) for f in ("v0", "e1", "e2", "face_norm"))
        moved = ~((v0 == pv0).all(axis=1) & (e1 == pe1).all(axis=1) & (e2 == pe2).all(axis=1))  # a NaN is unequal
        d = pos[k].astype(dtype) - v0
        nv = cross(e1, e2)
        nf = dot3(nv, fn)
        u = dot3(cross(d, e2), fn) / nf
        v = dot3(cross(e1, d), fn) / nf
        p = (pv0 + u[:, None] * pe1) + v[:, None] * pe2
        front = (flags[k] & FRONT_FACE) != 0
        nn = np.where(front[:, None], pfn, -pfn)
    m = k[moved]
    pp[m], npv[m] = p[moved], nn[moved]
    return {"pos_prev": pp.reshape(shape), "norm_prev": npv.reshape(shape)}


def accumulate_motion(color, g, cam, pos_prev=None, norm_prev=None, prev=None, g_prev=None, cam_prev=None,
                      max_history=32, normal_min=0.9, plane_tol=1.0, match_prim=False, moments=True):
    """wgt_temporal_accumulate_motion: temporal_restatement.accumulate with the previous camera
    projecting pos_prev, no history unless ok(pos_prev) and ok(norm_prev), and the tap tests against
    norm_prev and the plane through pos_prev.  prev, g_prev and cam_prev None: the first frame (pos_prev
    and norm_prev are not looked at)."""
    assert (prev is None) == (g_prev is None) == (cam_prev is None)
    with np.errstate(all="ignore"):
        H, W, _ = color.shape
        cur = color[..., :3].astype(f32)
        valid = tr.valid_mask(color, g)
        lum = tr.luminance(cur)
        wsum = np.zeros((H, W), f32)
        lsum = np.zeros((H, W), f32)
        m1sum = np.zeros((H, W), f32)
        m2sum = np.zeros((H, W), f32)
        csum = np.zeros((H, W, 3), f32)
        if prev is not None:
            pos = g["pos"].astype(f32)
            pp, npv = np.asarray(pos_prev, f32).reshape(H, W, 3), np.asarray(norm_prev, f32).reshape(H, W, 3)
            xc, yc, fc = tr.project(tr.camera_constants(cam, W, H), pos)
            xp, yp, fp = tr.project(tr.camera_constants(cam_prev, W, H), pp)
            hx = (np.arange(W, dtype=f32)[None, :] + (xp - xc)).astype(f32)
            hy = (np.arange(H, dtype=f32)[:, None] + (yp - yc)).astype(f32)
            has = (valid & fc & fp & ok(pp) & ok(npv) & (hx > f32(-1)) & (hx < f32(W)) & (hy > f32(-1)) & (hy < f32(H)))
            hx, hy = np.where(has, hx, f32(0)), np.where(has, hy, f32(0))
            x0f, y0f = np.floor(hx), np.floor(hy)
            fx, fy = (hx - x0f).astype(f32), (hy - y0f).astype(f32)
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            vprev = tr.valid_mask(prev["f32"], g_prev)
            for j in (0, 1):
                for i in (0, 1):
                    b = ((fx if i else f32(1) - fx) * (fy if j else f32(1) - fy)).astype(f32)
                    tx, ty = x0 + i, y0 + j
                    inb = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                    tx, ty = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                    lt = prev["len"][ty, tx].astype(f32)
                    use = (has & (b > 0) & inb & (lt >= f32(1)) & vprev[ty, tx] &
                           (dot3(npv, g_prev["norm"][ty, tx].astype(f32)) >= f32(normal_min)) &
                           (np.abs(dot3(npv, (g_prev["pos"][ty, tx] - pp).astype(f32))) <= f32(plane_tol)))
                    if match_prim:
                        use &= g_prev["prim"][ty, tx] == g["prim"]
                    # an unusable tap adds +0 (the kernel skips it: the sums are never -0, so the same bits)
                    zero = f32(0)
                    wsum = wsum + np.where(use, b, zero)
                    csum = csum + np.where(use[..., None], b[..., None] * prev["f32"][ty, tx, :3].astype(f32), zero)
                    lsum = lsum + np.where(use, b * lt, zero)
                    if moments:
                        m1sum = m1sum + np.where(use, b * prev["moments"][0][ty, tx].astype(f32), zero)
                        m2sum = m2sum + np.where(use, b * prev["moments"][1][ty, tx].astype(f32), zero)
        hist_ok = valid & (wsum >= tr.MIN_WEIGHT)
        hist = (csum / wsum[..., None]).astype(f32)
        up = (lsum / wsum).astype(f32) + f32(1)
        cap = f32(max_history)
        length = np.where(up < cap, up, cap).astype(f32)
        a = (f32(1) / length).astype(f32)
        rgb = np.where(hist_ok[..., None], hist + a[..., None] * (cur - hist), cur).astype(f32)
        out = {"f32": color.astype(f32).copy(),  # alpha, and every pixel outside valid_mask bit for bit
               "len": np.where(valid, np.where(hist_ok, length, f32(1)), f32(0)).astype(f32), "moments": None}
        out["f32"][..., :3][valid] = rgb[valid]
        if moments:
            h1, h2 = (m1sum / wsum).astype(f32), (m2sum / wsum).astype(f32)
            ll = lum * lum
            m1 = np.where(hist_ok, h1 + a * (lum - h1), lum)
            m2 = np.where(hist_ok, h2 + a * (ll - h2), ll)
            out["moments"] = np.stack([np.where(valid, m1, f32(0)), np.where(valid, m2, f32(0))]).astype(f32)
        return out


# ---- the moved meshes of the tests and of DESIGN.md §4.10's measurements ---------------------------

def vertices_of(tris):
    """(n, 9) float32: v0, v0 + e1, v0 + e2 of TRI_DTYPE records."""
    v0, e1, e2 = (np.ascontiguousarray(tris[k][:, :3], f32) for k in ("v0", "e1", "e2"))
    return np.concatenate([v0, v0 + e1, v0 + e2], axis=1).astype(f32)


def translated(verts, step):
    return (verts.reshape(-1, 3) + np.asarray(step, f32)).astype(f32).reshape(-1, 9)


def rotated_y(verts, degrees, centre):
    """Rotation about the y axis through `centre`, in float64, rounded to float32 once."""
    a = np.radians(degrees)
    p = verts.reshape(-1, 3).astype(np.float64) - centre
    q = np.stack([np.cos(a) * p[:, 0] + np.sin(a) * p[:, 2], p[:, 1], -np.sin(a) * p[:, 0] + np.cos(a) * p[:, 2]], axis=1)
    return (q + centre).astype(f32).reshape(-1, 9)


def sequence_vertices(tris, motion, frames):
    """The mesh of each frame: frame 0 as uploaded, each later frame the previous one moved again."""
    out = [vertices_of(tris)]
    centre = out[0].reshape(-1, 3).astype(np.float64).mean(axis=0)
    for _ in range(1, frames):
        out.append(translated(out[-1], (12.0, 0.0, 0.0)) if motion == "translate" else rotated_y(out[-1], 5.0, centre))
    return out


def chains(frames_g, colors, cam, meshes, nlq):
    """Chains A (the existing restatement) and B (the motion form) over rendered frames: frames_g[f]
    the G-buffer of frame f, meshes[f] its TRI_DTYPE records.  Returns the two lists of states."""
    a, b, sa, sb = [], [], None, None
    for f, g in enumerate(frames_g):
        first = f == 0
        sa = tr.accumulate(colors[f], g, cam, *((None,) * 3 if first else (sa, frames_g[f - 1], cam)))
        if first:
            sb = accumulate_motion(colors[f], g, cam)
        else:
            m = reproject(g, nlq, meshes[f], meshes[f - 1])
            sb = accumulate_motion(colors[f], g, cam, m["pos_prev"], m["norm_prev"], sb, frames_g[f - 1], cam)
        a.append(sa)
        b.append(sb)
    return a, b


def shares(state_a, state_b, is_tri, frames):
    """The two figures at the last frame, as shares of the triangle pixels: chain A's len >= 3, and chain
    B's full history, len == frames.  A history length is not an integer: it is the bilinear mean of the
    taps' lengths plus one, lsum / wsum + 1, so a pixel whose every tap has the full history comes out
    at 5.9999995 as often as at 6, and one tap of four with a shorter history gives 5.9.  The full
    history is therefore counted as the length that rounds to `frames` (np.rint), the reading under
    which the figures this work was proposed with are reproduced to their third digit (B: 0.730 and
    0.779; exact float equality gives 0.595 and 0.545 on the same states)."""
    n = max(int(is_tri.sum()), 1)
    return float((state_a["len"][is_tri] >= 3).sum()) / n, float((np.rint(state_b["len"][is_tri]) == frames).sum()) / n
