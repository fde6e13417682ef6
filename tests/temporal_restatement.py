"""The temporal accumulation's specification restated in numpy float32 (test infrastructure only):
wgt_temporal_accumulate, operation by operation.  Every operation is an IEEE
binary32 operation, none is fused, denormals are kept; the GPU result equals accumulate() bit for bit.

`g` is a dict of (H, W) prim (uint32) and flags (uint8) and (H, W, 3) float32 pos and norm, the shape
Context.render_gbuffer returns; a state is a dict of "f32" (H, W, 4), "len" (H, W) and "moments"
((2, H, W) or None), the shape Context.temporal_accumulate returns; a camera is a CAMERA_DTYPE record
array of length 1 (camera_param).
"""
import numpy as np

import numpy_restatement as nr
from denoise_restatement import EMISSIVE, MISS, OK_LIMIT, dot3, ok, unorm8  # noqa: F401 (unorm8: for the tests)

f32 = np.float32
MIN_WEIGHT = f32(2.0 ** -6)
LUMA = (f32(0.2126), f32(0.7152), f32(0.0722))


def camera_constants(cam, W, H):
    """plan_temporal's constants of one camera: make_frame's terms (setup_camera_ray,
    path_tracer.wgsl:239-257, evaluated as written there) and what the projection derives from them.
    A degenerate camera gives NaN."""
    cam = cam[0]
    with np.errstate(all="ignore"):
        origin = tuple(f32(v) for v in cam["origin"])
        end = tuple(f32(v) for v in cam["target"])
        theta = f32(cam["fovy"]) * f32(0.017453292519943295)
        focal = nr.length(nr.sub(origin, end))
        h = f32(nr.wsin(theta * f32(0.5))) / f32(nr.wcos(theta * f32(0.5)))
        vh = f32(2.0) * h * focal
        vw = vh * f32(cam["aspect"])
        w = nr.normalize(nr.sub(origin, end))
        u = nr.normalize(nr.cross((f32(0), f32(1), f32(0)), w))
        v = nr.cross(w, u)
        vu = nr.scl(vw, u)
        vv = nr.scl(vh, nr.neg(v))
        du = nr.dvs(vu, f32(W))
        dv = nr.dvs(vv, f32(H))
        vul = nr.sub(nr.sub(nr.sub(origin, nr.scl(focal, w)), nr.scl(f32(0.5), vu)), nr.scl(f32(0.5), vv))
        po = nr.add(vul, nr.scl(f32(0.5), nr.add(du, dv)))
        c = nr.sub(po, origin)
        nrm = nr.cross(du, dv)
        out = {"o": origin, "c": c, "nrm": nrm, "k": nr.dot(c, nrm), "iu": nr.dvs(du, nr.dot(du, du)),
               "iv": nr.dvs(dv, nr.dot(dv, dv)), "du": du, "dv": dv}
    for key in ("o", "c", "nrm", "iu", "iv", "du", "dv"):
        out[key] = np.array([f32(x) for x in out[key]], f32)
    out["k"] = f32(out["k"])
    return out


def project(C, p):
    """project(camera, p) of (..., 3) points: (x, y, front), pixel centres at the integers."""
    with np.errstate(all="ignore"):
        q = (p - C["o"]).astype(f32)
        z = dot3(q, C["nrm"])
        s = (C["k"] / z).astype(f32)
        front = (s > 0) & (s <= OK_LIMIT)
        r = (s[..., None] * q - C["c"]).astype(f32)
        return dot3(r, C["iu"]).astype(f32), dot3(r, C["iv"]).astype(f32), front


def valid_mask(color, g):
    """The pixels that accumulate and serve as taps: a hit that is not emissive, with finite position,
    normal and colour."""
    with np.errstate(all="ignore"):
        return ((g["prim"] != MISS) & ((g["flags"] & EMISSIVE) == 0) & ok(g["pos"]) & ok(g["norm"]) &
                ok(color[..., :3]))


def luminance(rgb):
    return ((LUMA[0] * rgb[..., 0] + LUMA[1] * rgb[..., 1]) + LUMA[2] * rgb[..., 2]).astype(f32)


def accumulate(color, g, cam, prev=None, g_prev=None, cam_prev=None, max_history=32, normal_min=0.9, plane_tol=1.0,
               match_prim=False, moments=True):
    """One call: the new state.  prev, g_prev and cam_prev None: the first frame."""
    assert (prev is None) == (g_prev is None) == (cam_prev is None)
    with np.errstate(all="ignore"):
        H, W, _ = color.shape
        cur = color[..., :3].astype(f32)
        valid = valid_mask(color, g)
        lum = luminance(cur)
        wsum = np.zeros((H, W), f32)
        lsum = np.zeros((H, W), f32)
        m1sum = np.zeros((H, W), f32)
        m2sum = np.zeros((H, W), f32)
        csum = np.zeros((H, W, 3), f32)
        if prev is not None:
            pos, n = g["pos"].astype(f32), g["norm"].astype(f32)
            xc, yc, fc = project(camera_constants(cam, W, H), pos)
            xp, yp, fp = project(camera_constants(cam_prev, W, H), pos)
            hx = (np.arange(W, dtype=f32)[None, :] + (xp - xc)).astype(f32)
            hy = (np.arange(H, dtype=f32)[:, None] + (yp - yc)).astype(f32)
            has = valid & fc & fp & (hx > f32(-1)) & (hx < f32(W)) & (hy > f32(-1)) & (hy < f32(H))
            hx, hy = np.where(has, hx, f32(0)), np.where(has, hy, f32(0))
            x0f, y0f = np.floor(hx), np.floor(hy)
            fx, fy = (hx - x0f).astype(f32), (hy - y0f).astype(f32)
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            vprev = valid_mask(prev["f32"], g_prev)
            for j in (0, 1):
                for i in (0, 1):
                    b = ((fx if i else f32(1) - fx) * (fy if j else f32(1) - fy)).astype(f32)
                    tx, ty = x0 + i, y0 + j
                    inb = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                    tx, ty = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                    lt = prev["len"][ty, tx].astype(f32)
                    use = (has & (b > 0) & inb & (lt >= f32(1)) & vprev[ty, tx] &
                           (dot3(n, g_prev["norm"][ty, tx].astype(f32)) >= f32(normal_min)) &
                           (np.abs(dot3(n, (g_prev["pos"][ty, tx] - pos).astype(f32))) <= f32(plane_tol)))
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
        hist_ok = valid & (wsum >= MIN_WEIGHT)
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
