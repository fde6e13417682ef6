"""The denoiser's specification restated in numpy float32 (test infrastructure only): the
edge-avoiding a-trous filter of wgt_denoise, operation by operation.  Every
operation is an IEEE binary32 operation, none is fused, denormals are kept; the GPU result equals
denoise() bit for bit.

`g` is a dict of (H, W) prim (uint32) and flags (uint8) and (H, W, 3) float32 pos, norm and col, the
shape Context.render_gbuffer returns.
"""
import numpy as np

f32 = np.float32
K = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], f32)  # the B3 spline's 5 taps
MISS = 0xFFFFFFFF
EMISSIVE = 1            # WGT_HIT_EMISSIVE
OK_LIMIT = f32(2.0 ** 100)
ALBEDO_MIN = f32(2.0 ** -8)


def max0(x):
    """wgt_math.h max0: x > 0 ? x : 0 (a NaN gives 0)."""
    return np.where(x > 0, x, f32(0)).astype(f32)


def falloff(x):
    """(1 - x / 16)^16: e^-x with compact support."""
    t = max0(f32(1) - x * f32(0.0625))
    for _ in range(4):
        t = t * t
    return t


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def ok(a):
    """Every component within 2^100 in magnitude; NaN and inf fail."""
    return np.all(np.abs(a) <= OK_LIMIT, axis=-1)


def valid_mask(color, g):
    """The pixels the filter averages: a hit that is not emissive, with finite guides and colour."""
    with np.errstate(all="ignore"):
        return ((g["prim"] != MISS) & ((g["flags"] & EMISSIVE) == 0) & ok(g["pos"]) & ok(g["norm"]) & ok(g["col"]) &
                ok(color[..., :3]))


def denoise(color, g, iters=5, sigma_p=1.0, npow=7, demod=True):
    """(H, W, 4) float32: the filtered image.  Alpha and every pixel outside valid_mask pass through."""
    with np.errstate(all="ignore"):
        H, W, _ = color.shape
        c = color[..., :3].astype(f32)
        valid = valid_mask(color, g)
        a = np.where(g["col"] > ALBEDO_MIN, g["col"], ALBEDO_MIN).astype(f32) if demod else np.ones_like(c)
        cur = (c / a).astype(f32)
        n = g["norm"].astype(f32)
        p = g["pos"].astype(f32)
        kz0 = f32(1) / (f32(sigma_p) * f32(sigma_p))
        for i in range(iters):
            s = 1 << i
            kz = kz0 * f32(4.0 ** -i)
            ssum = np.zeros_like(cur)
            wsum = np.zeros((H, W), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    h = K[dy + 2] * K[dx + 2]
                    ys = np.arange(H)[:, None] + dy * s
                    xs = np.arange(W)[None, :] + dx * s
                    inb = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
                    yc, xc = np.broadcast_arrays(np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1))
                    cq = cur[yc, xc]
                    if dy == 0 and dx == 0:
                        w = np.full((H, W), h, f32)
                    else:
                        wn = max0(dot3(n, n[yc, xc]))
                        for _ in range(npow):
                            wn = wn * wn
                        d = dot3(n, p[yc, xc] - p)
                        w = (h * wn) * falloff((d * d) * kz)
                        use = inb & valid[yc, xc]
                        w = np.where(use, w, f32(0)).astype(f32)  # added as zero, not skipped
                        cq = np.where(use[..., None], cq, f32(0)).astype(f32)
                    ssum = ssum + w[..., None] * cq
                    wsum = wsum + w
            cur = np.where(valid[..., None], (ssum / wsum[..., None]).astype(f32), cur)
        out = color.astype(f32).copy()
        out[..., :3] = np.where(valid[..., None], cur * a, c)
        return out


def unorm8(rgba):
    """The renderer's rgba8unorm store of an rgba32f image (write_pixel): floor(clamp(x, 0, 1) * 255 +
    0.5) of rgb in float32, a NaN giving 0, and alpha 255."""
    with np.errstate(all="ignore"):
        c = max0(rgba[..., :3].astype(f32))
        c = np.where(c < f32(1), c, f32(1)).astype(f32)
        out = np.full(rgba.shape, 255, np.uint8)
        out[..., :3] = np.floor(c * f32(255) + f32(0.5)).astype(np.uint8)
        return out
