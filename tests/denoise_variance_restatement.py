"""The variance-guided denoiser's specification restated in numpy float32 (test infrastructure only):
wgt_denoise_variance, operation by operation.  Every operation is an IEEE binary32
operation, none is fused, denormals are kept, the square root is correctly rounded; the GPU result
equals denoise_variance() bit for bit.

`state` is the dict Context.temporal_accumulate returns ("f32" (H, W, 4), "len" (H, W), "moments"
(2, H, W)); `g` is a dict of (H, W) prim (uint32) and flags (uint8) and (H, W, 3) float32 pos, norm
and col, the shape Context.render_gbuffer returns.

Nothing overflows to NaN for guides whose normals are within unit length and fields within 2^100:
every weight is then in 0..1, the divisors are >= the centre's weight (1, 1/4 or 9/64), the sums of
up to 49 terms within 2^101 stay finite, m1 * m1 may reach +inf but only under max0(m2 - inf) = 0,
s * s may reach +inf but only as a divisor of a finite value, a variance is never negative and a pass
never raises the largest one (its weights w^2 / (sum w)^2 sum to at most 1), so the square root's
argument is finite and >= 0 and kl is in 0..1e6, and a luminance difference of the iterate (within
2^110) is finite: |dl| * kl is never inf * 0.
"""
import numpy as np

from denoise_restatement import ALBEDO_MIN, K, OK_LIMIT, dot3, falloff, max0, valid_mask as denoise_valid_mask
from temporal_restatement import luminance

f32 = np.float32
G3 = np.array([1 / 4, 1 / 2, 1 / 4], f32)  # the variance prefilter's 3 taps
LUM_EPS = f32(1e-6)


def valid_mask(state, g):
    """The pixels the filter averages: wgt_denoise's, with a history and moments within 2^100."""
    with np.errstate(all="ignore"):
        m1, m2 = state["moments"][0], state["moments"][1]
        return (denoise_valid_mask(state["f32"], g) & (state["len"] >= f32(1)) & (np.abs(m1) <= OK_LIMIT) &
                (np.abs(m2) <= OK_LIMIT))


def _shifted(H, W, dy, dx):
    """The tap at (dy, dx) of every pixel: whether it lies in the image, and its clamped coordinates."""
    ys = np.arange(H)[:, None] + dy
    xs = np.arange(W)[None, :] + dx
    inb = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    yc, xc = np.broadcast_arrays(np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1))
    return inb, yc, xc


def _normal_weight(n, nq, npow):
    wn = max0(dot3(n, nq))
    for _ in range(npow):
        wn = wn * wn
    return wn


def _plane_weight(n, p, pq, kz):
    d = dot3(n, pq - p)
    return falloff((d * d) * kz)


def spatial_variance(state, g, valid, kz0, npow, min_history):
    """v_raw of a short history: from the 7 x 7 window's weighted moments (computed for every pixel)."""
    H, W = valid.shape
    n, p = g["norm"].astype(f32), g["pos"].astype(f32)
    m1, m2 = state["moments"][0].astype(f32), state["moments"][1].astype(f32)
    s1, s2, sw = np.zeros((H, W), f32), np.zeros((H, W), f32), np.zeros((H, W), f32)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            inb, yc, xc = _shifted(H, W, dy, dx)
            if dy == 0 and dx == 0:
                w, use = np.ones((H, W), f32), np.ones((H, W), bool)
            else:
                use = inb & valid[yc, xc]
                w = _normal_weight(n, n[yc, xc], npow) * _plane_weight(n, p, p[yc, xc], kz0)
                w = np.where(use, w, f32(0)).astype(f32)  # added as zero, not skipped
            s1 = s1 + w * np.where(use, m1[yc, xc], f32(0))
            s2 = s2 + w * np.where(use, m2[yc, xc], f32(0))
            sw = sw + w
    M1, M2 = (s1 / sw).astype(f32), (s2 / sw).astype(f32)
    return (max0(M2 - M1 * M1) * (f32(min_history) / state["len"].astype(f32))).astype(f32)


def denoise_variance(state, g, iters=5, sigma_p=1.0, npow=7, sigma_lum=4.0, min_history=4, demod=True):
    """((H, W, 4) float32, (H, W) float32): the filtered image and the filtered variance of the
    demodulated luminance.  Alpha and every pixel outside valid_mask pass through, with variance 0."""
    with np.errstate(all="ignore"):
        color = state["f32"]
        H, W, _ = color.shape
        c = color[..., :3].astype(f32)
        valid = valid_mask(state, g)
        a = np.where(g["col"] > ALBEDO_MIN, g["col"], ALBEDO_MIN).astype(f32) if demod else np.ones_like(c)
        cur = (c / a).astype(f32)
        n = g["norm"].astype(f32)
        p = g["pos"].astype(f32)
        kz0 = f32(1) / (f32(sigma_p) * f32(sigma_p))
        m1, m2 = state["moments"][0].astype(f32), state["moments"][1].astype(f32)
        s = luminance(a)
        longh = state["len"] >= f32(min_history)
        v_raw = np.where(longh, max0(m2 - m1 * m1), spatial_variance(state, g, valid, kz0, npow, min_history))
        v = np.where(valid, (v_raw / (s * s)).astype(f32), f32(0)).astype(f32)
        for i in range(iters):
            st = 1 << i
            kz = kz0 * f32(4.0 ** -i)
            # the luminance tolerance: a 3 x 3 Gaussian of the variance over in-image valid pixels
            gs, gw = np.zeros((H, W), f32), np.zeros((H, W), f32)
            for dy in range(-1, 2):
                for dx in range(-1, 2):
                    inb, yc, xc = _shifted(H, W, dy, dx)
                    use = inb & valid[yc, xc]
                    w = G3[dy + 1] * G3[dx + 1]
                    gs = gs + np.where(use, w * v[yc, xc], f32(0))
                    gw = gw + np.where(use, w, f32(0))
            kl = f32(1) / (f32(sigma_lum) * np.sqrt((gs / gw).astype(f32)) + LUM_EPS)
            lum = luminance(cur)
            ssum = np.zeros_like(cur)
            wsum = np.zeros((H, W), f32)
            vsum = np.zeros((H, W), f32)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    h = K[dy + 2] * K[dx + 2]
                    inb, yc, xc = _shifted(H, W, dy * st, dx * st)
                    cq, vq = cur[yc, xc], v[yc, xc]
                    if dy == 0 and dx == 0:
                        w = np.full((H, W), h, f32)
                    else:
                        wl = falloff(np.abs(lum[yc, xc] - lum) * kl)
                        w = ((h * _normal_weight(n, n[yc, xc], npow)) * _plane_weight(n, p, p[yc, xc], kz)) * wl
                        use = inb & valid[yc, xc]
                        w = np.where(use, w, f32(0)).astype(f32)  # added as zero, not skipped
                        cq = np.where(use[..., None], cq, f32(0)).astype(f32)
                        vq = np.where(use, vq, f32(0)).astype(f32)
                    ssum = ssum + w[..., None] * cq
                    wsum = wsum + w
                    vsum = vsum + (w * w) * vq
            cur = np.where(valid[..., None], (ssum / wsum[..., None]).astype(f32), cur)
            v = np.where(valid, (vsum / (wsum * wsum)).astype(f32), v)
        out = color.astype(f32).copy()
        out[..., :3] = np.where(valid[..., None], cur * a, c)
        return out, np.where(valid, v, f32(0)).astype(f32)
