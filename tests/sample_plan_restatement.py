"""The sample-map planner's arithmetic in numpy float32 (test infrastructure only): the specification
of wgt_sample_plan, DESIGN.md §4.11, which the GPU result equals bit for bit (tests/test_gpu_sample_plan.py).
Every float operation is one IEEE binary32 operation on float32 arrays, none fused, the square root
correctly rounded; everything across pixels is an integer.

A state is the dict tests/temporal_restatement.py's accumulate returns: "len" (H, W) float32 and
"moments" (2, H, W) float32 (the running means of luminance and of its square); "f32" is not read.
"""
import numpy as np

f32 = np.float32
DEFAULTS = dict(side_min=1, side_max=8, gain=12.0, lum_floor=1.0, min_history=4, dilate=2, budget_spp=0.0)
LIMIT = f32(2.0 ** 100)


def wanted(state, side_min, side_max, gain, lum_floor, min_history):
    """Steps 1-4: the side each pixel wants on its own, (H, W) int64."""
    length = np.asarray(state["len"], f32)
    m1, m2 = np.asarray(state["moments"][0], f32), np.asarray(state["moments"][1], f32)
    smin, smax = f32(side_min), f32(side_max)
    with np.errstate(all="ignore"):
        measured = (length >= f32(min_history)) & (np.abs(m1) <= LIMIT) & (np.abs(m2) <= LIMIT) & (length >= f32(1))
        d = (m2 - (m1 * m1).astype(f32)).astype(f32)
        var = np.where(d > f32(0), d, f32(0)).astype(f32)  # max0: NaN and -0 give +0
        rel = (np.sqrt(var).astype(f32) / (np.abs(m1) + f32(lum_floor)).astype(f32)).astype(f32)
        w = np.ceil((rel * f32(gain)).astype(f32)).astype(f32)
        w = np.where(w < smin, smin, w)  # compared in float: +inf saturates to side_max
        w = np.where(w > smax, smax, w)
        # a pixel that is not measured has NaN or inf here at most: never converted
        w = np.where(measured, w, np.where(length == f32(0), smin, smax)).astype(f32)
    return w.astype(np.int64)


def dilated(want, radius):
    """Step 5: the maximum over the in-image pixels within `radius` in x and y."""
    H, W = want.shape
    out = want.copy()
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
            xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            out[yd, xd] = np.maximum(out[yd, xd], want[ys, xs])
    return out


def budget_of(budget_spp, W, H):
    """B = floor(budget_spp * W * H): the float parameter's value times the pixel count, in double."""
    return int(np.floor(np.float64(f32(budget_spp)) * np.float64(W) * np.float64(H)))


def capped_total(d, c):
    """The sum over the pixels of min(dilated, c)^2, an exact integer."""
    m = np.minimum(d, c).astype(np.int64)
    return int((m * m).sum())


def cap(d, side_min, side_max, B):
    """Step 6: the largest c in [side_min, side_max] whose capped total is at most B; side_min when none is."""
    for c in range(side_max, side_min, -1):
        if capped_total(d, c) <= B:
            return c
    return side_min


def plan(state, **params):
    """{"map": (H, W) uint8, "total": int, "cap": int, "budget": int or None}."""
    p = dict(DEFAULTS, **params)
    want = wanted(state, p["side_min"], p["side_max"], p["gain"], p["lum_floor"], p["min_history"])
    d = dilated(want, p["dilate"])
    H, W = d.shape
    c, B = p["side_max"], None
    if f32(p["budget_spp"]) > f32(0):
        B = budget_of(p["budget_spp"], W, H)
        c = cap(d, p["side_min"], p["side_max"], B)
    m = np.minimum(d, c)
    return {"map": m.astype(np.uint8), "total": capped_total(m, 255), "cap": c, "budget": B}
