"""Synthetic two-frame sequences and camera pairs for the temporal accumulation's tests (test
infrastructure only), shared by tests/test_temporal_restatement.py and tests/test_gpu_temporal.py.
Built like synthetic() of tests/test_gpu_denoise.py, so that every branch of the tap test is taken
on both sides.
"""
import numpy as np

import temporal_restatement as tr

f32, U32 = np.float32, np.uint32
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], f32)
SIZES = [(1, 1), (5, 3), (17, 1), (1, 17), (67, 35), (130, 9)]  # none a multiple of the 64 x 4 block
BAD = (np.nan, np.inf, -np.inf, 2.0 ** 101, -(2.0 ** 101))


def camera(w, h, origin=(278.0, 278.0, -800.0), target=(278.0, 278.0, 0.0)):
    """A CAMERA_DTYPE record without the library (the layout of include/wgt_api.h): the reference's
    camera by default, spp and seed 0 (the accumulation ignores them)."""
    from webgputracer_amd._lib import CAMERA_DTYPE

    cam = np.zeros(1, CAMERA_DTYPE)
    cam["origin"], cam["target"] = origin, target
    cam["aspect"], cam["fovy"] = f32(w / h), f32(40.0)
    return cam


def camera_pairs(w, h):
    """{name: (cam, cam_prev)}: identical; translated by fractions of a pixel and by several pixels
    (a pixel is some 580 / h scene units wide at the synthetic positions' depth); rotated; and a
    previous camera that stands among the positions and so has part of them behind it."""
    px = 582.0 / h
    o, t = np.array([278.0, 278.0, -800.0]), np.array([278.0, 278.0, 0.0])

    def moved(d_origin, d_target=None):
        d_origin = np.asarray(d_origin, float)
        return camera(w, h, o + d_origin, t + (d_origin if d_target is None else np.asarray(d_target, float)))

    return {"identical": (camera(w, h), camera(w, h)),
            "subpixel": (camera(w, h), moved([0.3 * px, -0.45 * px, 0.0])),
            "pixels": (moved([1.0, 0.0, 0.0]), moved([3.6 * px, -2.3 * px, 5.0])),
            "rotated": (camera(w, h), moved([0.0, 0.0, 0.0], [1.7 * px, 0.8 * px, 0.0])),
            "behind": (camera(w, h), camera(w, h, (20.0, 20.0, 1.5), (21.0, 20.5, 801.5)))}


def _guides(rng, w, h):
    n = w * h
    axis = AXES[rng.choice(6, n, p=[0.55, 0.05, 0.2, 0.05, 0.1, 0.05])]
    scale = rng.choice(np.array([1.0, 1.0, 1.0, 0.99, 0.97, 0.93, 0.918], f32), n)
    norm = axis * scale[:, None] + np.where(rng.random((n, 1)) < 0.3, rng.normal(0, 0.05, (n, 3)), 0)
    norm = (norm / np.maximum(1.0, np.linalg.norm(norm, axis=1, keepdims=True))).astype(f32)
    lattice = np.array([0, 0.25, 0.5, 1, 2, 3, 8, 40], f32)
    pos = (rng.choice(lattice, (n, 3), p=[0.5, 0.12, 0.12, 0.1, 0.05, 0.05, 0.03, 0.03]) +
           np.where(rng.random((n, 1)) < 0.5, rng.normal(0, 0.3, (n, 3)), 0)).astype(f32)
    prim = rng.integers(0, 4, n).astype(U32)
    flags = (rng.integers(0, 2, n) * 2).astype(np.uint8)  # WGT_HIT_FRONT_FACE on and off
    return {"prim": prim, "flags": flags, "pos": pos, "norm": norm}


def _colour(rng, n):
    color = np.concatenate([rng.gamma(0.5, 1.0, (n, 3)), rng.random((n, 1))], axis=1).astype(f32)
    rgb = color[:, :3]  # a view
    rgb[rng.random((n, 3)) < 0.05] = 0.0
    rgb[rng.random((n, 3)) < 0.05] = -0.0
    rgb[rng.random((n, 3)) < 0.03] *= -1.0
    return color


def _sprinkle(rng, g, color):
    """Misses, emissive pixels, and NaN, inf and 2^101 in every float field; -0 positions and normals."""
    n = len(g["prim"])
    g["prim"][rng.random(n) < 0.04] = tr.MISS
    g["flags"][rng.random(n) < 0.04] |= 1
    for field in (g["pos"], g["norm"], color[:, :3]):
        for bad in BAD:
            k = rng.random(n) < 0.008
            field[k, rng.integers(0, 3, k.sum())] = bad
    for field in (g["pos"], g["norm"]):
        k = rng.random(n) < 0.02
        field[k, rng.integers(0, 3, k.sum())] = -0.0
    color[rng.random(n) < 0.01, 3] = np.nan  # alpha is carried, never looked at


def _shaped(g, color, w, h):
    return color.reshape(h, w, 4), {k: v.reshape((h, w) + v.shape[1:]) for k, v in g.items()}


def synthetic(w, h, seed):
    """(color, g, prev, g_prev): the current frame and a previous state with its guides.  The previous
    guides are the current ones with a part of the normals, positions and primitives drawn again, so
    that taps pass and fail each test; prev.len holds 0, 0.5, 1, 7 and more, NaN, inf and -0; the
    previous moments hold 2^101 and -0 (no NaN or inf: moments are not part of the tap test, and a
    NaN's payload is the hardware's)."""
    rng = np.random.default_rng(seed)
    n = w * h
    g = _guides(rng, w, h)
    other = _guides(rng, w, h)
    gp = {k: v.copy() for k, v in g.items()}
    for key, frac in (("norm", 0.3), ("pos", 0.3), ("prim", 0.2), ("flags", 0.3)):
        k = rng.random(n) < frac
        gp[key][k] = other[key][k]
    color, pcolor = _colour(rng, n), _colour(rng, n)
    _sprinkle(rng, g, color)
    _sprinkle(rng, gp, pcolor)
    plen = rng.choice(np.array([0.0, 0.5, 1.0, 1.0, 2.0, 3.5, 7.0, 7.0, 31.0, 65536.0], f32), n)
    for bad in (np.nan, np.inf, -np.inf, -0.0, -3.0):
        plen[rng.random(n) < 0.01] = bad
    lum = tr.luminance(np.where(np.abs(pcolor[:, :3]) < 100.0, np.abs(pcolor[:, :3]), f32(1)).astype(f32))
    pmom = np.stack([lum, lum * lum + rng.random(n).astype(f32)]).astype(f32)
    for bad in (2.0 ** 101, -(2.0 ** 101), -0.0):
        pmom[rng.random((2, n)) < 0.01] = bad
    color, g = _shaped(g, color, w, h)
    pcolor, gp = _shaped(gp, pcolor, w, h)
    prev = {"f32": pcolor, "len": plen.reshape(h, w), "moments": pmom.reshape(2, h, w)}
    return color, g, prev, gp


def valid_outputs_finite(state, color, g):
    """No accumulated pixel of a restated state is NaN or inf (its rgb, len and moments)."""
    v = tr.valid_mask(color, g)
    fine = np.isfinite(state["f32"][..., :3][v]).all() and np.isfinite(state["len"][v]).all()
    if state["moments"] is not None:
        fine = fine and np.isfinite(state["moments"][:, v]).all()
    return bool(fine)
