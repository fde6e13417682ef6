"""The denoiser's specification on the CPU (tests/denoise_restatement.py, which the GPU result
equals bit for bit): what the filter must and must not do at edges, lights and broken pixels, and
that it denoises a Cornell frame of the oracle.
"""
import numpy as np
import pytest

import denoise_restatement as dr

f32, U32 = np.float32, np.uint32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(U32)


def plane(h, w, normal=(0, 0, -1), albedo=1.0):
    """Guides of a w x h image of one plane through the origin, pixel (x, y) at (x, y, 0)."""
    ys, xs = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    return {"prim": np.full((h, w), 3, U32), "flags": np.zeros((h, w), np.uint8),
            "pos": np.stack([xs, ys, np.zeros_like(xs)], axis=-1),
            "norm": np.broadcast_to(np.asarray(normal, f32), (h, w, 3)).copy(),
            "col": np.full((h, w, 3), albedo, f32)}


def rgba(rgb):
    return np.concatenate([rgb, np.ones(rgb.shape[:2] + (1,), f32)], axis=-1).astype(f32)


def test_edge_between_two_half_planes():
    """Two half-planes with normals (0,0,-1) and (1,0,0), colours 0 and 1: nothing crosses the edge."""
    h, w = 9, 40
    g = plane(h, w)
    g["norm"][:, w // 2:] = (1, 0, 0)
    g["pos"][:, w // 2:] = np.stack([np.full((h, w - w // 2), f32(w // 2)),
                                     g["pos"][:, w // 2:, 1], g["pos"][:, w // 2:, 0] - f32(w // 2)], axis=-1)
    color = rgba(np.zeros((h, w, 3), f32))
    color[:, w // 2:, :3] = 1.0
    out = dr.denoise(color, g, iters=8)
    assert np.array_equal(_bits(out), _bits(color))
    noisy = color.copy()
    noisy[:, :w // 2, :3] = np.random.default_rng(1).random((h, w // 2, 3)).astype(f32)
    out = dr.denoise(noisy, g, iters=8)
    assert np.array_equal(_bits(out[:, w // 2:]), _bits(noisy[:, w // 2:]))
    before, after = noisy[:, :w // 2, :3].var(), out[:, :w // 2, :3].var()
    print(f"left half variance {before:.4f} -> {after:.6f}")
    assert after < 0.01 * before


def test_emissive_pixel_neither_blurs_nor_bleeds():
    h, w = 12, 15
    g = plane(h, w)
    base = rgba(np.random.default_rng(2).random((h, w, 3)).astype(f32))
    lit = base.copy()
    lit[5, 7, :3] = 1e6
    g_lit = {k: v.copy() for k, v in g.items()}
    g_lit["flags"][5, 7] = 1
    out, ref = dr.denoise(lit, g_lit), dr.denoise(base, g_lit)
    others = np.ones((h, w), bool)
    others[5, 7] = False
    assert np.array_equal(_bits(out)[others], _bits(ref)[others])
    assert np.array_equal(_bits(out[5, 7]), _bits(lit[5, 7]))
    assert out[others].max() <= 1.0


def test_nan_and_inf_stay_in_their_pixels():
    h, w = 10, 11
    g = plane(h, w)
    color = rgba(np.random.default_rng(3).random((h, w, 3)).astype(f32))
    color[2, 3, 1] = np.nan
    g["pos"][6, 8, 0] = np.inf
    out = dr.denoise(color, g, iters=8)
    assert np.isnan(out).sum() == 1 and np.isnan(out[2, 3, 1])
    assert np.array_equal(_bits(out[6, 8]), _bits(color[6, 8])) and not np.isinf(out).any()


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (1, 17)])
def test_small_sizes_are_finite(size):
    w, h = size
    color = rgba(np.random.default_rng(4).random((h, w, 3)).astype(f32))
    out = dr.denoise(color, plane(h, w), iters=8)
    assert out.shape == (h, w, 4) and np.isfinite(out).all()
    if size == (1, 1):
        assert np.array_equal(_bits(out), _bits(color))  # (h c / a) / h * a at a = 1


def test_unorm8_is_the_renderers_store(oracle, wgt):
    """dr.unorm8 of the oracle's radiance equals the oracle's rgba8."""
    L, Q, S = wgt.cornell_scene()
    osc = oracle.OracleScene(L, Q, S)
    r = osc.render(oracle.camera_param(1.0, 4, 3), 24, 24, want=("f32", "u8"))
    osc.close()
    assert np.array_equal(dr.unorm8(r["f32"]), r["u8"])


def test_the_filter_denoises_a_cornell_frame(oracle, wgt):
    """Cornell 96 x 96 at 4 spp against 1024 spp: the clamped mean squared error falls below half
    (0.409 measured; 0.406 at 1 spp and 0.269 at 16 spp).  Guides: sample 0's camera
    rays restated (test_gpu_gbuffer.camera_rays) through the numpy quad-and-sphere scan."""
    import hit_records as hr
    from test_gpu_gbuffer import camera_rays

    n = 96
    L, Q, S = wgt.cornell_scene()
    osc = oracle.OracleScene(L, Q, S)
    cam = oracle.camera_param(1.0, 4, 3)
    noisy = osc.render(cam, n, n, want=("f32",))["f32"]
    ref = osc.render(oracle.camera_param(1.0, 1024, 77), n, n, want=("f32",))["f32"]
    osc.close()
    o, d = camera_rays(cam, n, n)
    rec = hr.quad_sphere_records(o.reshape(-1, 3), d.reshape(-1, 3), L, Q, S)
    g = {k: rec[k].reshape((n, n, 3) if k in hr.VEC else (n, n)) for k in ("prim", "pos", "norm", "col", "flags")}
    out = dr.denoise(noisy, g)

    def mse(img):
        return float(np.mean((np.minimum(img[..., :3], 1) - np.minimum(ref[..., :3], 1)) ** 2, dtype=np.float64))

    ratio = mse(out) / mse(noisy)
    print(f"clamped MSE noisy {mse(noisy):.4f}, denoised {mse(out):.4f}, ratio {ratio:.3f}")
    assert ratio < 0.5
