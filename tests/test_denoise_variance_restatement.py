"""The variance-guided denoiser's specification on the CPU (tests/denoise_variance_restatement.py,
DESIGN.md §4.9, which the GPU result equals bit for bit in tests/test_gpu_denoise_variance.py): that it
beats the plain filter on accumulated Cornell frames of the oracle, which is its whole point, and what
it must and must not do at luminance edges, lights and broken pixels.
"""
import numpy as np
import pytest

import denoise_restatement as dr
import denoise_variance_restatement as dv
import hit_records as hr
import temporal_restatement as tr
from test_denoise_restatement import plane, rgba
from test_gpu_gbuffer import camera_rays

f32, U32 = np.float32, np.uint32
K, N = 8, 64


def _bits(a):
    return np.ascontiguousarray(a, f32).view(U32)


def state_of(color, length=8.0, m1=0.0, m2=0.0):
    """A state of `color` with constant len and moments (the filter asks no consistency of them)."""
    h, w = color.shape[:2]
    return {"f32": color.astype(f32), "len": np.full((h, w), length, f32),
            "moments": np.stack([np.full((h, w), m1, f32), np.full((h, w), m2, f32)])}


@pytest.fixture(scope="module")
def cornell_states(oracle):
    """The states after 1..K frames of the 64 x 64 Cornell box at 4 spp (seeds 0..K-1, one camera,
    chained through tr.accumulate), the guides of seed 0's frame with col, and a 1024-spp frame."""
    L, Q, S = oracle.cornell_scene()
    scene = oracle.OracleScene(L, Q, S)
    cams = [oracle.camera_param(1.0, 4, s) for s in range(K)]
    colors = [scene.render(c, N, N, want=("f32",))["f32"] for c in cams]
    ref = scene.render(oracle.camera_param(1.0, 1024, 77), N, N, want=("f32",))["f32"]
    o, d = camera_rays(cams[0], N, N)
    rec = hr.quad_sphere_records(o.reshape(-1, 3), d.reshape(-1, 3), L, Q, S)
    g = {k: rec[k].reshape((N, N) + rec[k].shape[1:]) for k in ("prim", "flags", "pos", "norm", "col")}
    states, prev = [], None
    for c in colors:
        prev = tr.accumulate(c, g, cams[0], prev, None if prev is None else g, None if prev is None else cams[0])
        states.append(prev)
    return states, g, ref


@pytest.mark.parametrize("frames", [K, 1])
def test_beats_the_plain_filter_on_accumulated_cornell_frames(cornell_states, frames):
    """Clamped MSE against 1024 spp of the state after `frames` frames: the variance-guided result is
    below dr.denoise of the same accumulated frame.  Measured: ratio 0.471 after 8 frames (0.00589
    against 0.01251) and 0.641 on the first frame alone (0.00821 against 0.01280), where every pixel
    takes the spatial estimate."""
    states, g, ref = cornell_states
    st = states[frames - 1]
    assert (st["len"][dv.valid_mask(st, g)] == frames).all()

    def mse(img):
        return float(np.mean((np.minimum(img[..., :3], 1) - np.minimum(ref[..., :3], 1)) ** 2, dtype=np.float64))

    plain = mse(dr.denoise(st["f32"], g))
    out, var = dv.denoise_variance(st, g)
    guided = mse(out)
    print(f"{frames} frames: clamped MSE accumulated {mse(st['f32']):.5f}, plain {plain:.5f}, "
          f"variance-guided {guided:.5f}, ratio {guided / plain:.3f}")
    assert np.isfinite(out).all() and np.isfinite(var).all() and (var >= 0).all()
    assert guided / plain < 1


def _varied_plane(h, w, seed):
    """One plane with varied albedo and slightly varied normals and depths: the guide weights differ
    from tap to tap."""
    rng = np.random.default_rng(seed)
    g = plane(h, w)
    g["col"] = (0.2 + 0.7 * rng.random((h, w, 3))).astype(f32)
    n = np.array([0, 0, -1], f32) + 0.2 * rng.standard_normal((h, w, 3)).astype(f32)
    g["norm"] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(f32)
    g["pos"][..., 2] = 0.3 * rng.standard_normal((h, w)).astype(f32)
    return g, rng


def test_zero_variance_and_constant_luminance_is_the_plain_filter():
    """Every falloff(0) is 1: with zero variance and an iterate of constant luminance (colour = albedo,
    so rgb / a is exactly 1 and stays 1) the result equals dr.denoise bit for bit."""
    h, w = 23, 37
    g, _ = _varied_plane(h, w, 5)
    color = rgba(g["col"])
    for st in (state_of(color), state_of(color, m1=0.5, m2=0.25), state_of(color, length=1.0)):
        out, var = dv.denoise_variance(st, g)
        assert np.array_equal(_bits(out), _bits(dr.denoise(color, g)))
        assert (var == 0).all()


def test_a_huge_variance_opens_the_luminance_weight_entirely():
    """A variance so large that every |dl| * kl rounds away under 1: the plain filter bit for bit, on
    random colours, with and without demodulation."""
    h, w = 23, 37
    g, rng = _varied_plane(h, w, 6)
    color = rgba(rng.random((h, w, 3)).astype(f32))
    st = state_of(color, m2=2.0 ** 90)
    for demod in (True, False):
        out, var = dv.denoise_variance(st, g, demod=demod)
        assert np.array_equal(_bits(out), _bits(dr.denoise(color, g, demod=demod)))
        assert (var > 2.0 ** 60).all()


def test_a_luminance_edge_on_one_plane_survives():
    """A step in luminance on one plane, zero variance: five passes leave it where dr.denoise blurs it."""
    h, w = 16, 40
    g = plane(h, w)
    color = rgba(np.full((h, w, 3), 0.25, f32))
    color[:, w // 2:, :3] = 0.75
    out, var = dv.denoise_variance(state_of(color), g)
    assert np.abs(out - color).max() < 1e-6 and (var == 0).all()
    plain = dr.denoise(color, g)
    assert np.abs(plain - color)[:, w // 2 - 1:w // 2 + 1, :3].min() > 0.05
    # ... and noise with an honest variance on either side of it is still filtered
    rng = np.random.default_rng(7)
    noise = (0.05 * rng.standard_normal((8, h, w))).astype(f32)
    frames = color[None, ..., :1] + noise[..., None]
    mean = frames.mean(axis=0)
    lum = tr.luminance(np.repeat(frames, 3, axis=-1))
    st = {"f32": rgba(np.repeat(mean, 3, axis=-1)), "len": np.full((h, w), 8, f32),
          "moments": np.stack([lum.mean(axis=0), (lum * lum).mean(axis=0)]).astype(f32)}
    out, var = dv.denoise_variance(st, g)
    err_in = np.abs(st["f32"] - color)[..., :3].mean()
    err_out = np.abs(out - color)[..., :3].mean()
    print(f"edge with noise: mean error {err_in:.5f} -> {err_out:.5f}")
    assert err_out < 0.5 * err_in
    assert np.abs(out - color)[:, w // 2 - 1:w // 2 + 1, :3].max() < 0.05  # the step is 0.5


def test_pass_through_rules():
    """Lights, misses, NaN, len 0 and non-finite moments: bit for bit, variance 0, never a tap."""
    h, w = 14, 19
    g, rng = _varied_plane(h, w, 8)
    color = rgba(rng.random((h, w, 3)).astype(f32))
    color[..., 3] = rng.random((h, w)).astype(f32)
    st = state_of(color, m1=0.5, m2=0.26)
    st["len"] = rng.choice(np.array([1, 2, 3, 4, 9], f32), (h, w))
    broken = {(2, 3): "light", (5, 7): "miss", (8, 2): "nan colour", (3, 12): "len 0", (9, 9): "len nan",
              (11, 15): "m1 nan", (6, 16): "m2 inf", (12, 4): "m1 2^101", (1, 10): "inf normal", (10, 1): "inf albedo"}
    g["flags"][2, 3] = 1
    g["prim"][5, 7] = dr.MISS
    st["f32"][8, 2, 1] = np.nan
    st["len"][3, 12] = 0
    st["len"][9, 9] = np.nan
    st["moments"][0, 11, 15] = np.nan
    st["moments"][1, 6, 16] = np.inf
    st["moments"][0, 12, 4] = 2.0 ** 101
    g["norm"][1, 10, 2] = np.inf
    g["col"][10, 1, 0] = np.inf
    mask = np.zeros((h, w), bool)
    for y, x in broken:
        mask[y, x] = True
    assert np.array_equal(~dv.valid_mask(st, g), mask)
    out, var = dv.denoise_variance(st, g)
    assert np.array_equal(_bits(out)[mask], _bits(st["f32"])[mask])
    assert (var[mask] == 0).all() and np.isfinite(out[~mask]).all() and np.isfinite(var[~mask]).all()
    assert np.array_equal(_bits(out[..., 3]), _bits(st["f32"][..., 3]))  # alpha is the input's everywhere
    assert not np.array_equal(_bits(out)[~mask], _bits(st["f32"])[~mask])
    # never a tap: other colours and moments in the broken pixels change nothing elsewhere
    st2 = {k: v.copy() for k, v in st.items()}
    st2["f32"][mask, :3] = 1e6
    st2["f32"][8, 2, 1] = np.nan
    st2["moments"][:, mask & (st["len"] >= 1)] = np.nan
    out2, var2 = dv.denoise_variance(st2, g)
    assert np.array_equal(_bits(out2)[~mask], _bits(out)[~mask])
    assert np.array_equal(_bits(var2)[~mask], _bits(var)[~mask])


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (1, 17), (17, 1)])
@pytest.mark.parametrize("length", [1.0, 8.0])
def test_small_sizes_are_finite(size, length):
    w, h = size
    rng = np.random.default_rng(4)
    color = rgba(rng.random((h, w, 3)).astype(f32))
    st = state_of(color, length=length, m1=0.5, m2=0.3)
    out, var = dv.denoise_variance(st, plane(h, w), iters=8)
    assert out.shape == (h, w, 4) and var.shape == (h, w) and np.isfinite(out).all() and np.isfinite(var).all()
    if size == (1, 1):
        assert np.array_equal(_bits(out), _bits(color))  # (h c / a) / h * a at a = 1


def test_extreme_fields_give_no_nan():
    """Fields at 2^100 and moments at +-2^100 with unit normals: no NaN in a valid pixel (the module
    docstring's argument), for both variance paths."""
    h, w = 9, 11
    g, rng = _varied_plane(h, w, 9)
    big = f32(2.0 ** 100)
    color = rgba((big * rng.choice(np.array([-1, 1e-30, 1], f32), (h, w, 3))).astype(f32))
    g["col"] = (big * rng.choice(np.array([-1, 0, 1], f32), (h, w, 3))).astype(f32)
    g["pos"] = (big * rng.choice(np.array([-1, 0, 1], f32), (h, w, 3))).astype(f32)
    for length in (1.0, 64.0):
        for m1, m2 in ((big, big), (-big, -big), (0, big), (1e-20, 1e-45)):
            st = state_of(color, length=length, m1=m1, m2=m2)
            assert dv.valid_mask(st, g).all()
            for sigma_lum in (1e-30, 4.0, 3e38):
                out, var = dv.denoise_variance(st, g, iters=8, sigma_lum=sigma_lum, min_history=4)
                assert not np.isnan(out).any() and not np.isnan(var).any() and (var >= 0).all()
