"""Properties of the motion passes' specification itself (tests/motion_restatement.py, DESIGN.md
§4.10), on the CPU: synthetic data and the C oracle's G-buffer of the moving bunny scene.  The GPU
results are compared with the same restatement bit for bit in tests/test_gpu_motion.py."""
import numpy as np
import pytest

import hit_records as hr
import motion_restatement as mr
import temporal_cases as tc
import temporal_restatement as tr
from test_gpu_gbuffer import camera_rays

f32, U32 = np.float32, np.uint32
W, H, FRAMES = 64, 48, 6
GUIDES = ("prim", "flags", "pos", "norm")
STATE = ("f32", "len", "moments")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(U32)


def _same_state(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(_bits(a[k]), _bits(b[k])) for k in STATE)


@pytest.mark.parametrize("size", tc.SIZES, ids=[f"{w}x{h}" for w, h in tc.SIZES])
def test_identity_with_the_plain_accumulation(size):
    """pos_prev = pos and norm_prev = norm: temporal_restatement.accumulate, bit for bit."""
    w, h = size
    color, g, prev, gp = tc.synthetic(w, h, 100 * w + h)
    for name, (cam, cam_prev) in tc.camera_pairs(w, h).items():
        for moments in (True, False):
            for match in (False, True):
                kw = dict(match_prim=match, moments=moments)
                want = tr.accumulate(color, g, cam, prev, gp, cam_prev, **kw)
                got = mr.accumulate_motion(color, g, cam, g["pos"], g["norm"], prev, gp, cam_prev, **kw)
                assert _same_state(got, want), (size, name, kw)
    assert _same_state(mr.accumulate_motion(color, g, tc.camera(w, h)), tr.accumulate(color, g, tc.camera(w, h)))


def test_non_finite_motion_starts_a_history():
    """A pixel whose pos_prev or norm_prev is NaN, inf or beyond 2^100 is still valid and has len 1."""
    w, h = 67, 35
    color, g, prev, gp = tc.synthetic(w, h, 11)
    cam, cam_prev = tc.camera_pairs(w, h)["subpixel"]
    base = tr.accumulate(color, g, cam, prev, gp, cam_prev)
    v = tr.valid_mask(color, g)
    found = v & (base["len"] > 1)
    assert found.sum() > 100
    for field in ("pos", "norm"):
        for bad in tc.BAD:
            pp, npv = g["pos"].copy(), g["norm"].copy()
            (pp if field == "pos" else npv)[..., 1][found] = bad
            st = mr.accumulate_motion(color, g, cam, pp, npv, prev, gp, cam_prev)
            assert (st["len"][found] == 1).all() and (st["len"][~v] == 0).all(), (field, bad)
            assert np.array_equal(_bits(st["f32"][found]), _bits(color[found]))
            assert np.array_equal(_bits(st["len"][~found]), _bits(base["len"][~found]))


# ---- the moving bunny through the oracle's G-buffer ------------------------------------------------

def _oracle_sequence(wgt, oracle, motion):
    """Six frames of the 2,000-triangle bunny scene at 64 x 48, spp 4, seed = frame index, a static
    camera: each frame's mesh (TRI_DTYPE, original order) and G-buffer (the oracle's closest hits on
    sample 0's camera rays through hit_records.expected_records)."""
    L, Q, S, T = wgt.mesh_scene("bunny", 2000)
    nlq = len(L) + len(Q)
    meshes, frames = [], []
    for f, verts in enumerate(mr.sequence_vertices(T, motion, FRAMES)):
        tris = T.copy() if f == 0 else wgt.make_triangles(verts)
        tris["col"], tris["emissive"] = T["col"], T["emissive"]
        o, d = camera_rays(oracle.camera_param(W / H, 4, f), W, H)
        rec, is_tri = hr.expected_records(oracle.OracleScene(L, Q, S, tris), L, Q, S, tris, o.reshape(-1, 3), d.reshape(-1, 3))
        meshes.append(tris)
        frames.append(({k: rec[k].reshape((H, W) + rec[k].shape[1:]) for k in GUIDES}, is_tri.reshape(H, W)))
    return nlq, meshes, frames


@pytest.fixture(scope="module", params=["translate", "rotate"])
def sequence(request, wgt, oracle):
    return (request.param,) + _oracle_sequence(wgt, oracle, request.param)


def test_unmoved_mesh_passes_through(sequence):
    _, nlq, meshes, frames = sequence
    g = frames[0][0]
    m = mr.reproject(g, nlq, meshes[0], meshes[0].copy())
    assert np.array_equal(_bits(m["pos_prev"]), _bits(g["pos"])) and np.array_equal(_bits(m["norm_prev"]), _bits(g["norm"]))


def test_reprojection_is_accurate_against_float64(sequence):
    """The float32 pos_prev against the same formula in float64 from the same float32 inputs: at most
    4 * 2^-23 * (the largest |vertex coordinate| of the two meshes); a chain of about ten roundings.
    Measured: 0.58 (translation) and 0.60 (rotation) of that unit."""
    motion, nlq, meshes, frames = sequence
    worst = 0.0
    for f in range(1, FRAMES):
        g, is_tri = frames[f]
        assert is_tri.sum() > 100  # the bunny covers some 240 of the 3,072 pixels
        m32 = mr.reproject(g, nlq, meshes[f], meshes[f - 1])
        m64 = mr.reproject(g, nlq, meshes[f], meshes[f - 1], dtype=np.float64)
        unit = 2.0 ** -23 * max(np.abs(mr.vertices_of(meshes[k])).max() for k in (f - 1, f))
        err = np.abs(m32["pos_prev"].astype(np.float64) - m64["pos_prev"])[is_tri].max() / unit
        worst = max(worst, float(err))
        # pixels that hit no triangle pass through exactly
        assert np.array_equal(_bits(m32["pos_prev"][~is_tri]), _bits(g["pos"][~is_tri]))
        assert np.array_equal(_bits(m32["norm_prev"][~is_tri]), _bits(g["norm"][~is_tri]))
    print(f"{motion}: max |pos_prev32 - pos_prev64| = {worst:.3f} x 2^-23 x max|coordinate|")
    assert worst <= 4.0, worst


def test_history_follows_the_mesh(sequence):
    """Chains A (the plain restatement) and B (the motion form) over the six frames with a constant
    colour: at frame 5, as shares of the triangle pixels, A keeps len >= 3 on at most 0.15
    (translation) / 0.25 (rotation), B has the full history len == 6 on at least 0.60 / 0.65; len on
    pixels that hit no triangle is equal between A and B at every frame.

    A length is the bilinear mean of the taps' lengths plus one, so "len == 6" is the length that
    rounds to 6 (motion_restatement.shares says why).  Measured: A 0.051 and 0.126; B 0.730 and 0.779,
    the figures this work was proposed with; with exact float equality B is 0.595 and 0.545, printed
    beside them.  What keeps B from 1 is the plane test between neighbouring pixels of the coarsely
    faceted mesh under a fractional history coordinate, DESIGN.md §4.10."""
    motion, nlq, meshes, frames = sequence
    color = np.full((H, W, 4), 0.5, f32)
    color[..., 3] = 1.0
    a, b = mr.chains([g for g, _ in frames], [color] * FRAMES, tc.camera(W, H), meshes, nlq)
    for f in range(FRAMES):
        other = ~frames[f][1]
        assert np.array_equal(_bits(a[f]["len"][other]), _bits(b[f]["len"][other])), f
    share_a, share_b = mr.shares(a[-1], b[-1], frames[-1][1], FRAMES)
    exact = float((b[-1]["len"][frames[-1][1]] == FRAMES).mean())
    print(f"{motion}: A len >= 3: {share_a:.3f}; B len == 6: {share_b:.3f} (exactly 6.0: {exact:.3f})")
    max_a, min_b = {"translate": (0.15, 0.60), "rotate": (0.25, 0.65)}[motion]
    assert share_a <= max_a, share_a
    assert share_b >= min_b, share_b
