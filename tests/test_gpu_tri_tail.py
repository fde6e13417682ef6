"""The triangle step's single tail (wgt_trav_ps.h tri_step) against the oracle,
bit for bit as tests/test_gpu_parity.py compares: a 64 x 36 frame at 4 spp (radiance words, bytes,
hit ids, counters) and a wgt_trace_rays query of camera-like rays, on scenes built so that the tail
is entered in every way it can be:

  leaves      SAH leaves of exactly 1, 2, 3, 5, 7 and 8 coplanar triangles: odd counts leave slot 1
              dead on a leaf's last step
  near_first  two overlapping triangles in one leaf, both slots pass, t0 < t1
  far_first   the same with t0 > t1
  tie_up      the same triangle twice, t0 == t1, slot 0 holds the lower index
  tie_down    ... slot 0 holds the higher index
  bound       both slots pass behind the back wall: neither beats the quad-seeded bound
  clamp_big   the scene of tests/test_gpu_numerics.py scaled by 2^20 with two coplanar triangles in
              the plane z = 0: their padded boxes are 2e-6 thick there, thinner than Moller-Trumbore's
              error in t, so the clamp to the box's slab interval moves t
  clamp_small the scene scaled by 2^-20 with two coplanar triangles in z = 0 whose edges are 768 long,
              seen from a camera a thousand units away.  From the scaled camera (7.6e-4 from the
              plane) the pad's absolute 1e-6 makes the slab interval 2.6e-3 t wide around t = 1, a
              thousand times Moller-Trumbore's error, and the clamp can move nothing at that scale
              whatever the triangle; from a thousand units the interval is narrower than an ulp of t

What each scene is built for is asserted on the CPU when the cases are built (the builder's leaves
and slot order from wgt_bvh_build's export; passing slots, the bound and the clamp with the oracle
and tests/tri_tail_restatement.py), so a case that does not exercise its path is an error, not a
pass.  Every case runs under two schedules of the persistent kernel (the phase thresholds 18/16
with a triangle ratio of 70, and 10/8 with 150): the result does not depend on the schedule."""
import numpy as np
import pytest

import tri_tail_restatement as R
from test_gpu_mode_runs import leaf_ranges
from test_gpu_numerics import scale_scene, scaled_camera
from test_gpu_parity import assert_radiance, check_counters

pytestmark = pytest.mark.gpu

W, H, SPP = 64, 36, 4
U32, f32 = np.uint32, np.float32
SCHEDULES = [{"WGT_PS_TO_TRAV": "18", "WGT_PS_TO_SERVICE": "16", "WGT_TRI_RATIO": "70"},
             {"WGT_PS_TO_TRAV": "10", "WGT_PS_TO_SERVICE": "8", "WGT_TRI_RATIO": "150"}]
SCHEDULE_IDS = ["18_16_ratio70", "10_8_ratio150"]
BUILDER_ENV = {"WGT_SAH_LEAF": "8", "WGT_DP_LEAF": "0"}  # the leaf cap the scenes are sized for
CASES = ["leaves", "near_first", "far_first", "tie_up", "tie_down", "bound", "clamp_big", "clamp_small"]
SEEDS = dict(zip(CASES, range(11, 19)))

NEAR = [[80, 80, 250], [420, 100, 250], [250, 460, 250]]
FAR = [[90, 70, 262], [410, 110, 258], [240, 450, 266]]
# rising through the back wall (z = 555): the upper part of both lies behind it
WALL_A = [[60, 40, 380], [520, 60, 640], [280, 520, 760]]
WALL_B = [[70, 30, 388], [510, 80, 650], [270, 500, 770]]
FLAT_A = [[50, 50, 0], [500, 60, 0], [280, 500, 0]]
FLAT_B = [[60, 40, 0], [510, 80, 0], [270, 480, 0]]
P = 2.0 ** 28
HUGE_A = [[-P, -P, 0], [2 * P, -P, 0], [0, 2 * P, 0]]  # times 2^-20: (-256, -256), (512, -256), (0, 512)
HUGE_B = [[-P - 2 ** 22, -P, 0], [2 * P, -P + 2 ** 22, 0], [2 ** 22, 2 * P, 0]]


FAR_ORIGIN = (100.0, 100.0, -1000.0)  # clamp_small's camera: unscaled, a thousand units from the 5e-4 scene


def query_rays(s=1.0, origin=(278, 278, -800), lo=3, hi=552, z=300):
    """Camera-like rays: from the camera's origin through a 48 x 27 grid inside the box."""
    x, y = np.meshgrid(np.linspace(lo, hi, 48), np.linspace(lo, hi, 27))
    tgt = np.stack([x.ravel(), y.ravel(), np.full(x.size, z)], 1).astype(f32) * f32(s)
    o = np.broadcast_to(np.array(origin, f32) * f32(s), tgt.shape).copy()
    return o, tgt - o


def case_camera(mod, name, s):
    if name != "clamp_small":
        return scaled_camera(mod, W / H, SPP, SEEDS[name], s)
    cam = mod.camera_param(W / H, SPP, SEEDS[name])
    cam["origin"][..., :3] = FAR_ORIGIN
    cam["target"][..., :3] = (FAR_ORIGIN[0], FAR_ORIGIN[1], 0.0)
    return cam


def tri_vecs(T, idx):
    return tuple(tuple(T[k][idx, c] for c in range(3)) for k in ("v0", "e1", "e2"))


def both_pass(T, o, d, i0, i1):
    """Moller-Trumbore of triangles i0 and i1 for every ray (numpy restatement): passes and t."""
    oo, dd = tuple(o.T), tuple(d.T)
    n = len(o)
    a = R.mt_test(oo, dd, *tri_vecs(T, np.full(n, i0)))
    b = R.mt_test(oo, dd, *tri_vecs(T, np.full(n, i1)))
    return a, b


def slots_of(wgt, T, i0, i1):
    """The original indices in slots 0 and 1 of the triangle step that tests T[i0] and T[i1] together,
    or None when the builder's leaf order does not put the two in one step."""
    _, nodes, recs = wgt.bvh_build(T)
    idx = np.ascontiguousarray(recs[:, 0, 3]).view(U32)
    first, count = leaf_ranges(nodes)
    pa, pb = int(np.flatnonzero(idx == i0)[0]), int(np.flatnonzero(idx == i1)[0])
    lo = min(pa, pb)
    leaf = int(np.searchsorted(first, lo, side="right")) - 1
    if abs(pa - pb) != 1 or (lo - int(first[leaf])) % 2 or lo + 1 >= int(first[leaf]) + int(count[leaf]):
        return None
    return int(idx[lo]), int(idx[lo + 1])


def arrange(wgt, a, b, want):
    """Triangles a and b with up to six small filler triangles beside them, in the first input order
    for which the builder puts a and b into one triangle step with want(slot 0's index, slot 1's
    index, a's index, b's index) true.  The builder partitions in place (std::partition), so the
    order of a leaf's records depends on what else the scene holds and where."""
    rng = np.random.default_rng(5)
    sides = [np.array([500, 40, 300], f32), np.array([8, 40, 300], f32)]
    for side in sides:
        fill = [(side + rng.uniform(0, 30, (3, 3))).astype(f32) for _ in range(6)]
        for nf in range(7):
            for pos in range(nf + 1):
                for first, second in ((a, b), (b, a)):
                    verts = fill[:pos] + [np.array(first, f32), np.array(second, f32)] + fill[pos:nf]
                    T = wgt.make_triangles(np.array(verts, f32))
                    ia, ib = (pos, pos + 1) if first is a else (pos + 1, pos)
                    s = slots_of(wgt, T, ia, ib)
                    if s is not None and want(s[0], s[1], ia, ib):
                        return T, ia, ib
    raise AssertionError("no input order puts the two triangles into one step as wanted")


def leaves_mesh(wgt):
    """Clusters of 1, 2, 3, 5, 7 and 8 coplanar, nearly coincident triangles (each size twice), far
    enough apart that the builder keeps each cluster as one leaf."""
    rng = np.random.default_rng(7)
    sizes = [1, 2, 3, 5, 7, 8] * 2
    rng.shuffle(sizes)
    verts = []
    for i, k in enumerate(sizes):
        centre = np.array([90 + 125 * (i % 4), 70 + 150 * (i // 4), 150 + 60 * (i % 3)], f32)
        base = rng.uniform(-55, 55, (3, 3)).astype(f32)
        base[:, 2] = 0  # one plane per cluster
        for _ in range(k):
            jit = rng.uniform(-1.5, 1.5, (3, 3)).astype(f32)
            jit[:, 2] = 0
            verts.append(centre + base + jit)
    return wgt.make_triangles(np.array(verts, f32))


def build_case(name, wgt, oracle):
    """(scene, oracle frame, query rays, oracle answers) of one case, with the CPU checks of what the
    case is for."""
    s = 1.0
    L, Q, S = wgt.cornell_scene()
    Q = Q[:5].copy()
    nlq = len(L) + len(Q)
    if name == "leaves":
        T = leaves_mesh(wgt)
        _, nodes, _ = wgt.bvh_build(T)
        first, count = leaf_ranges(nodes)
        assert sorted(set(count.tolist())) == [1, 2, 3, 5, 7, 8], sorted(set(count.tolist()))
    elif name in ("near_first", "far_first"):
        near0 = name == "near_first"
        T, ia, ib = arrange(wgt, NEAR, FAR, lambda s0, s1, a, b: (s0 == a) == near0)
    elif name in ("tie_up", "tie_down"):
        up = name == "tie_up"
        T, ia, ib = arrange(wgt, NEAR, NEAR, lambda s0, s1, a, b: (s0 < s1) == up)
    elif name == "bound":
        T, ia, ib = arrange(wgt, WALL_A, WALL_B, lambda *_: True)
    else:
        s = 2.0 ** 20 if name == "clamp_big" else 2.0 ** -20
        pair = (FLAT_A, FLAT_B) if name == "clamp_big" else (HUGE_A, HUGE_B)
        T0 = wgt.make_triangles(np.array(pair, f32))
        L, Q, S, T = scale_scene(wgt, s, T0)
        ia, ib = 0, 1
        assert slots_of(wgt, T, 0, 1) is not None
    scene = (L, Q, S, T)
    osc = oracle.OracleScene(*scene)
    o, d = query_rays(1.0, FAR_ORIGIN, -150, 350, 37) if name == "clamp_small" else query_rays(s)
    prim, dist = osc.trace(o, d)
    if name != "leaves":
        (ok_a, t_a), (ok_b, t_b) = both_pass(T, o, d, ia, ib)
        both = ok_a & ok_b
        assert both.sum() > 50, f"{name}: both slots pass for {both.sum()} rays"
        if name in ("near_first", "far_first"):
            assert (both & (t_a < t_b)).sum() > 50  # a is NEAR: the slot order was asserted by arrange
        if name in ("tie_up", "tie_down"):
            assert np.array_equal(t_a.view(U32), t_b.view(U32))
        if name == "bound":
            assert (both & (prim < nlq)).sum() > 50, "both pass and a quad stays the closest hit"
            assert (both & (prim >= nlq)).sum() > 50
    if name.startswith("clamp"):
        tid, t = osc.trace_tris(o, d)
        hit = tid != R.NO_HIT
        idx = np.where(hit, tid, 0)
        oo, dd = tuple(o.T), tuple(d.T)
        with np.errstate(all="ignore"):
            inv = tuple(f32(1.0) / c for c in dd)
            ot = tuple(-(a * b) for a, b in zip(oo, inv))
            _, t_mt = R.mt_test(oo, dd, *tri_vecs(T, idx))
            lo, hi = R.tri_box(*tri_vecs(T, idx))
            n = len(o)
            _, c = R.tri_tail(lo, hi, ot, inv, np.full(n, R.kRayMax, f32), np.full(n, R.NO_HIT, U32), t_mt, idx.astype(U32))
        moved = hit & (t != t_mt) & (t.view(U32) == c.view(U32))
        print(f"{name}: {hit.sum()} triangle hits, the clamp moved t for {moved.sum()}")
        assert moved.sum() > 0, f"{name}: the clamp moves no sampled ray's t"
    return scene, osc.render(case_camera(oracle, name, s), W, H), (o, d), (prim, dist), s


@pytest.fixture(scope="module")
def cases(wgt, oracle):
    mp = pytest.MonkeyPatch()
    for k, v in BUILDER_ENV.items():
        mp.setenv(k, v)
    try:
        return {name: build_case(name, wgt, oracle) for name in CASES}
    finally:
        mp.undo()


@pytest.mark.parametrize("env", SCHEDULES, ids=SCHEDULE_IDS)
@pytest.mark.parametrize("name", CASES)
def test_single_tail_vs_oracle(ctx, wgt, oracle, cases, name, env, monkeypatch):
    scene, ref, (o, d), (rprim, rdist), s = cases[name]
    for k, v in {**BUILDER_ENV, **env}.items():
        monkeypatch.setenv(k, v)
    ctx.upload_scene(*scene)
    g = ctx.render_tile(case_camera(wgt, name, s), W, H, stats=True)
    assert_radiance(g["f32"], ref["f32"])
    assert np.array_equal(g["u8"], ref["u8"])
    assert np.array_equal(g["hit"], ref["hit"])
    check_counters(g["stats"], ref["counters"], oracle)
    assert g["stats"]["tri_tests"] > 0
    prim, dist = ctx.trace_rays(o, d)
    assert np.array_equal(prim, rprim)
    assert np.array_equal(dist.view(U32), rdist.view(U32))
