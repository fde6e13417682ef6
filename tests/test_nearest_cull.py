"""The closest-point kernel's culling argument (wgt_nearest.h) checked pair by pair on the
CPU: for every point and every triangle with a finite d2, the cull bound of the triangle's own padded box
(wgt_geom.h tri_box, which nests in every node box above it), computed with nearest_gap's float32
operations restated in numpy, stays at or below fl(d2 F).  A box is culled only when its bound exceeds
fl(best F), so this is what keeps a triangle with d2 <= best from being dropped.  The plain bound (no
shrink, no factor) is reported beside it.  CPU only."""
import numpy as np
import pytest

import adversarial_meshes as am
import nearest_cases as nc
import nearest_restatement as nr
import refit_cases as rc

f32 = np.float32
SHRINK, FACTOR = f32(2.0 ** -8), f32(1.0 + 2.0 ** -6)  # wgt_nearest.h kNearestShrink, kNearestCullFactor


def box_bound(lo, hi, p, shrink):
    """nearest_box_bound for points (n, 3) x boxes (t, 3)."""
    g = []
    for a in range(3):
        gap = np.maximum(lo[None, :, a] - p[:, None, a], p[:, None, a] - hi[None, :, a])
        g.append(np.maximum(gap - shrink * (hi[None, :, a] - lo[None, :, a]), f32(0)))
    return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]


def _near(T, n, seed):
    rng = np.random.default_rng(seed)
    c = nc.centroids(T, rng.integers(0, len(T), n))
    return (c + rng.normal(size=c.shape) * (0.05 * np.linalg.norm(c, axis=1, keepdims=True) + 5.0)).astype(f32)


def _cases():
    B = nc.bunny
    return {
        "bunny box": lambda: (B(), nc.box_points()[:500]),
        "bunny surface": lambda: (B(), nc.surface_points()[:500]),
        "bunny far 1e3": lambda: (B(), nc.far_points(1e3)[:200]),
        "bunny far 1e5": lambda: (B(), nc.far_points(1e5)[:200]),
        "bunny far 1e7": lambda: (B(), nc.far_points(1e7)[:200]),
        "slivers": lambda: (am.small_mesh("slivers"), np.concatenate([_near(am.small_mesh("slivers"), 500, 11), nc.small_points(500, 4)])),
        "geometric_up": lambda: (am.small_mesh("geometric_up"), _near(am.small_mesh("geometric_up"), 500, 12)),
        "degenerate": lambda: (nc.degenerate_mix(), nc.small_points()),
    }


@pytest.mark.parametrize("name", list(_cases()))
def test_cull_bound_is_below_the_computed_d2(name):
    T, P = _cases()[name]()
    lo, hi = (x.astype(f32) for x in rc.tri_boxes(T))
    v0, e1, e2 = (np.ascontiguousarray(T[k][:, :3], f32)[None] for k in ("v0", "e1", "e2"))
    pairs = bad = plain = 0
    for a in range(0, len(P), 250):
        p = P[a:a + 250]
        with np.errstate(all="ignore"):
            d2 = nr.nearest_on_tri(p[:, None, :], v0, e1, e2)[0]
            fin = d2 < f32(np.inf)
            bad += int((fin & (box_bound(lo, hi, p, SHRINK) > d2 * FACTOR)).sum())
            plain += int((fin & (box_bound(lo, hi, p, f32(0)) > d2)).sum())
        pairs += int(fin.sum())
    print(f"{name}: {pairs} pairs, {bad} above fl(d2 F), {plain} above d2 without shrink and factor")
    assert pairs > 0 and bad == 0
