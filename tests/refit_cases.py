"""Meshes, motions and numpy restatements for the BVH refit tests.  TEST INFRASTRUCTURE ONLY.

Shared by tests/test_refit_host.py (RefitBvh through wgt_bvh_refit, on the CPU) and
tests/test_gpu_refit.py (wgt_update_triangles).  The meshes are the smallest at which each refit
kernel can go wrong; the motions A -> B change the compact form's scene-wide bound and step in
either direction.  A motion may carry a mesh beyond the scene limits (the chain mesh spans 5e10, so
its scale by 8 and its jitter push edge components past 2^30): within_limits says so from B alone,
and for such a case the tests assert the refusal the C-ABI specifies instead of the tree.
"""
import functools

import numpy as np

import adversarial_meshes as am

f32 = np.float32
MESHES = ("one", "nine", "bunny2000", "chain")
MOTIONS = ("identity", "translate1000", "shrink64", "scale8", "jitter5", "collapse")
COORD_LIMIT, EDGE_LIMIT = 2.0 ** 40, 2.0 ** 30  # host/launch_plan.h
EMPTY = f32(3e38)  # wgt_geom.h kEmptySlotCoord


def _wgt():
    import webgputracer_amd

    return webgputracer_amd


@functools.lru_cache(maxsize=None)
def mesh(name):
    """Triangles (TRI_DTYPE) of mesh A."""
    w = _wgt()
    if name == "one":  # a root with one leaf and one empty slot
        return w.make_triangles(np.array([[[100, 120, 140], [160, 130, 150], [110, 190, 170]]], f32))
    if name == "nine":  # two leaves
        rng = np.random.default_rng(9)
        c = rng.uniform(50.0, 450.0, (9, 3))
        return w.make_triangles(am.tri_at(c, 30.0, rng))
    if name == "bunny2000":  # several partial waves per level
        return w.procedural_mesh("bunny", 2000)
    if name == "chain":  # the deepest chain mesh an upload accepts: the depth and stack limits
        return am.small_mesh("geometric_up")
    raise KeyError(name)


def vertices(tris):
    """(n, 3, 3) float64 vertices of TRI_DTYPE triangles."""
    v0 = tris["v0"][:, :3].astype(np.float64)
    return np.stack([v0, v0 + tris["e1"][:, :3], v0 + tris["e2"][:, :3]], axis=1)


def rotate_y(tris, degrees):
    """The triangles turned about the vertical axis through their bounding box's centre."""
    v = vertices(tris)
    c = 0.5 * (v.reshape(-1, 3).min(0) + v.reshape(-1, 3).max(0))
    a = np.radians(degrees)
    R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
    return _wgt().make_triangles(((v - c) @ R.T + c).astype(f32))


@functools.lru_cache(maxsize=None)
def moved(name, motion):
    """Triangles of B = motion(A), same count and order."""
    A = mesh(name)
    if motion == "identity":
        return A
    v = vertices(A)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    if motion == "translate1000":
        v = v + np.array([1000.0, 0.0, 0.0])
    elif motion == "shrink64":  # about the box's lower corner: the step shrinks
        v = lo + (v - lo) * 2.0 ** -6
    elif motion == "scale8":
        v = lo + (v - lo) * 8.0
    elif motion == "jitter5":  # per vertex, 5 % of the mesh size
        rng = np.random.default_rng(5)
        v = v + rng.uniform(-1.0, 1.0, v.shape) * 0.05 * np.linalg.norm(hi - lo)
    elif motion == "collapse":  # every triangle to its v0: zero area
        v = np.repeat(v[:, :1], 3, axis=1)
    else:
        raise KeyError(motion)
    return _wgt().make_triangles(v.astype(f32))


def within_limits(tris):
    """check_scene_limits on triangles, restated: coordinates within 2^40, edge components within 2^30."""
    with np.errstate(invalid="ignore"):
        ok = [np.all(np.abs(tris[k][:, :3].astype(np.float64)) <= COORD_LIMIT) for k in ("v0", "e1", "e2")]
        ok += [np.all(np.abs(tris[k][:, :3].astype(np.float64)) <= EDGE_LIMIT) for k in ("e1", "e2")]
    return bool(all(ok))


def extent(tris):
    """launch_plan.h scene_extent of triangles alone (float64)."""
    v = vertices(tris)
    return float(np.abs(v).max())


def tri_boxes(tris):
    """wgt_geom.h tri_box with the same float32 operations: (lo (n, 3), hi (n, 3))."""
    a = tris["v0"][:, :3].astype(f32)
    b = a + tris["e1"][:, :3].astype(f32)
    d = a + tris["e2"][:, :3].astype(f32)
    mn = np.minimum(np.minimum(a, b), d)
    mx = np.maximum(np.maximum(a, b), d)
    pad = ((mx - mn) * f32(1e-4) + (np.abs(mn) + np.abs(mx)) * f32(1e-5)) + f32(1e-6)
    assert pad.dtype == f32
    return mn - pad, mx + pad


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def refs_of(nodes):
    return bits(nodes[:, 6, :]).view(np.int32)


def live_slots(nodes):
    """(n, 4) bool: wgt_geom.h's empty slot is the point box at EMPTY."""
    return ~((nodes[:, 0, :] == EMPTY) & (nodes[:, 1, :] == EMPTY))


def expected_nodes(nodes, recs):
    """The nodes with every live slot's box recomputed bottom-up as the exact min/max union of the record
    boxes below it (refs point forward, so one pass from the last node to the root)."""
    out = nodes.copy()
    refs, live = refs_of(nodes), live_slots(nodes)
    rlo = np.stack([recs[:, 1, 3], recs[:, 2, 3], recs[:, 3, 0]], 1)
    rhi = recs[:, 3, 1:4]
    for k in range(len(nodes) - 1, -1, -1):
        for s in range(4):
            if not live[k, s]:
                continue
            r = int(refs[k, s])
            if r < 0:
                u = ~r & 0xFFFFFFFF
                first, cnt = u >> 3, (u & 7) + 1
                lo, hi = rlo[first:first + cnt].min(0), rhi[first:first + cnt].max(0)
            else:
                assert r > k
                c = live[r]
                lo, hi = out[r, 0:6:2][:, c].min(1), out[r, 1:6:2][:, c].max(1)
            out[k, 0:6:2, s] = lo
            out[k, 1:6:2, s] = hi
    return out


def compact_margin_violations(nodes, cnodes, step, origin_bound):
    """Count decoded compact planes without CompactNode's margin, in float64: a live slot's lo plane must lie
    <= lo - G and its hi plane >= hi + G, G = 2^-21 M, M = max(origin_bound, 2 max |coordinate|); an empty
    slot's codes must be +inf (0x7c00)."""
    live = live_slots(nodes)
    coords = nodes[:, :6, :].astype(np.float64)
    M = max(origin_bound, 2.0 ** -60, 2.0 * np.abs(coords[np.broadcast_to(live[:, None, :], coords.shape)]).max())
    G = M * 2.0 ** -21
    s = float(step)
    bad = 0
    for a in range(3):
        orgd = cnodes[:, a].copy().view(f32).astype(np.float64) * s
        w = cnodes[:, 4 + 4 * a:8 + 4 * a]
        codes = np.stack([w[:, 0] & 0xFFFF, w[:, 0] >> 16, w[:, 1] & 0xFFFF, w[:, 1] >> 16,
                          w[:, 2] & 0xFFFF, w[:, 2] >> 16, w[:, 3] & 0xFFFF, w[:, 3] >> 16], 1).astype(np.uint16)
        bad += int(np.sum(codes.reshape(-1, 2, 4)[~np.stack([live, live], 1)] != 0x7C00))
        with np.errstate(over="ignore", invalid="ignore"):
            plane = orgd[:, None] + codes.view(np.float16).astype(np.float64) * s
        lo_ok = plane[:, :4] <= coords[:, 2 * a, :] - G
        hi_ok = plane[:, 4:] >= coords[:, 2 * a + 1, :] + G
        bad += int(np.sum(~lo_ok & live)) + int(np.sum(~hi_ok & live))
    return bad


def assert_trees_equal(got, want, what=""):
    """(nodes, recs, cnodes, crefs, step) by bits."""
    for name, g, w in zip(("nodes", "tris", "cnodes", "crefs"), got[:4], want[:4]):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        ne = bits(g) != bits(w)
        assert not ne.any(), f"{what}: {name} differ in {int(ne.sum())} words, first at {np.argwhere(ne)[0].tolist()}"
    assert bits(f32(got[4])) == bits(f32(want[4])), (what, "step", got[4], want[4])
