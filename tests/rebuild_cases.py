"""Meshes for the rebuild tests.  TEST INFRASTRUCTURE ONLY.

Shared by tests/test_rebuild_host.py (wgt_bvh_build_morton against tests/rebuild_restatement.py, on
the CPU) and tests/test_gpu_rebuild.py (wgt_rebuild_triangles against wgt_bvh_build_morton).  Each
mesh is the smallest at which one step of the build can go wrong; the largest has 2075 triangles.
"""
import functools

import numpy as np

import refit_cases as rc

f32 = np.float32
LEAF = 4  # the default leaf target (wgt_morton.h kRebuildLeafDefault)

# leaf and level edges for the leaf target L, the 256-lane block's edge, then the shaped meshes
COUNTS = ("n1", "n2", "nL", "nL+1", "n4L", "n4L+1", "n16L+1", "n255", "n256", "n257")
SHAPED = ("one", "nine", "bunny2000", "chain", "same64", "sheet", "tiny", "huge")
CASES = COUNTS + SHAPED


def _wgt():
    import webgputracer_amd

    return webgputracer_amd


def count_of(name, L):
    """The triangle count of a COUNTS case for the leaf target L."""
    return {"n1": 1, "n2": 2, "nL": L, "nL+1": L + 1, "n4L": 4 * L, "n4L+1": 4 * L + 1, "n16L+1": 16 * L + 1,
            "n255": 255, "n256": 256, "n257": 257}[name]


@functools.lru_cache(maxsize=None)
def case(name, L=LEAF):
    """Triangles (TRI_DTYPE) of one case."""
    w = _wgt()
    if name in COUNTS:  # the first n triangles of the bunny
        return rc.mesh("bunny2000")[:count_of(name, L)].copy()
    if name in rc.MESHES:
        return rc.mesh(name)
    if name == "same64":  # all codes equal: the order is the indices', every split the median
        return np.repeat(rc.mesh("one"), 64)
    if name == "sheet":  # a coplanar sheet: every centre has the same y, so that axis has no extent
        g = np.arange(12, dtype=np.float64) * 20.0
        x, z = [a.reshape(-1) for a in np.meshgrid(g, g)]
        y = np.full_like(x, 100.0)
        v0 = np.stack([x, y, z], 1)
        v = np.stack([v0, v0 + [15.0, 0.0, 0.0], v0 + [0.0, 0.0, 15.0]], 1)
        return w.make_triangles(v.astype(f32))
    if name in ("tiny", "huge"):  # the bunny scaled by 2^-12 and by 2^20: the compact step moves
        return w.make_triangles((rc.vertices(rc.mesh("bunny2000")) * (2.0 ** -12 if name == "tiny" else 2.0 ** 20)).astype(f32))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def permuted(seed=12):
    """bunny2000 with its triangles' positions permuted among the indices: triangle i lies where triangle
    perm[i] lay, so every node of a tree refit to it spans the mesh."""
    A = rc.mesh("bunny2000")
    return A[np.random.default_rng(seed).permutation(len(A))].copy()
