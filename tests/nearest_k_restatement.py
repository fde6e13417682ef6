"""The k-nearest closest-point query's definition (webgputracer_amd/csrc/wgt_nearest_k.h) a
third time, in numpy: nearest_restatement's per-triangle d2, a stable sort by (d2, index) over the triangles
with a finite d2, and the radius prefix.  TEST INFRASTRUCTURE ONLY.

    ranked(tris, points) -> Ranked: per point every triangle's (d2, index) in the definition's order, computed once
    nearest_k_points(ranked, k, max_dist=None, first_prim=0) -> dict(count, prim, dist, pos, uv)
"""
import numpy as np

from nearest_restatement import nearest_on_tri

f32 = np.float32
NO_HIT = np.uint32(0xFFFFFFFF)
MAX_K = 32


class Ranked:
    """Per point the first `keep` triangles by (d2, index), d2 finite first: order (n, keep) indices, d2,
    dist = sqrt(d2), q, v, w along that order, ok (n, keep) whether the entry's d2 is finite, and all_dist
    (n, n_tris) every triangle's dist (NaN or inf where d2 is not finite) for the count."""

    def __init__(self, tris, points, keep=MAX_K + 8, chunk=128):
        points = np.asarray(points, f32).reshape(-1, 3)
        n, nt = len(points), len(tris)
        self.n, self.nt, keep = n, nt, min(keep, nt)
        self.order = np.zeros((n, keep), np.int64)
        self.d2 = np.full((n, keep), np.inf, f32)
        self.q = np.zeros((n, keep, 3), f32)
        self.vw = np.zeros((n, keep, 2), f32)
        self.ok = np.zeros((n, keep), bool)
        self.all_dist = np.full((n, nt), np.inf, f32)
        if nt == 0:
            return
        v0, e1, e2 = (np.ascontiguousarray(tris[k][:, :3], f32)[None] for k in ("v0", "e1", "e2"))
        # a point with a NaN or infinite component has no finite d2: the definition says so outright
        finite = np.isfinite(points).all(1)
        for a in range(0, n, chunk):
            dd, v, w, q, _ = nearest_on_tri(points[a:a + chunk, None, :], v0, e1, e2)
            ok = (dd < f32(np.inf)) & finite[a:a + chunk, None]  # not NaN, not infinite
            key = np.where(ok, dd, f32(np.inf))
            order = np.argsort(key, axis=1, kind="stable")[:, :keep]  # stable: ties keep the lower index first
            r = np.arange(len(order))[:, None]
            sl = slice(a, a + len(order))
            self.order[sl], self.d2[sl], self.ok[sl] = order, key[r, order], ok[r, order]
            self.q[sl] = q[r, order]
            self.vw[sl] = np.stack([v[r, order], w[r, order]], -1)
            with np.errstate(invalid="ignore"):
                self.all_dist[sl] = np.where(ok, np.sqrt(dd), f32(np.inf))
        with np.errstate(invalid="ignore"):
            self.dist = np.sqrt(self.d2)
        assert self.dist.dtype == f32


def nearest_k_points(rk, k, max_dist=None, first_prim=0):
    """count = the triangles with a finite d2 and dist < m; entry j < k = the j-th triangle of the order if it
    is one of them (they are a prefix of the order), else the miss entry."""
    n = rk.n
    lim = np.full(n, np.inf, f32) if max_dist is None else np.broadcast_to(np.asarray(max_dist, f32), (n,))
    out = {"count": np.zeros(n, np.uint32), "prim": np.full((n, k), NO_HIT, np.uint32), "dist": np.full((n, k), np.inf, f32),
           "pos": np.zeros((n, k, 3), f32), "uv": np.zeros((n, k, 2), f32)}
    if rk.nt == 0:
        return out
    with np.errstate(invalid="ignore"):
        # all_dist is +inf where d2 is not finite, and +inf is below no m
        out["count"] = (rk.all_dist < lim[:, None]).sum(1).astype(np.uint32)
        kk = min(k, rk.order.shape[1])
        have = rk.ok[:, :kk] & (rk.dist[:, :kk] < lim[:, None])
    assert kk == k or kk == rk.nt  # fewer than k only when the mesh has fewer
    out["prim"][:, :kk] = np.where(have, np.uint32(first_prim) + rk.order[:, :kk].astype(np.uint32), NO_HIT)
    out["dist"][:, :kk] = np.where(have, rk.dist[:, :kk], f32(np.inf))
    out["pos"][:, :kk] = np.where(have[..., None], rk.q[:, :kk], f32(0))
    out["uv"][:, :kk] = np.where(have[..., None], rk.vw[:, :kk], f32(0))
    return out
