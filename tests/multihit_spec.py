"""The multi-hit query's specification for tests, from the untouched CPU oracle.  TEST INFRASTRUCTURE ONLY.

wgt_trace_multi_hits (include/wgt_api.h) calls a primitive hit when the closest-hit code accepts it tested
alone.  So for each primitive p of a scene this builds an OracleScene that holds p alone (the other three
lists empty) and traces the rays through it: that is p's accept decision and distance.  The limit rule
(dist < min(max_dist, 1e20) as float32, nothing below a zero, negative or NaN limit), the non-finite-ray
rule (no hits) and the order (dist, primitive id) are applied here.  Ids are wgt_trace_rays': lights,
quads, triangles, spheres.
"""
import numpy as np

NO_HIT = np.uint32(0xFFFFFFFF)
INF = np.float32(np.inf)
RAY_MAX = np.float32(1e20)


def uv_sphere(center, radius, segments=12, rings=8):
    """(segments * (2 * rings - 2), 3, 3) float32 vertices of a closed UV sphere."""
    c = np.asarray(center, np.float64)
    lat = np.pi * np.arange(rings + 1) / rings
    lon = 2.0 * np.pi * np.arange(segments + 1) / segments

    def p(i, j):
        j %= segments  # the seam's vertices are the same floats
        return c + radius * np.array([np.sin(lat[i]) * np.cos(lon[j]), np.cos(lat[i]), np.sin(lat[i]) * np.sin(lon[j])])

    tris = []
    for i in range(rings):
        for j in range(segments):
            a, b, cc, d = p(i, j), p(i, j + 1), p(i + 1, j + 1), p(i + 1, j)
            if i > 0:
                tris.append([a, b, cc])
            if i < rings - 1:
                tris.append([a, cc, d])
    return np.asarray(tris).astype(np.float32)


def concentric_verts(radii=(150.0, 100.0, 50.0), center=(278.0, 200.0, 278.0)):
    return np.concatenate([uv_sphere(center, r) for r in radii])


def concentric_scene(wgt, radii=(150.0, 100.0, 50.0), translation=(0.0, 0.0, 0.0)):
    """The Cornell box (its light, 17 quads and dummy sphere) plus concentric UV spheres: 168 triangles each."""
    L, Q, S = wgt.cornell_scene()
    return L, Q, S, wgt.make_triangles(concentric_verts(radii), translation=translation)


def random_rays(n, rng):
    """As tests/test_gpu_occlusion.py draws them."""
    o = rng.uniform(5, 550, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o, d.astype(np.float32)


class MultiHitSpec:
    """Every primitive's accept decision and distance for n rays, computed once; answer() applies a limit,
    the triangle filter and k."""

    def __init__(self, oracle, L, Q, S, T, o, d):
        o = np.ascontiguousarray(o, np.float32).reshape(-1, 3)
        d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
        self.n = len(o)
        self.finite = np.isfinite(o).all(1) & np.isfinite(d).all(1)
        # a non-finite ray has no hits by definition: the oracle is not asked about it
        oo, dd = o.copy(), d.copy()
        oo[~self.finite] = 0.0
        dd[~self.finite] = (0.0, 0.0, 1.0)
        T = np.zeros(0, oracle.TRI_DTYPE) if T is None else T
        self.n_lq, self.n_tris = len(L) + len(Q), len(T)
        self.P = self.n_lq + len(T) + len(S)
        self.acc = np.zeros((self.P, self.n), bool)
        self.dist = np.full((self.P, self.n), INF, np.float32)
        pid = 0
        for which, arr in enumerate((L, Q, T, S)):
            for j in range(len(arr)):
                parts = [a[:0] for a in (L, Q, S, T)]
                parts[(0, 1, 3, 2)[which]] = arr[j:j + 1]
                sc = oracle.OracleScene(*parts)
                prim, dist = sc.trace(oo, dd)
                sc.close()
                self.acc[pid] = (prim != NO_HIT) & self.finite
                self.dist[pid] = dist
                pid += 1
        self.tri_row = np.zeros(self.P, bool)
        self.tri_row[self.n_lq:self.n_lq + self.n_tris] = True

    def valid(self, max_dist=None, tris_only=False):
        """(P, n) bool: primitive p is in ray i's set S."""
        m = np.broadcast_to(np.asarray(INF if max_dist is None else max_dist, np.float32), (self.n,))
        with np.errstate(invalid="ignore"):
            lim = np.where(m < RAY_MAX, m, RAY_MAX).astype(np.float32)  # min(m, 1e20); a NaN m is refused below
            v = self.acc & (self.dist < lim[None, :]) & (m > 0)[None, :]
        return v & self.tri_row[:, None] if tris_only else v

    def answer(self, k, max_dist=None, tris_only=False):
        """{"count": (n,), "prim": (n, k), "dist": (n, k)} as Context.trace_multi_hits returns them."""
        v = self.valid(max_dist, tris_only)
        count = v.sum(0).astype(np.uint32)
        dm = np.where(v, self.dist, INF)
        ids = np.broadcast_to(np.arange(self.P, dtype=np.uint32)[:, None], v.shape)
        order = np.lexsort((ids, dm), axis=0)[:k]  # by dist, then id; a member's dist is below 1e20, never inf
        prim = np.full((k, self.n), NO_HIT, np.uint32)
        dist = np.full((k, self.n), INF, np.float32)
        rows = min(k, self.P)
        have = np.arange(rows)[:, None] < count[None, :]
        prim[:rows] = np.where(have, np.take_along_axis(ids, order, 0), NO_HIT)
        dist[:rows] = np.where(have, np.take_along_axis(dm, order, 0), INF)
        return {"count": count, "prim": np.ascontiguousarray(prim.T), "dist": np.ascontiguousarray(dist.T)}


def assert_equal(got, want, what=""):
    """Every field of `got` equals the specification bit for bit."""
    for f, a in got.items():
        w = want[f]
        assert a.shape == w.shape and a.dtype == w.dtype, (what, f, a.shape, w.shape, a.dtype, w.dtype)
        same = a.view(np.uint32) == w.view(np.uint32)
        if not same.all():
            bad = np.argwhere(~same)
            i = tuple(bad[0])
            raise AssertionError(f"{what}: {f}: {len(bad)} of {a.size} differ; first at {i}: got {a[i]!r}, want {w[i]!r}")
