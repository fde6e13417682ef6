"""The closest-point query's definition (webgputracer_amd/csrc/wgt_nearest.h) a third
time, in numpy: vectorised over points x triangles, float32 at every operation, in the header's
order.  TEST INFRASTRUCTURE ONLY.

    nearest_on_tri(p, v0, e1, e2) -> d2, v, w, q, region      (broadcasting over leading axes)
    nearest_points(tris, points, max_dist=None, first_prim=0) -> dict(prim, dist, pos, uv, region)
"""
import numpy as np

f32 = np.float32
NO_HIT = np.uint32(0xFFFFFFFF)
VERTEX, EDGE, FACE = 0, 1, 2


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def nearest_on_tri(p, v0, e1, e2):
    """Ericson 5.1.5 with a = v0, ab = e1, ac = e2; the first test that holds names the region."""
    p, v0, e1, e2 = (np.asarray(a, f32) for a in (p, v0, e1, e2))
    with np.errstate(all="ignore"):
        ap = p - v0
        d1, d2 = _dot(e1, ap), _dot(e2, ap)
        bp = ap - e1
        d3, d4 = _dot(e1, bp), _dot(e2, bp)
        cp = ap - e2
        d5, d6 = _dot(e1, cp), _dot(e2, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        tests = [(d1 <= 0) & (d2 <= 0),
                 (d3 >= 0) & (d4 <= d3),
                 (vc <= 0) & (d1 >= 0) & (d3 <= 0),
                 (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0),
                 (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        k = np.full(d1.shape, 7, np.int32)
        for i in range(5, -1, -1):
            k = np.where(tests[i], np.int32(i + 1), k)
        zero, one = f32(0), f32(1)
        q_ab = d1 / (d1 - d3)
        q_ac = d2 / (d2 - d6)
        q_bc = e43 / (e43 + e56)
        s = (va + vb) + vc
        fv, fw = vb / s, vc / s
        v = np.select([k == 1, k == 2, k == 3, k == 4, k == 5, k == 6], [zero, one, q_ab, zero, zero, one - q_bc], fv)
        w = np.select([k == 1, k == 2, k == 3, k == 4, k == 5, k == 6], [zero, zero, zero, one, q_ac, q_bc], fw)
        v, w = v.astype(f32), w.astype(f32)
        q = (v0 + v[..., None] * e1) + w[..., None] * e2
        dl = p - q
        dd = _dot(dl, dl)
    region = np.where((k == 1) | (k == 2) | (k == 4), VERTEX, np.where(k == 7, FACE, EDGE))
    assert dd.dtype == f32 and q.dtype == f32
    return dd, v, w, q, region


def nearest_points(tris, points, max_dist=None, first_prim=0, chunk=256):
    """The minimum of (d2, index) over tris (records with v0, e1, e2 fields) per point, the radius and
    the miss record; `region` is the winner's (VERTEX, EDGE, FACE; -1 for a miss)."""
    points = np.asarray(points, f32).reshape(-1, 3)
    n, nt = len(points), len(tris)
    lim = np.full(n, np.inf, f32) if max_dist is None else np.broadcast_to(np.asarray(max_dist, f32), (n,))
    out = {"prim": np.full(n, NO_HIT, np.uint32), "dist": np.full(n, np.inf, f32), "pos": np.zeros((n, 3), f32),
           "uv": np.zeros((n, 2), f32), "region": np.full(n, -1, np.int64)}
    if nt == 0:
        return out
    v0, e1, e2 = (np.ascontiguousarray(tris[k][:, :3], f32)[None] for k in ("v0", "e1", "e2"))
    for a in range(0, n, chunk):
        p = points[a:a + chunk, None, :]
        dd, v, w, q, region = nearest_on_tri(p, v0, e1, e2)
        ok = dd < f32(np.inf)                      # not NaN, not infinite
        key = np.where(ok, dd, f32(np.inf))
        j = np.argmin(key, axis=1)                 # the first minimum: the lowest index among ties
        r = np.arange(len(j))
        any_ok = ok[r, j]
        with np.errstate(invalid="ignore"):
            dist = np.sqrt(dd[r, j])
            hit = any_ok & (dist < lim[a:a + chunk])
        sl = slice(a, a + len(j))
        out["prim"][sl] = np.where(hit, np.uint32(first_prim) + j.astype(np.uint32), NO_HIT)
        out["dist"][sl] = np.where(hit, dist, f32(np.inf))
        out["pos"][sl] = np.where(hit[:, None], q[r, j], f32(0))
        out["uv"][sl] = np.where(hit[:, None], np.stack([v[r, j], w[r, j]], 1), f32(0))
        out["region"][sl] = np.where(hit, region[r, j], -1)
    return out
