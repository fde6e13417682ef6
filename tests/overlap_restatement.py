"""An independent numpy statement of the triangle overlap query's definition (webgputracer_amd/csrc/
wgt_overlap.h), written from the text, not from the C++.  TEST INFRASTRUCTURE ONLY.

Every array has the dtype asked for and every operation is one numpy ufunc on arrays of that dtype, so with
float32 each +, -, * rounds once, in the order written, and nothing is fused: what the definition demands.
With float64 the same formulas are the comparison the float32 decisions are judged against, and `margins`
says how far each of a pair's segment tests is from flipping.
"""
import numpy as np

f32 = np.float32
NO_HIT = np.uint32(0xFFFFFFFF)
COORD_LIMIT = 2.0 ** 40
EDGE_LIMIT = 2.0 ** 30


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def seg_terms(o, d, w0, f1, f2):
    """(a, U', V', T') of the segment o + t d against the triangle (w0, f1, f2): the determinant's magnitude
    and the three numerators with its sign taken out."""
    p = cross(d, f2)
    det = dot(f1, p)
    tv = o - w0
    U = dot(tv, p)
    q = cross(tv, f1)
    V = dot(d, q)
    T = dot(f2, q)
    neg = det < 0
    return np.where(neg, -det, det), np.where(neg, -U, U), np.where(neg, -V, V), np.where(neg, -T, T)


def seg_crosses(o, d, w0, f1, f2):
    a, U, V, T = seg_terms(o, d, w0, f1, f2)
    return (a > 0) & (U >= 0) & (V >= 0) & (U + V <= a) & (T >= 0) & (T <= a)


def tri_box(v0, e1, e2):
    """The padded box of a record: bounds of v0, v0 + e1, v0 + e2, pad = ((hi - lo) 1e-4 + (|lo| + |hi|) 1e-5) + 1e-6."""
    dt = v0.dtype.type
    b, d = v0 + e1, v0 + e2
    mn = np.where(v0 < b, v0, b)
    mn = np.where(mn < d, mn, d)
    mx = np.where(v0 > b, v0, b)
    mx = np.where(mx > d, mx, d)
    pad = ((mx - mn) * dt(f32(1e-4)) + (np.abs(mn) + np.abs(mx)) * dt(f32(1e-5))) + dt(f32(1e-6))
    return mn - pad, mx + pad


def query_box(a0, a1, a2):
    mn = np.where(a0 < a1, a0, a1)
    mn = np.where(mn < a2, mn, a2)
    mx = np.where(a0 > a1, a0, a1)
    mx = np.where(mx > a2, mx, a2)
    return mn, mx


def box_clause(a0, a1, a2, lo, hi):
    qlo, qhi = query_box(a0, a1, a2)
    return ((qlo <= hi) & (qhi >= lo)).all(-1)


def six_segments(a0, a1, a2, v0, e1, e2):
    """The six (origin, direction, triangle) of the definition, in its order."""
    g1, g2 = a1 - a0, a2 - a0
    return ((a0, a1 - a0, v0, e1, e2), (a1, a2 - a1, v0, e1, e2), (a2, a0 - a2, v0, e1, e2),
            (v0, e1, a0, g1, g2), (v0, e2, a0, g1, g2), (v0 + e1, e2 - e1, a0, g1, g2))


def tri_overlap(A, v0, e1, e2, dtype=f32):
    """A (..., 3, 3) corners against records (..., 3), broadcast: the decision in `dtype`."""
    with np.errstate(all="ignore"):
        A, v0, e1, e2 = (np.asarray(x, dtype) for x in (A, v0, e1, e2))
        a0, a1, a2 = A[..., 0, :], A[..., 1, :], A[..., 2, :]
        lo, hi = tri_box(v0, e1, e2)
        yes = np.zeros(np.broadcast(a0[..., 0], v0[..., 0]).shape, bool)
        for s in six_segments(a0, a1, a2, v0, e1, e2):
            yes |= seg_crosses(*s)
        return box_clause(a0, a1, a2, lo, hi) & yes


def margins(A, v0, e1, e2):
    """In float64, per pair: the smallest over the six segment tests of
    min(|U'|, |V'|, |a - (U' + V')|, |T'|, |a - T'|, a) / max(a, 1e-3 max|d| max|f1| max|f2|)."""
    A, v0, e1, e2 = (np.asarray(x, np.float64) for x in (A, v0, e1, e2))
    a0, a1, a2 = A[..., 0, :], A[..., 1, :], A[..., 2, :]
    worst = None
    for o, d, w0, f1, f2 in six_segments(a0, a1, a2, v0, e1, e2):
        a, U, V, T = seg_terms(o, d, w0, f1, f2)
        num = np.minimum.reduce([np.abs(U), np.abs(V), np.abs(a - (U + V)), np.abs(T), np.abs(a - T), a])
        den = np.maximum(a, 1e-3 * np.abs(d).max(-1) * np.abs(f1).max(-1) * np.abs(f2).max(-1))
        with np.errstate(invalid="ignore"):  # a zero-length edge: 0 / 0, a NaN, which is below no bound and above none
            m = num / den
        worst = m if worst is None else np.minimum(worst, m)
    return worst


def query_ok(Q):
    """(n, 3, 3) float32 corners -> valid: nine coordinates within 2^40, the three edges' components within 2^30."""
    with np.errstate(all="ignore"):
        Q = np.asarray(Q, f32)
        a0, a1, a2 = Q[:, 0], Q[:, 1], Q[:, 2]
        ok = (np.abs(Q) <= f32(COORD_LIMIT)).all((1, 2))
        for e in (a1 - a0, a2 - a0, a2 - a1):
            ok &= (np.abs(e) <= f32(EDGE_LIMIT)).all(1)
        return ok


def overlap(T, Q, k, first_prim=0):
    """The whole answer in float32: hit (n,) bool, count (n,) uint32, prim (n, k) uint32 for records T (v0, e1,
    e2 fields) and queries Q (n, 3, 3)."""
    Q = np.asarray(Q, f32).reshape(-1, 3, 3)
    v0, e1, e2 = (np.ascontiguousarray(T[f][:, :3], f32) for f in ("v0", "e1", "e2"))
    n = len(Q)
    ok = query_ok(Q)
    count = np.zeros(n, np.uint32)
    prim = np.full((n, k), NO_HIT, np.uint32)
    for i in range(n):
        if not ok[i] or len(v0) == 0:
            continue
        S = np.flatnonzero(tri_overlap(Q[i], v0, e1, e2))  # ascending ids
        count[i] = len(S)
        m = min(len(S), k)
        prim[i, :m] = first_prim + S[:m]
    return {"hit": count > 0, "count": count, "prim": prim}
