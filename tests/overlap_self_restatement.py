"""An independent numpy statement of the self-intersection query's definition (webgputracer_amd/csrc/
wgt_overlap_self.h), written from the text, not from the C++.  TEST INFRASTRUCTURE ONLY.

It stands on overlap_restatement's statement of the segment test and of the padded box, and adds what is the
self query's own: the corners rebuilt from the record, adjacency by labels, the box clause on two padded boxes
and the roles by id.  Every array has the dtype asked for and every operation is one numpy ufunc on arrays of
that dtype, so with float32 each +, -, * rounds once, in the order written, and nothing is fused.
"""
import numpy as np

import overlap_restatement as rs

f32 = np.float32
NO_HIT = np.uint32(0xFFFFFFFF)


def record(T, dtype=f32):
    return tuple(np.ascontiguousarray(T[f][:, :3], f32).astype(dtype) for f in ("v0", "e1", "e2"))


def adjacent(labels, n):
    """(n, n) bool: some label of s equals some label of t; all False without labels."""
    if labels is None:
        return np.zeros((n, n), bool)
    L = np.asarray(labels, np.uint32).reshape(n, 3)
    return (L[:, None, :, None] == L[None, :, None, :]).any((2, 3))


def segments(T, dtype=f32):
    """(n, n) bool D[i, j]: one of the six segments crosses with corners(i) as the query and record j resident."""
    v0, e1, e2 = record(T, dtype)
    with np.errstate(all="ignore"):
        a0, a1, a2 = v0[:, None, :], (v0 + e1)[:, None, :], (v0 + e2)[:, None, :]
        yes = np.zeros((len(v0), len(v0)), bool)
        for s in rs.six_segments(a0, a1, a2, v0[None], e1[None], e2[None]):
            yes |= rs.seg_crosses(*s)
    return yes


def boxes(T, dtype=f32):
    """(n, n) bool: the two padded boxes overlap on every axis, equality included."""
    with np.errstate(all="ignore"):
        lo, hi = rs.tri_box(*record(T, dtype))
        return ((lo[:, None, :] <= hi[None, :, :]) & (hi[:, None, :] >= lo[None, :, :])).all(-1)


def matrix(T, labels=None, dtype=f32):
    """(n, n) bool M[s, t] = self_overlap(s, t): the segment clause is taken at (min(s, t), max(s, t))."""
    n = len(T)
    D = np.triu(segments(T, dtype), 1)
    return ~np.eye(n, dtype=bool) & ~adjacent(labels, n) & boxes(T, dtype) & (D | D.T)


def overlap_self(T, labels, k, first_prim=0):
    """The whole answer in float32: hit (n,) bool, count (n,) uint32, prim (n, k) uint32."""
    M = matrix(T, labels)
    n = len(T)
    count = M.sum(1).astype(np.uint32)
    prim = np.full((n, k), NO_HIT, np.uint32)
    for s in range(n):
        S = np.flatnonzero(M[s])[:k]  # ascending ids
        prim[s, :len(S)] = first_prim + S
    return {"hit": count > 0, "count": count, "prim": prim}


def pairs(M):
    """The unique pairs (s, t), s < t, of a membership matrix, in lexicographic order."""
    s, t = np.nonzero(np.triu(M, 1))
    return np.stack([s, t], 1).astype(np.int64)
