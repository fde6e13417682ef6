"""Inputs of the triangle overlap tests (tests/test_overlap_restatement.py on the CPU, tests/test_gpu_overlap.py
on the GPU), built once per process.  TEST INFRASTRUCTURE ONLY.

Query triangles are (n, 3, 3) float32 corners, drawn from seeded generators in float64 and rounded once.
"""
import functools

import numpy as np

import nearest_cases as nc

f32 = np.float32
N_MAIN = 512
KS = (0, 1, 8, 32)


def corners(tris):
    """(n, 3, 3) corners of records, each corner rounded once as the record's box rounds it."""
    v0, e1, e2 = (tris[f][:, :3].astype(f32) for f in ("v0", "e1", "e2"))
    return np.stack([v0, v0 + e1, v0 + e2], 1)


def _rotations(rng, n):
    """n rotation matrices: a uniform random axis and a uniform random angle (Rodrigues)."""
    axis = rng.normal(size=(n, 3))
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    K = np.zeros((n, 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0] = -axis[:, 2], axis[:, 1], axis[:, 2]
    K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -axis[:, 0], -axis[:, 1], axis[:, 0]
    return np.eye(3) + np.sin(ang)[:, None, None] * K + (1.0 - np.cos(ang))[:, None, None] * (K @ K)


def from_own_triangles(tris, n, seed):
    """n queries made from the mesh's own triangles (those with an area): each rotated by a seeded random
    angle about its centroid and shifted by up to one edge length."""
    rng = np.random.default_rng(seed)
    C = corners(tris).astype(np.float64)
    area = np.linalg.norm(np.cross(C[:, 1] - C[:, 0], C[:, 2] - C[:, 0]), axis=1)
    live = np.flatnonzero(area > 0.0)
    C = C[live[rng.integers(0, len(live), n)]]
    mid = C.mean(1, keepdims=True)
    edge = np.linalg.norm(C[:, 1] - C[:, 0], axis=1)
    shift = rng.uniform(-1.0, 1.0, (n, 3)) / np.sqrt(3.0) * edge[:, None]
    return (np.einsum("nij,nkj->nki", _rotations(rng, n), C - mid) + mid + shift[:, None, :]).astype(f32)


@functools.lru_cache(maxsize=None)
def bunny_queries(n=N_MAIN, seed=17):
    """The main set: 512 queries from bunny2000's own triangles."""
    return from_own_triangles(nc.bunny(), n, seed)


# ------------------------------------------------------------------ known answers by hand
UNIT = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], f32)  # the resident triangle: v0 = 0, e1 = x, e2 = y


@functools.lru_cache(maxsize=None)
def unit_tris():
    import webgputracer_amd as wgt

    return wgt.make_triangles(UNIT)


def unit_box_hi_x():
    """hi.x of the unit triangle's padded box, op by op in float32: 1 + ((1 - 0) 1e-4 + (0 + 1) 1e-5) + 1e-6."""
    pad = (f32(1.0) * f32(1e-4) + f32(1.0) * f32(1e-5)) + f32(1e-6)
    return f32(1.0) + pad


def known_answers():
    """name -> (query (3, 3), count against the unit triangle)."""
    hx = unit_box_hi_x()
    above = np.nextafter(hx, f32(np.inf))
    return {
        # an edge of the query goes through the face
        "piercing": ([[0.25, 0.25, -1], [0.25, 0.25, 1], [2, 2, 1]], 1),
        # the boxes overlap, the nearest edge passes at (0.9, 0.9), outside the hypotenuse
        "disjoint, boxes overlap": ([[0.9, 0.9, -1], [0.9, 0.9, 1], [2, 2, 0]], 0),
        # in the resident triangle's plane, inside it: all six determinants are zero
        "coplanar, overlapping": ([[0.1, 0.1, 0], [0.8, 0.1, 0], [0.1, 0.8, 0]], 0),
        # the query's plane x = 0.25 cuts the resident triangle, the query's edges all pass outside it: the
        # resident edge along x goes through the query's face.  Three rays along the query's edges miss this.
        "resident edge through the query's face": ([[0.25, -5, -5], [0.25, 5, -5], [0.25, 0, 5]], 1),
        # an edge of the query passes exactly through the vertex (1, 0, 0), a corner of the resident triangle's
        # unpadded box, and the boxes share nothing else: touching counts, and the pad keeps the box clause true
        "crossing at a box corner": ([[1, 0, -1], [1, 0, 1], [3, -2, 0]], 1),
        # the same edge moved to the first float past the padded box: the box clause says no
        "box misses by one ulp": ([[above, 0, -1], [above, 0, 1], [3, -2, 0]], 0),
        # ... and at the padded box's own plane the box clause holds and the segments decide: no
        "box touches the pad": ([[hx, 0, -1], [hx, 0, 1], [3, -2, 0]], 0),
    }


def invalid_queries():
    """name -> query (3, 3): each would pierce the unit triangle if it were valid."""
    p = [[0.25, 0.25, -1], [0.25, 0.25, 1], [2, 2, 1]]
    q = {}
    for name, (corner, axis, v) in {"NaN": (2, 0, np.nan), "inf": (2, 1, np.inf), "-inf": (0, 2, -np.inf),
                                    "2^41": (2, 0, 2.0 ** 41)}.items():
        a = np.array(p, f32)
        a[corner, axis] = v
        q[name] = a
    # coordinates within 2^40, the first edge's z component 2^31
    q["edge 2^31"] = np.array([[0.25, 0.25, -2.0 ** 30], [0.25, 0.25, 2.0 ** 30], [2, 2, 1]], f32)
    return q


def longest_valid_query():
    """The edge at the limit itself: components of exactly 2^30 are valid, and it pierces."""
    return np.array([[0.25, 0.25, -2.0 ** 29], [0.25, 0.25, 2.0 ** 29], [2, 2, 1]], f32)


def interleaved(Q):
    """Valid queries with the invalid ones between them, one every fourth lane, and which are which."""
    Q = np.array(Q, f32)
    odd = np.zeros(len(Q), bool)
    for m, j in enumerate(range(0, len(Q), 4)):  # the query keeps its place in the mesh, one coordinate is spoiled
        if m % 5 == 0:
            Q[j, 2, 0] = np.nan
        elif m % 5 == 1:
            Q[j, 2, 1] = np.inf
        elif m % 5 == 2:
            Q[j, 0, 2] = -np.inf
        elif m % 5 == 3:
            Q[j, 1, 0] = 2.0 ** 41
        else:  # coordinates within 2^40, an edge component of 2^31
            Q[j, 0, 2], Q[j, 1, 2] = -2.0 ** 30, 2.0 ** 30
        odd[j] = True
    return Q, odd


def zero_area_queries(tris, n=64, seed=23):
    """Points (three equal corners) and collinear triples at the mesh's own vertices and edges."""
    rng = np.random.default_rng(seed)
    C = corners(tris)[rng.integers(0, len(tris), n)]
    Q = C.copy()
    Q[0::2, 1] = Q[0::2, 0]
    Q[0::2, 2] = Q[0::2, 0]                                  # a point at a vertex
    Q[1::2, 2] = Q[1::2, 0] + f32(2.0) * (Q[1::2, 1] - Q[1::2, 0])  # collinear, along an edge and beyond
    return Q


def through_copies64():
    """Queries that pierce copies64's one triangle, and one that passes it by."""
    c = corners(nc.copies64())[0].astype(np.float64)
    mid, nrm = c.mean(0), np.cross(c[1] - c[0], c[2] - c[0])
    nrm /= np.linalg.norm(nrm)
    Q = [[mid - 30 * nrm, mid + 30 * nrm, mid + 500 * (c[1] - c[0])]]
    Q.append([c[0] * 0.5 + c[1] * 0.5 - 7 * nrm, c[2] + 9 * nrm, mid + 40 * nrm + 300 * (c[2] - c[0])])
    Q.append([mid + 100 * nrm, mid + 130 * nrm, mid + 100 * nrm + (c[1] - c[0])])
    return np.array(Q, f32)


# ------------------------------------------------------------------ the float64 comparison's pairs
SIZES = (0.05, 0.3, 1.0)
N_PAIRS = 100_000


@functools.lru_cache(maxsize=None)
def pair_sets():
    """name -> (A (n, 3, 3) corners, (v0, e1, e2) records), float32.  One generator, seed 1, draws the three
    sizes in turn: the centre uniform in the unit cube, corners = centre + s (U - 0.5), the second triangle's
    centre offset by 0.5 s (U - 0.5); then the s = 0.3 set again times 2^-12 and 2^20 (exact)."""
    rng = np.random.default_rng(1)
    sets = {}
    for s in SIZES:
        centre = rng.uniform(0.0, 1.0, (N_PAIRS, 1, 3))
        A = (centre + s * (rng.uniform(0.0, 1.0, (N_PAIRS, 3, 3)) - 0.5)).astype(f32)
        centre_b = centre + 0.5 * s * (rng.uniform(0.0, 1.0, (N_PAIRS, 1, 3)) - 0.5)
        B = (centre_b + s * (rng.uniform(0.0, 1.0, (N_PAIRS, 3, 3)) - 0.5)).astype(f32)
        sets[f"s = {s:g}"] = (A, (B[:, 0].copy(), B[:, 1] - B[:, 0], B[:, 2] - B[:, 0]))
    A, rec = sets["s = 0.3"]
    for scale in nc.SCALES:
        sets[f"s = 0.3 x {scale:g}"] = (A * f32(scale), tuple(r * f32(scale) for r in rec))
    return sets
