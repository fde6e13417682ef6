"""Inputs of the closest-point tests (tests/test_nearest_restatement.py on the CPU, tests/test_gpu_nearest.py
on the GPU), built once per process.  TEST INFRASTRUCTURE ONLY.

The mesh is the 2,000-triangle bunny stand-in (a closed blob of radius about 120 in the middle of the
Cornell box); the point sets are drawn from seeded generators, in float64, and rounded once.
"""
import functools

import numpy as np

f32 = np.float32
INF = f32(np.inf)
N_MAIN = 4000


def _wgt():
    import webgputracer_amd

    return webgputracer_amd


# ------------------------------------------------------------------ the known-answer table
KAT_TRI = np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], f32)  # v0 = 0, e1 = x, e2 = y
# point, (v, w), d2: one point per region of the right triangle; every value is exact in float32
KAT = [
    ((-1.0, -2.0, 0.5), (0.0, 0.0), 5.25),     # vertex a
    ((3.0, -1.0, 0.0), (1.0, 0.0), 5.0),       # vertex b
    ((-0.5, 2.0, 1.0), (0.0, 1.0), 2.25),      # vertex c
    ((0.25, -2.0, 0.0), (0.25, 0.0), 4.0),     # edge ab: the foot (0.25, 0, 0)
    ((-3.0, 0.75, 4.0), (0.0, 0.75), 25.0),    # edge ac: the foot (0, 0.75, 0)
    ((1.5, 1.5, 0.0), (0.5, 0.5), 2.0),        # edge bc: the foot (0.5, 0.5, 0)
    ((0.25, 0.5, -3.0), (0.25, 0.5), 9.0),     # the face: the projection (0.25, 0.5, 0)
]
KAT_REGION = [0, 0, 0, 1, 1, 1, 2]  # nearest_restatement.VERTEX, EDGE, FACE


@functools.lru_cache(maxsize=None)
def kat_tris():
    return _wgt().make_triangles(KAT_TRI)


# ------------------------------------------------------------------ the mesh and the two main point sets
@functools.lru_cache(maxsize=None)
def bunny_scene():
    """(lights, quads, spheres, tris) of the Cornell walls plus bunny2000."""
    return _wgt().mesh_scene("bunny", 2000)


def bunny():
    return bunny_scene()[3]


def centroids(tris, idx):
    return (tris["v0"][idx, :3].astype(np.float64)
            + (tris["e1"][idx, :3].astype(np.float64) + tris["e2"][idx, :3].astype(np.float64)) / 3.0)


def unit_normals(tris, idx):
    n = np.cross(tris["e1"][idx, :3].astype(np.float64), tris["e2"][idx, :3].astype(np.float64))
    return n / np.linalg.norm(n, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def box_points(n=N_MAIN, seed=0):
    """Uniform in [5, 550]^3: mostly far from the mesh, every region of a triangle answers."""
    return np.random.default_rng(seed).uniform(5.0, 550.0, (n, 3)).astype(f32)


@functools.lru_cache(maxsize=None)
def surface_points(n=N_MAIN, seed=1):
    """Within +-2 units of the surface: random centroids moved along their face normal.  The stand-in's
    zero-area triangles (its poles: 90 of 1,980) have no normal and are not drawn."""
    rng = np.random.default_rng(seed)
    T = bunny()
    area = np.linalg.norm(np.cross(T["e1"][:, :3].astype(np.float64), T["e2"][:, :3].astype(np.float64)), axis=1)
    idx = np.flatnonzero(area > 0.0)[rng.integers(0, np.count_nonzero(area > 0.0), n)]
    return (centroids(T, idx) + rng.uniform(-2.0, 2.0, (n, 1)) * unit_normals(T, idx)).astype(f32)


@functools.lru_cache(maxsize=None)
def far_points(back, n=600, seed=2):
    """About `back` units from random centroids, in random directions."""
    rng = np.random.default_rng(seed)
    T = bunny()
    idx = rng.integers(0, len(T), n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (centroids(T, idx) + back * d).astype(f32)


FAR = (1e3, 1e5, 1e7)


def scaled(tris, s):
    """The records with v0, e1, e2 times s, a power of two (exact)."""
    out = tris.copy()
    for k in ("v0", "e1", "e2"):
        out[k][:, :3] *= f32(s)
    return out


SCALES = (2.0 ** -12, 2.0 ** 20)


# ------------------------------------------------------------------ radii
def radius_sets(D):
    """0.5 D, D, the float above D, 2 D, +inf, 0, -1, NaN per point (D: its distance)."""
    D = np.asarray(D, f32)
    return [f32(0.5) * D, D, np.nextafter(D, INF), f32(2.0) * D, np.full_like(D, INF), np.zeros_like(D),
            np.full_like(D, f32(-1.0)), np.full_like(D, f32(np.nan))]


def around(D):
    """One float below D, D, one float above D."""
    D = np.asarray(D, f32)
    return [np.nextafter(D, f32(0)), D, np.nextafter(D, INF)]


# ------------------------------------------------------------------ ties and degenerates
@functools.lru_cache(maxsize=None)
def copies64():
    """64 exact copies of one triangle."""
    one = np.array([[[200, 200, 200], [260, 210, 190], [215, 270, 230]]], f32)
    return _wgt().make_triangles(np.tile(one, (64, 1, 1)))


@functools.lru_cache(maxsize=None)
def degenerate_mix():
    """adversarial_meshes' `degenerate`: collinear triangles and points among ordinary ones."""
    import adversarial_meshes as am

    return am.small_mesh("degenerate")


@functools.lru_cache(maxsize=None)
def degenerate_only():
    """Nothing but its zero-area triangles (v2 = v1, or all three corners equal)."""
    T = degenerate_mix()
    k = np.arange(len(T))
    return T[(k % 3 == 0) | (k % 7 == 1)].copy()


@functools.lru_cache(maxsize=None)
def bad_points():
    """Points with a NaN or an infinite component, and ordinary ones between them."""
    p = box_points(64, 5).copy()
    p[0::8, 0] = np.nan
    p[1::8, 1] = np.inf
    p[2::8, 2] = -np.inf
    p[3::8] = np.nan
    return p


def small_points(n=512, seed=3):
    return box_points(n, seed)


# ------------------------------------------------------------------ every case, for the CPU comparison
def cpu_cases():
    """name -> (tris, points, max_dist or None): what the spec and the numpy statement are compared on."""
    T = bunny()
    cases = {
        "kat": (kat_tris(), np.array([k[0] for k in KAT], f32), None),
        "box": (T, box_points(), None),
        "surface": (T, surface_points(), None),
        "copies64": (copies64(), small_points(), None),
        "degenerate_mix": (degenerate_mix(), small_points(), None),
        "degenerate_only": (degenerate_only(), small_points(), None),
        "bad_points": (T, bad_points(), None),
        "no_triangles": (T[:0], small_points(64), None),
        "one_triangle": (T[:1], small_points(), None),
    }
    for back in FAR:
        cases[f"far_{back:g}"] = (T, far_points(back), None)
    for s in SCALES:
        cases[f"scale_{s:g}"] = (scaled(T, s), small_points() * f32(s), None)
    return cases
