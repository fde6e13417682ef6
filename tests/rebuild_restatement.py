"""A numpy statement of the rebuild's tree.  TEST INFRASTRUCTURE ONLY.

Keys, order, splits, breadth-first refs, leaf order, stack need and depth of the LBVH that
wgt_rebuild_triangles makes and wgt_bvh_build_morton specifies, written independently of the C++:
Python integers for the codes, a first-in-first-out queue for the numbering.  Boxes and compact
codes are not restated here: tests/refit_cases.py states them for any topology.
"""
import collections

import numpy as np

import refit_cases as rc

f32 = np.float32
BITS = 21
LEVELS = 10  # BVH4 levels: 20 binary levels


def max_tris(L):
    return L * 4 ** LEVELS


def centres(tris):
    lo, hi = rc.tri_boxes(tris)
    c = f32(0.5) * lo + f32(0.5) * hi
    assert c.dtype == f32
    return c


def cells(tris):
    """(n, 3) cell of each centre between the centres' bounds, per axis, in float64."""
    c = centres(tris).astype(np.float64)
    cmin, cmax = c.min(0), c.max(0)
    q = np.zeros(c.shape, np.int64)
    for a in range(3):
        d = cmax[a] - cmin[a]
        if d > 0:
            q[:, a] = np.minimum(2 ** BITS - 1, np.floor((c[:, a] - cmin[a]) / d * 2097152.0).astype(np.int64))
    return q


def codes(tris):
    """Python ints: bit k of x at 3k + 2, of y at 3k + 1, of z at 3k."""
    out = []
    for qx, qy, qz in cells(tris).tolist():
        v = 0
        for k in range(BITS):
            v |= ((qx >> k) & 1) << (3 * k + 2) | ((qy >> k) & 1) << (3 * k + 1) | ((qz >> k) & 1) << (3 * k)
        out.append(v)
    return out


def leaf_order(tris):
    """Original indices ascending by (code, index), and the sorted codes."""
    key = codes(tris)
    order = sorted(range(len(key)), key=lambda i: (key[i], i))
    return np.array(order, np.uint32), [key[i] for i in order]


def split(code, b, e, r, L):
    if code[b] != code[e - 1]:
        h = (code[b] ^ code[e - 1]).bit_length() - 1
        p = next(i for i in range(b, e) if (code[i] >> h) & 1)
        if max(p - b, e - p) <= L * 2 ** (r - 1):
            return p
    return b + (e - b + 1) // 2


def slots_of(code, b, e, r, L):
    p = split(code, b, e, r, L)
    parts = []
    for lo, hi in ((b, p), (p, e)):
        if hi - lo > L:
            m = split(code, lo, hi, r - 1, L)
            parts += [(lo, m), (m, hi)]
        else:
            parts.append((lo, hi))
    return parts


def leaf_ref(first, count):
    return ~(first << 3 | (count - 1))


def topology(code, L):
    """(refs (n_nodes, 4) int32 with empty slots holding slot 0's ref, live slots per node, level per
    node, stack_need, depth, leaves as (first, count))."""
    n = len(code)
    if n <= L:
        r = leaf_ref(0, n)
        return np.array([[r] * 4], np.int32), [1], [0], 1, 1, [(0, n)]
    refs, live, level, leaves = [], [], [], []
    stack_need = 0
    queue = collections.deque([(0, n, 2 * LEVELS, 0, 0)])
    made = 1  # nodes numbered so far: the queue's order is the numbering
    while queue:
        b, e, r, path, lvl = queue.popleft()
        parts = slots_of(code, b, e, r, L)
        path += len(parts) - 1
        stack_need = max(stack_need, path)
        row = []
        for lo, hi in parts:
            if hi - lo <= L:
                row.append(leaf_ref(lo, hi - lo))
                leaves.append((lo, hi - lo))
            else:
                assert r >= 4, "a node below the depth budget"
                row.append(made)
                made += 1
                queue.append((lo, hi, r - 2, path, lvl + 1))
        live.append(len(row))
        level.append(lvl)
        refs.append(row + [row[0]] * (4 - len(row)))
    return np.array(refs, np.int32), live, level, stack_need, max(level) + 1, leaves


def tree(tris, L):
    order, code = leaf_order(tris)
    return (order,) + topology(code, L)
