"""A numpy float32 restatement of the triangle step of k_render_ps (wgt_trav_ps.h tri_step), written
twice: as two whole triangle tests followed by a merge (the form the step had), and as both
Moller-Trumbore bodies followed by one tail that takes a lane's passing slots lowest first (the
form it has).  tests/test_tri_tail_restatement.py runs both on random record pairs: the argument
of DESIGN.md §4.2 item 34 as executable text.  TEST INFRASTRUCTURE ONLY.

Vectorised over lanes; every operation is one fp32 operation in the kernel's order (no fused
multiply-add except the slab's, as in wgt_geom.h)."""
import numpy as np

f32 = np.float32
U32 = np.uint32
kRayMin = f32(0.001)
kRayMax = f32(1e20)
NO_HIT = U32(0xFFFFFFFF)
DET_MIN = f32(1e-12)


def dot(a, b): return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
def cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
def sub(a, b): return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def fma(a, b, c):
    """One rounding of a * b + c: exact in float64 for fp32 operands' product, then the sum rounds
    once to fp32 except where float64's own rounding of the sum falls on an fp32 tie (not within
    reach of these tests' operands often enough to matter to a comparison of two forms that both
    call this function)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def mt_test(o, d, v0, e1, e2):
    """wgt_geom.h mt_test: (pass, t).  The early-outs are masks here: a lane that leaves early
    computes values nobody reads."""
    with np.errstate(all="ignore"):
        pvec = cross(d, e2)
        det = dot(e1, pvec)
        det_ok = ~(np.abs(det) < DET_MIN)
        inv_det = f32(1.0) / det
        tvec = sub(o, v0)
        u = dot(tvec, pvec) * inv_det
        ok = det_ok & ~(u < 0) & ~(u > 1)
        qvec = cross(tvec, e1)
        v = dot(d, qvec) * inv_det
        ok &= ~(v < 0) & ~(u + v > 1)
        t = dot(e2, qvec) * inv_det
        ok &= ~(t < kRayMin) & ~(kRayMax < t)
    return ok, t


def slab(ot, inv, lo, hi):
    t0 = [fma(lo[k], inv[k], ot[k]) for k in range(3)]
    t1 = [fma(hi[k], inv[k], ot[k]) for k in range(3)]
    near = np.maximum(np.maximum(np.minimum(t0[0], t1[0]), np.minimum(t0[1], t1[1])), np.minimum(t0[2], t1[2]))
    far = np.minimum(np.minimum(np.maximum(t0[0], t1[0]), np.maximum(t0[1], t1[1])), np.maximum(t0[2], t1[2]))
    return near, far


def med3(a, b, c):
    return np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), c))


def tri_tail(lo, hi, ot, inv, bt, bi, t, idx):
    """wgt_trav.h tri_tail: (accepted, clamped t)."""
    bn, bf = slab(ot, inv, lo, hi)
    tt = med3(t, bn, bf)
    return (bn <= bf) & (tt >= kRayMin) & ((tt < bt) | ((tt == bt) & (idx < bi))), tt


def tri_box(v0, e1, e2):
    """wgt_geom.h tri_box per axis."""
    lo, hi = [], []
    for c in range(3):
        a = v0[c]
        b = a + e1[c]
        d = a + e2[c]
        mn = np.minimum(np.minimum(a, b), d)
        mx = np.maximum(np.maximum(a, b), d)
        pad = ((mx - mn) * f32(1e-4) + (np.abs(mn) + np.abs(mx)) * f32(1e-5)) + f32(1e-6)
        lo.append(mn - pad)
        hi.append(mx + pad)
    return tuple(lo), tuple(hi)


def step_whole_tests_then_merge(o, d, ot, inv, rec, live1, bt, bi):
    """Two whole tests against the same (bt, bi), slot 1 ignored where it is dead, then the merge:
    slot 0's hit is taken, slot 1's replaces it when (t, index) is strictly below."""
    tt, hit = [], []
    for r in rec:
        ok, t = mt_test(o, d, r["v0"], r["e1"], r["e2"])
        acc, tc = tri_tail(r["lo"], r["hi"], ot, inv, bt, bi, t, r["idx"])
        hit.append(ok & acc)
        tt.append(tc)
    hit[1] &= live1
    bt = np.where(hit[0], tt[0], bt)
    bi = np.where(hit[0], rec[0]["idx"], bi)
    m = hit[1] & ((tt[1] < bt) | ((tt[1] == bt) & (rec[1]["idx"] < bi)))
    return np.where(m, tt[1], bt), np.where(m, rec[1]["idx"], bi)


def step_one_tail(o, d, ot, inv, rec, live1, bt, bi):
    """Both Moller-Trumbore bodies, then one tail run while a lane has a passing slot left, the
    lowest first, each against the bound as it then stands.  Returns the rounds run too."""
    ok0, t0 = mt_test(o, d, rec[0]["v0"], rec[0]["e1"], rec[0]["e2"])
    ok1, t1 = mt_test(o, d, rec[1]["v0"], rec[1]["e1"], rec[1]["e2"])
    pas = ok0.astype(U32) | ((ok1 & live1).astype(U32) << U32(1))
    bt, bi = bt.copy(), bi.copy()
    rounds = 0
    while pas.any():
        rounds += 1
        run = pas != 0
        s0 = (pas & U32(1)) != 0  # slot 0 is the lowest set
        lo = tuple(np.where(s0, rec[0]["lo"][k], rec[1]["lo"][k]) for k in range(3))
        hi = tuple(np.where(s0, rec[0]["hi"][k], rec[1]["hi"][k]) for k in range(3))
        t = np.where(s0, t0, t1)
        idx = np.where(s0, rec[0]["idx"], rec[1]["idx"])
        pas = pas & (pas - U32(1))
        acc, tc = tri_tail(lo, hi, ot, inv, bt, bi, t, idx)
        acc &= run
        bt = np.where(acc, tc, bt)
        bi = np.where(acc, idx, bi)
    return bt, bi, rounds
