"""The triangle step's one tail against its two whole tests and a merge, in numpy (no GPU):
tests/tri_tail_restatement.py's two forms must leave the same (bt, bi) bits on 10^5 random record
pairs.  In a tenth of the pairs the two records are the same triangle under two indices (equal t:
the index decides, in either order), and in a tenth the padded box is replaced by a thin one just
beside the hit, so that the clamp moves t (and in some of those the two clamped t tie).  The bound
(bt, bi) the step starts from is kRayMax / no hit, a quad's t (no index), a value among the hits'
t, or exactly one slot's t with an index on either side of that slot's."""
import numpy as np

import tri_tail_restatement as R

f32, U32 = np.float32, np.uint32
N = 100_000


def records(rng, n):
    """Rays from around the camera's distance and pairs of triangles most of which they hit."""
    o = rng.uniform(-300, 300, (3, n)).astype(f32)
    d = rng.normal(size=(3, n)).astype(f32)
    d /= np.sqrt((d * d).sum(0, dtype=f32))
    rec = []
    for _ in range(2):
        t = rng.uniform(50, 900, n).astype(f32)
        p = o + t * d
        # a triangle around p (barycentric weights inside for 80 %, outside for the rest)
        e1 = rng.normal(size=(3, n)).astype(f32) * f32(40)
        e2 = rng.normal(size=(3, n)).astype(f32) * f32(40)
        u = rng.uniform(0.05, 0.45, n).astype(f32)
        v = rng.uniform(0.05, 0.45, n).astype(f32)
        miss = rng.random(n) < 0.2
        u = np.where(miss, u + f32(1.0), u)
        v0 = p - u * e1 - v * e2
        rec.append({"v0": tuple(v0), "e1": tuple(e1), "e2": tuple(e2),
                    "idx": rng.integers(0, 1 << 20, n).astype(U32)})
    # ties: the same triangle under two indices, in either order (and sometimes the same index)
    tie = rng.random(n) < 0.1
    for k in ("v0", "e1", "e2"):
        rec[1][k] = tuple(np.where(tie, a, b) for a, b in zip(rec[0][k], rec[1][k]))
    delta = rng.integers(-2, 3, n)
    rec[1]["idx"] = np.where(tie, (rec[0]["idx"].astype(np.int64) + delta).clip(0, (1 << 20) - 1).astype(U32), rec[1]["idx"])
    for r in rec:
        r["lo"], r["hi"] = R.tri_box(r["v0"], r["e1"], r["e2"])
    # clamped hits: a thin box a little beyond (or before) the hit point along the ray, so that the
    # slab interval lies beside Moller-Trumbore's t and the clamp moves it; for the pairs that are
    # also ties both records get the same box (two clamped t that tie)
    clamp = rng.random(n) < 0.1
    shift = rng.uniform(-3, 3, n).astype(f32)
    for j, r in enumerate(rec):
        ok, t = R.mt_test(tuple(o), tuple(d), r["v0"], r["e1"], r["e2"])
        src = rec[0] if j == 1 else r
        if j == 1:
            _, t_first = R.mt_test(tuple(o), tuple(d), src["v0"], src["e1"], src["e2"])
            t = np.where(tie, t_first, t)
        c = o + (np.where(ok, t, f32(100)) + shift) * d
        r["lo"] = tuple(np.where(clamp, c[k] - f32(0.25), r["lo"][k]) for k in range(3))
        r["hi"] = tuple(np.where(clamp, c[k] + f32(0.25), r["hi"][k]) for k in range(3))
    live1 = rng.random(n) < 0.8
    # a dead slot re-reads the first record
    for k in ("v0", "e1", "e2", "lo", "hi"):
        rec[1][k] = tuple(np.where(live1, b, a) for a, b in zip(rec[0][k], rec[1][k]))
    rec[1]["idx"] = np.where(live1, rec[1]["idx"], rec[0]["idx"])
    return tuple(o), tuple(d), rec, live1, tie, clamp


def bounds(rng, n, o, d, rec, ot, inv):
    """The (bt, bi) a step starts from."""
    kind = rng.integers(0, 5, n)
    bt = np.full(n, R.kRayMax, f32)
    bi = np.full(n, R.NO_HIT, U32)
    _, t0 = R.mt_test(o, d, rec[0]["v0"], rec[0]["e1"], rec[0]["e2"])
    _, c0 = R.tri_tail(rec[0]["lo"], rec[0]["hi"], ot, inv, bt, bi, t0, rec[0]["idx"])
    _, t1 = R.mt_test(o, d, rec[1]["v0"], rec[1]["e1"], rec[1]["e2"])
    _, c1 = R.tri_tail(rec[1]["lo"], rec[1]["hi"], ot, inv, bt, bi, t1, rec[1]["idx"])
    good0 = np.isfinite(c0) & (c0 > 0)
    good1 = np.isfinite(c1) & (c1 > 0)
    quad = rng.uniform(50, 900, n).astype(f32)
    bt = np.where(kind == 1, quad, bt)  # a quad's t: no index
    between = (np.where(good0, c0, quad) + np.where(good1, c1, quad)) * f32(0.5)
    bt = np.where(kind == 2, between, bt)
    bi = np.where(kind == 2, rng.integers(0, 1 << 20, n).astype(U32), bi)
    for k, (c, good, r) in ((3, (c0, good0, rec[0])), (4, (c1, good1, rec[1]))):
        m = (kind == k) & good
        bt = np.where(m, c, bt)  # exactly this slot's t: the index decides
        near = (r["idx"].astype(np.int64) + rng.integers(-1, 2, n)).clip(0, (1 << 20) - 1).astype(U32)
        bi = np.where(m, np.where(rng.random(n) < 0.3, R.NO_HIT, near), bi)
    return bt, bi


def test_one_tail_equals_two_whole_tests_and_a_merge():
    rng = np.random.default_rng(34)
    o, d, rec, live1, tie, clamp = records(rng, N)
    with np.errstate(all="ignore"):
        inv = tuple(f32(1.0) / c for c in d)
        ot = tuple(-(a * b) for a, b in zip(o, inv))
        bt, bi = bounds(rng, N, o, d, rec, ot, inv)
        a_bt, a_bi = R.step_whole_tests_then_merge(o, d, ot, inv, rec, live1, bt, bi)
        b_bt, b_bi, rounds = R.step_one_tail(o, d, ot, inv, rec, live1, bt, bi)
        # what the inputs exercise, so that the equality below is not vacuous
        ok0, t0 = R.mt_test(o, d, rec[0]["v0"], rec[0]["e1"], rec[0]["e2"])
        ok1, t1 = R.mt_test(o, d, rec[1]["v0"], rec[1]["e1"], rec[1]["e2"])
        both = ok0 & ok1 & live1
        acc0, c0 = R.tri_tail(rec[0]["lo"], rec[0]["hi"], ot, inv, bt, bi, t0, rec[0]["idx"])
        acc1, c1 = R.tri_tail(rec[1]["lo"], rec[1]["hi"], ot, inv, bt, bi, t1, rec[1]["idx"])
    changed = (a_bt.view(U32) != bt.view(U32)) | (a_bi != bi)
    print(f"both slots pass {both.sum()}, of them equal clamped t {(both & (c0 == c1)).sum()}, clamp moved t "
          f"{(ok0 & (c0 != t0)).sum()} + {(ok1 & live1 & (c1 != t1)).sum()}, both accepted {(both & acc0 & acc1).sum()}, "
          f"neither accepted {(both & ~acc0 & ~acc1).sum()}, steps that changed the bound {changed.sum()}, rounds {rounds}")
    assert rounds == 2
    assert both.sum() > N // 4 and (both & (c0 == c1)).sum() > N // 50
    assert (both & (c0 == c1) & (rec[0]["idx"] < rec[1]["idx"])).sum() > 500
    assert (both & (c0 == c1) & (rec[0]["idx"] > rec[1]["idx"])).sum() > 500
    assert (both & (c0 < c1) & acc0 & acc1).sum() > 500 and (both & (c0 > c1) & acc0 & acc1).sum() > 500
    assert (ok0 & (c0 != t0)).sum() > N // 50 and (ok1 & live1 & (c1 != t1)).sum() > N // 50
    assert (both & ~acc0 & ~acc1).sum() > 500 and changed.sum() > N // 4
    assert np.array_equal(a_bt.view(U32), b_bt.view(U32))
    assert np.array_equal(a_bi, b_bi)
