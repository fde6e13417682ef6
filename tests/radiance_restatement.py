"""The radiance query's definition (include/wgt_api.h wgt_trace_radiance) restated in numpy
float32 for scenes without triangles: compute_sample's path loop (path_tracer.wgsl:386-393) on caller rays,
one RNG state per ray, assembled from numpy_restatement's sample_hit, RNG, build_onb_from_w, wsin and wcos.
raytrace() is written out as numpy_restatement.render writes it (that function keeps it inside its pixel
loop).  It runs every bounce of a NaN ray as the shader does, without the kernels' skip-ahead.
TEST INFRASTRUCTURE ONLY."""
import numpy as np

import numpy_restatement as nr
from numpy_restatement import (U32, add, cross, dot, dvs, f32, full, length, mul, normalize, scl, sel, sub)


def advance(seeds, draws):
    """The RNG states `draws` rand() past `seeds` (path_tracer.wgsl:91-95: one LCG step per draw)."""
    s = np.asarray(seeds, U32).copy()
    with np.errstate(over="ignore"):
        for _ in range(draws):
            s = s * U32(747796405) + U32(2891336453)
    return s


def trace_paths(lights, quads, spheres, o, d, seeds, samples):
    """The `samples` paths of each ray (o, d: (n, 3) float32) from its state seeds[i], in order: ->
    (path colours: `samples` arrays (n, 3) before the clamp, prim (n,) of the first path's first hit or
    NO_HIT without a path, states: `samples` + 1 arrays (n,), the state before path j)."""
    with np.errstate(all="ignore"):
        o = np.asarray(o, f32).reshape(-1, 3)
        d = np.asarray(d, f32).reshape(-1, 3)
        n = len(o)
        rng = nr.RNG(np.asarray(seeds, U32).reshape(n))
        L0 = lights[0]
        lpos, lright, lup = (tuple(f32(v) for v in L0[k][:3]) for k in ("pos", "right", "up"))
        area = length(cross(lright, lup))
        prim = np.full(n, nr.NO_HIT, U32)
        cols, states = [], [rng.s.copy()]
        for j in range(samples):
            ro = tuple(o[:, k].copy() for k in range(3))
            rd = tuple(d[:, k].copy() for k in range(3))
            pcol = full(n, (1, 1, 1))
            alive = np.ones(n, bool)
            for depth in range(nr.kRayDepth):
                hit = nr.sample_hit(ro, rd, lights, quads, spheres)
                if j == 0 and depth == 0:
                    prim = hit["prim"].copy()
                em = alive & hit["emissive"]
                ne = alive & ~hit["emissive"]
                em_col = hit["col"] if depth == 0 else mul(scl(hit["ff"].astype(f32), hit["col"]), pcol)
                use_cos = rng.rand(ne) > f32(0.5)
                cu, cv, cw = nr.build_onb_from_w(hit["norm"])
                r1 = rng.rand(ne)
                r2 = rng.rand(ne)
                phi = f32(2.0) * nr.kPI * r1
                cdir = add(add(scl(nr.wcos(phi) * np.sqrt(r2), cu), scl(nr.wsin(phi) * np.sqrt(r2), cv)),
                           scl(np.sqrt(f32(1) - r2), cw))
                ldir = sub(add(add(lpos, scl(r1, lright)), scl(r2, lup)), hit["pos"])
                sdir = sel(use_cos, cdir, ldir)
                ndir = normalize(sdir)
                cpd = dot(ndir, cw)
                cpdf = np.where(cpd <= 0, f32(0), cpd * nr.k_1_PI)
                lc = np.where(ndir[1] < 0, -ndir[1], ndir[1]) + nr.kRayMin
                lpdf = (length(sdir) * length(sdir)) / (lc * area)
                pdf = f32(0.5) * cpdf + f32(0.5) * lpdf
                sc = dot(hit["norm"], normalize(ndir))
                spdf = np.where(sc < 0, f32(0), sc * nr.k_1_PI)
                new_col = dvs(scl(spdf, mul(pcol, hit["col"])), pdf)
                pcol = sel(em, em_col, sel(ne, new_col, pcol))
                ro = sel(ne, hit["pos"], ro)
                rd = sel(ne, ndir, rd)
                alive = ne
                if not alive.any():
                    break
            cols.append(np.stack(pcol, axis=1))
            states.append(rng.s.copy())
        return cols, prim, states


def combine(cols, samples, n):
    """col += max(path.col, 0) / f32(samples) over the first `samples` paths, in order (path_tracer.wgsl:393)."""
    with np.errstate(all="ignore"):
        col = np.zeros((n, 3), f32)
        for j in range(samples):
            col = col + np.where(cols[j] > 0, cols[j], f32(0)) / f32(samples)
        return col


def trace_radiance(lights, quads, spheres, o, d, seeds, samples):
    """-> (col (n, 3) float32, prim (n,) uint32, final seed (n,) uint32), the definition's three outputs."""
    cols, prim, states = trace_paths(lights, quads, spheres, o, d, seeds, samples)
    return combine(cols, samples, len(prim)), prim, states[samples]
