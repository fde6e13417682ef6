"""The kernels on the meshes of tests/adversarial_meshes.py: the trees tests/test_bvh_adversarial.py
checks on the CPU, through the ray queries (k_trace_hits, k_occluded), the render kernels
in every stack form (k_render_ps unparked at 6 and 5 waves, parked with the default and the
smallest LDS stack, on both node forms and on the narrow tree; the simple k_render) and the
G-buffer pass.  Every other GPU test runs benign trees; these reach the builder's depth limit and
the 31-entry stack bound that the unparked k_render_ps relies on without a bound check, leaves
with zero-area triangles and exact duplicates, and refs next to either limit of the 3-byte stack
entry (Stack24).

Expected values: the C oracle bit for bit (its brute-force scan for the queries, which
tests/test_bvh_adversarial.py shows equal to its BVH), tests/hit_records.py for whole records, and
float64 geometry (tests/f64_truth.py) on the decided rays of the four meshes that have any.

The query, render and G-buffer tests are bodies that take the way the mesh's tree is installed:
here an upload (the SAH tree), in tests/test_gpu_rebuild_adversarial.py a rebuild on the device.
"""
import numpy as np
import pytest

import adversarial_meshes as am
import f64_truth as ft
import hit_records as hr
from test_gpu_parity import _random_rays, assert_radiance, check_counters

pytestmark = pytest.mark.gpu

NO_HIT = hr.NO_HIT
W, H = am.W, am.H
KNOBS = ("WGT_CNODE", "WGT_KERNEL", "WGT_PS_WAVES", "WGT_PARK", "WGT_PS_CAP", "WGT_NARROW")
FORMS = {"default": {}, "128B": {"WGT_CNODE": "0"}, "simple": {"WGT_KERNEL": "1"}, "5waves": {"WGT_PS_WAVES": "5"},
         "parked": {"WGT_PARK": "1"}, "parked-cap8": {"WGT_PARK": "1", "WGT_PS_CAP": "8"}, "narrow": {"WGT_NARROW": "1"}}
# required shares of decided rays, as tests/test_bvh_adversarial.py
SHARE = {"geometric_up": 0.95, "huge_tiny": 0.95, "degenerate": 0.60, "slivers": 0.60}
MESH_SHARE = 0.30  # of a frame's pixels, first hits on the mesh

_SCENES, _RENDERS, _QUERIES = {}, {}, {}


def _scene(oracle, name):
    """(L, Q, S, T), the oracle's scene and the number of lights and quads, built once per mesh."""
    if name not in _SCENES:
        L, Q, S = am.scene_parts(name)
        T = am.small_mesh(name) if name in am.GPU else am.limit_mesh(name)
        _SCENES[name] = ((L, Q, S, T), oracle.OracleScene(L, Q, S, T), len(L) + len(Q))
    return _SCENES[name]


def _oracle_render(oracle, name, tag, cam):
    if (name, tag) not in _RENDERS:
        _RENDERS[name, tag] = _scene(oracle, name)[1].render(cam, W, H)
    return _RENDERS[name, tag]


def _set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _query_rays(name):
    """The 3,000 aimed rays (seed 3) of tests/test_bvh_adversarial.py and 1,000 of test_gpu_parity's
    random rays, their origins scaled from the Cornell box to the mesh's bounds."""
    T = am.small_mesh(name)
    o, d = am.aimed_rays(T, 3000, 3)
    v = np.concatenate([T["v0"][:, :3], T["v0"][:, :3] + T["e1"][:, :3], T["v0"][:, :3] + T["e2"][:, :3]]).astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    ro, rd = _random_rays(1000, np.random.default_rng(4))
    ro = (lo + ro.astype(np.float64) / 555.0 * (hi - lo)).astype(np.float32)
    return np.concatenate([o, ro]), np.concatenate([d, rd])


def _mesh_share(hit, nlq, nt):
    return float(np.mean((hit >= nlq) & (hit < nlq + nt)))


def _check_normals(name, truth, rec, T, nlq):
    """check_records' normal and front-face checks with the conditioning of these triangles.  A
    triangle's stored normal is the float32 normalize(e1 x e2) of its constructor, whose error is
    that of the cross product's terms, of size |e1| |e2|, over the result's |e1 x e2|: check_records'
    4 ulp (of 1.0) hold for cond = |e1| |e2| / |e1 x e2| near 1 and scale with it (a sliver's is
    about 8,000, and among 2,080 triangles with N(0, 1) edges some are thin).  The front-face
    flag, the sign of d . n, is demanded where |d . n| / |d| exceeds twice that error."""
    k = np.flatnonzero(truth["decided"] & (truth["prim"] >= 0) & (truth["nan_prim"] < 0))
    prim = truth["prim"][k]
    tri = (prim >= nlq) & (prim < nlq + len(T))
    e1, e2 = (T[f][prim[tri] - nlq, :3].astype(np.float64) for f in ("e1", "e2"))
    cond = np.ones(len(k))
    cond[tri] = np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1) / np.linalg.norm(np.cross(e1, e2), axis=1)
    allowed = 4.0 * ft.ULP1 * cond
    nerr = np.abs(np.asarray(rec["norm"], np.float64)[k] - truth["norm"][k]).max(axis=1)
    j = int(np.argmax(nerr / allowed))
    assert nerr[j] <= allowed[j], (f"{name}: norm is off by {nerr[j] / ft.ULP1:.2f} ulp on decided ray {k[j]} "
                                   f"(allowed {allowed[j] / ft.ULP1:.2f}, cond {cond[j]:.3g})")
    facing = np.abs(np.einsum("ij,ij->i", truth["d"][k], truth["norm"][k])) / truth["dnorm"][k]
    sure = facing > 2.0 * np.sqrt(3.0) * allowed
    ff = (np.asarray(rec["flags"])[k] & hr.FRONT_FACE) != 0
    bad = np.flatnonzero(sure & (ff != truth["front"][k]))
    assert bad.size == 0, f"{name}: {bad.size} front-face flags differ on decided rays; first: ray {k[bad[0]]}"
    assert sure.mean() > 0.9
    return float(nerr[j] / allowed[j])


def _query_reference(oracle, name):
    """The rays of a mesh with what does not depend on the tree, computed once: the oracle's brute-force
    (prim, dist), hit_records' restatement of every field, and on the truth meshes the float64 scan of
    the first 2,000 rays."""
    if name not in _QUERIES:
        (L, Q, S, T), osc, nlq = _scene(oracle, name)
        o, d = _query_rays(name)
        rp, rd = osc.trace(o, d, brute=True)
        want, is_tri = hr.expected_records(osc, L, Q, S, T, o, d)
        truth = ft.scan(o[:2000], d[:2000], L, Q, S, T) if name in am.TRUTH else None
        _QUERIES[name] = (o, d, rp, rd, want, is_tri, truth)
    return _QUERIES[name]


def upload(ctx, L, Q, S, T):
    """install: a fresh upload, the SAH tree."""
    ctx.upload_scene(L, Q, S, T)


def queries_body(ctx, oracle, name, install):
    """trace_rays, trace_hits and occluded on 4,000 rays through the tree that install(ctx, L, Q, S, T)
    leaves: the oracle's brute-force prim and dist bits, hit_records' restatement of every field,
    occlusion at 0.5 x and 2 x the oracle's distance; on the truth meshes float64 geometry on the
    decided rays of the first 2,000; on the tie meshes the winner's index itself."""
    (L, Q, S, T), osc, nlq = _scene(oracle, name)
    install(ctx, L, Q, S, T)
    o, d, rp, rd, want, is_tri, truth = _query_reference(oracle, name)
    gp, gd = ctx.trace_rays(o, d)
    assert np.array_equal(gp, rp), f"{int(np.sum(gp != rp))} prims differ; first: ray {np.flatnonzero(gp != rp)[0]}"
    # a NaN distance (the dummy sphere under a ray with |d| |o - c| beyond 1.8e19, f64_truth.sphere_terms;
    # geometric_up alone has such rays) equals a NaN distance: a NaN's payload bits are not specified
    nan = np.isnan(rd)
    assert np.array_equal(np.isnan(gd), nan) and np.array_equal(hr.bits(gd)[~nan], hr.bits(rd)[~nan])
    assert nan.sum() == 0 or name == "geometric_up"
    assert np.array_equal(want["prim"], rp)
    got = ctx.trace_hits(o, d)
    # assert_records_equal compares NaN fields loosely only on rays it takes for NaN rays: name those
    hr.assert_records_equal(got, want, np.where(nan[:, None], np.float32(np.nan), o), d, what=name)
    hit = rp != NO_HIT
    for f in (0.5, 2.0):
        lim = np.where(hit, np.float32(f) * rd, np.float32(1e9)).astype(np.float32)
        with np.errstate(invalid="ignore"):
            expect = hit & (rd < lim)
        occ = ctx.occluded(o, d, lim)
        bad = np.flatnonzero(occ != expect)
        assert bad.size == 0, f"occluded at {f} x the oracle's distance is wrong on {bad.size} rays; first: ray {bad[0]}"
    print(f"{name}: {len(o)} rays, triangle hits {int(is_tri.sum())}, other hits {int((hit & ~is_tri).sum())}, NaN distances {int(nan.sum())}")
    assert is_tri.sum() >= 1000
    tid = rp[is_tri].astype(np.int64) - nlq
    if name == "copies300":
        assert (tid == 0).all()  # 300 exact copies: index 0
    if name == "coplanar_x2":
        assert (tid < 2048).all()  # the lower of the two duplicates
    if name in am.TRUTH:
        k = slice(0, 2000)
        share = ft.check_share(name, truth, SHARE[name])
        worst = ft.check_closest(f"{name}: trace_rays", truth, gp[k], dist32=gd[k])
        rec = {f: got[f][k] for f in ("pos", "norm", "flags")}
        pos_r, _ = ft.check_records(f"{name}: trace_hits", truth, rec, norms=False)
        norm_r = _check_normals(name, truth, rec, T, nlq)
        print(f"{name}: decided {share:.3f}, max error / E_t {worst:.3f}, pos {pos_r:.3f}, norm error / allowed {norm_r:.3f}")


@pytest.mark.parametrize("name", am.GPU)
def test_queries(ctx, oracle, name):
    """queries_body on the uploaded tree."""
    queries_body(ctx, oracle, name, upload)


def uploaded_tree(ctx, name, form, info):
    """tree: what test_render states about the SAH tree of an upload, from the scene report."""
    if name == "geometric_up":
        assert info["bvh_stack"] == 31 or (form == "narrow" and info["bvh_stack"] <= 25)


def uploaded_spills(ctx, name, form, info, spills):
    """spilled: on geometric_up the forms whose LDS stack is smaller than the tree's bound spill."""
    if name == "geometric_up" and info["ps_park"]:
        assert info["ps_stack"] < info["bvh_stack"] + 1 and spills > 0


def render_body(ctx, oracle, name, form, monkeypatch, install, tree, spilled):
    """One 48 x 27 frame at 4 spp (geometric_up: two) against the oracle under each stack form, through
    the tree that install(ctx, L, Q, S, T) leaves: the radiance and hit ids bit for bit, the counters
    (stack_overflows == 0), at least 30 % of the pixels on the mesh.  What depends on the tree is the
    caller's: tree(ctx, name, form, info) with the scene report after the install, and spilled(ctx,
    name, form, info, spills) with the frames' stack spills.  scene_info's node_form is the upload's
    (the reference camera's): both cameras of geometric_up are inside the compact codes' bound of 4 x
    the scene's extent."""
    env = FORMS[form]
    _set_env(monkeypatch, env)
    (L, Q, S, T), _, nlq = _scene(oracle, name)
    install(ctx, L, Q, S, T)
    info = ctx.scene_info()
    assert info["ps_waves"] == (5 if form == "5waves" else 6) and info["ps_park"] == (1 if "WGT_PARK" in env else 0)
    if form == "parked-cap8":
        assert info["ps_stack"] == 8
    if not info["ps_park"]:
        assert info["ps_stack"] == info["bvh_stack"] + 1  # the whole stack in LDS, no bound check
    tree(ctx, name, form, info)
    if name == "geometric_up":
        assert info["node_form"] == (0 if form == "128B" else 1)
    spills = refills = 0
    for tag, cam in am.cameras(name):
        r = _oracle_render(oracle, name, tag, cam)
        share = _mesh_share(r["hit"], nlq, len(T))
        assert share >= MESH_SHARE, (name, tag, share)
        g = ctx.render_tile(cam, W, H, stats=True)
        assert np.array_equal(g["hit"], r["hit"]), f"{name} {tag} {form}: {int(np.sum(g['hit'] != r['hit']))} hit ids differ"
        assert_radiance(g["f32"], r["f32"])
        check_counters(g["stats"], r["counters"], oracle)
        spills += g["stats"]["stack_spills"]
        refills += g["stats"]["stack_refills"]
        print(f"{name} {tag} {form}: on the mesh {share:.3f}, traced rays {g['stats']['traced_rays']}, "
              f"spills {g['stats']['stack_spills']}, refills {g['stats']['stack_refills']}")
    spilled(ctx, name, form, info, spills)
    if not info["ps_park"] or form == "simple":
        assert spills == 0 and refills == 0


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", am.GPU)
def test_render(ctx, oracle, name, form, monkeypatch):
    """render_body on the uploaded tree: geometric_up meets the stack bound exactly (31; the narrow tree
    at most 25), and on it the forms whose LDS stack is smaller than the tree's bound spill."""
    render_body(ctx, oracle, name, form, monkeypatch, upload, uploaded_tree, uploaded_spills)


def gbuffer_body(ctx, oracle, name, monkeypatch, install):
    """render_gbuffer(rays=True) of the same frames through the tree that install leaves: prim is the
    oracle's hit id, and every field equals trace_hits on the returned rays."""
    _set_env(monkeypatch, {})
    (L, Q, S, T), _, nlq = _scene(oracle, name)
    install(ctx, L, Q, S, T)
    for tag, cam in am.cameras(name):
        g = ctx.render_gbuffer(cam, W, H, rays=True)
        assert np.array_equal(g["prim"], _oracle_render(oracle, name, tag, cam)["hit"])
        ro, rd = g["origin"].reshape(-1, 3), g["direction"].reshape(-1, 3)
        got = {k: g[k].reshape((-1, 3) if g[k].ndim == 3 else (-1,)) for k in hr.FIELDS}
        hr.assert_records_equal(got, ctx.trace_hits(ro, rd), ro, rd, what=f"{name} {tag}")
        assert _mesh_share(g["prim"], nlq, len(T)) >= MESH_SHARE


@pytest.mark.parametrize("name", am.GPU)
def test_gbuffer(ctx, oracle, name, monkeypatch):
    """gbuffer_body on the uploaded tree."""
    gbuffer_body(ctx, oracle, name, monkeypatch, upload)


def _limit_camera(name):
    """Inside the bounding box of the limit targets, looking at its centre."""
    T = am.limit_mesh(name)
    v0 = T["v0"][am.limit_targets(name), :3].astype(np.float64)
    lo, hi = v0.min(0), v0.max(0)
    frac, fovy = (0.02, 20.0) if name == "tris_2p20m8" else (0.3, 40.0)
    return am._cam(lo + frac * (hi - lo), (lo + hi) / 2, fovy, 12)


@pytest.mark.parametrize("name", am.LIMITS)
def test_stack24_limits(ctx, oracle, wgt, name, monkeypatch):
    """The trees next to the 3-byte stack entry's limits (65,535 nodes and 2^20 - 8 triangles at 6
    waves, 65,536 nodes at 5): scene_info agrees with the host report; trace_rays equals the
    oracle's BVH on the 1,000 limit rays and 2,000 aimed rays, and its brute force on 200 of them;
    two frames (the reference camera, and one inside the bounding box of the last 512 nodes'
    or records' triangles) equal the oracle on both node forms; and the host walk shows that at
    least 100 primary rays of the second frame push a ref at the limit."""
    _set_env(monkeypatch, {})
    (L, Q, S, T), osc, nlq = _scene(oracle, name)
    ctx.upload_scene(L, Q, S, T)
    up, host = ctx.scene_info(), am.built(name)[0]
    for key in ("n_tris", "ps_waves", "ps_park", "ps_stack", "bvh_stack", "bvh_nodes", "bvh_width", "bvh_max_leaf"):
        assert up[key] == host[key], (key, up[key], host[key])
    assert up["ps_waves"] == (5 if name == "nodes_65536" else 6), "adversarial_meshes.find_node_prefix() searches the prefixes again"
    o, d = am.limit_rays(name)
    ao, ad = am.aimed_rays(T, 2000, 4)
    o, d = np.concatenate([o, ao]), np.concatenate([d, ad])
    gp, gd = ctx.trace_rays(o, d)
    rp, rd = osc.trace(o, d)
    assert np.array_equal(gp, rp) and np.array_equal(hr.bits(gd), hr.bits(rd))
    k = np.r_[0:100, 1000:1100]
    bp, bd = osc.trace(o[k], d[k], brute=True)
    assert np.array_equal(rp[k], bp) and np.array_equal(hr.bits(rd[k]), hr.bits(bd))
    assert np.mean((gp >= nlq) & (gp < nlq + len(T))) > 0.3  # about half the origins lie outside the walls
    cams = [("reference", wgt.camera_param(W / H, am.SPP, 13)), ("limit", _limit_camera(name))]
    for env in ({}, {"WGT_CNODE": "0"}):  # the node form is the frame's: no second upload
        _set_env(monkeypatch, env)
        for tag, cam in cams:
            r = _oracle_render(oracle, name, tag, cam)
            g = ctx.render_tile(cam, W, H, stats=True)
            assert np.array_equal(g["hit"], r["hit"]), f"{name} {tag} {env}: {int(np.sum(g['hit'] != r['hit']))} hit ids differ"
            assert_radiance(g["f32"], r["f32"])
            check_counters(g["stats"], r["counters"], oracle)
    _set_env(monkeypatch, {})
    g = ctx.render_gbuffer(cams[1][1], W, H, rays=True)
    assert np.array_equal(g["prim"], _oracle_render(oracle, name, "limit", cams[1][1])["hit"])
    ro, rd = g["origin"].reshape(-1, 3), g["direction"].reshape(-1, 3)
    hr.assert_records_equal({f: g[f].reshape((-1, 3) if g[f].ndim == 3 else (-1,)) for f in hr.FIELDS},
                            ctx.trace_hits(ro, rd), ro, rd, what=f"{name} limit frame")
    walk = am.push_walk(am.tree(name), ro, rd)
    n = int(am.at_limit(name, walk).sum())
    print(f"{name}: {n} of {len(ro)} primary rays of the limit frame push a ref at the limit; largest node "
          f"{walk['max_node'].max()}, smallest leaf ref {walk['min_leaf'].min()}")
    assert n >= 100
