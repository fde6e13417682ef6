"""The host specification of the BVH refit (host/bvh.cpp RefitBvh, through wgt_bvh_refit), on the CPU.

A refit keeps the tree's topology and recomputes what depends on coordinates with the builder's
own operations.  So a refit to the build's own triangles must reproduce the build bit for bit, and
for every mesh and motion of tests/refit_cases.py the returned records are recomputed here in
numpy: exact boxes, unchanged refs and order, and the compact codes' margin.
"""
import numpy as np
import pytest

import refit_cases as rc


@pytest.mark.parametrize("name", rc.MESHES)
def test_refit_to_the_build_triangles_reproduces_the_build(wgt, name):
    A = rc.mesh(name)
    info_b, nodes, recs = wgt.bvh_build(A)
    cn, cr, step = wgt.bvh_build_compact(A)
    info, *tree = wgt.bvh_refit(A, A)
    rc.assert_trees_equal(tree, (nodes, recs, cn, cr, step), what=name)
    assert info == info_b  # counts, stack, kernel form, the build's sah_cost, the step


@pytest.mark.parametrize("motion", rc.MOTIONS)
@pytest.mark.parametrize("name", rc.MESHES)
def test_refit_records_recomputed(wgt, name, motion):
    A, B = rc.mesh(name), rc.moved(name, motion)
    assert len(A) == len(B)
    if not rc.within_limits(B):  # the motion carried the mesh past the scene limits: refused, as an update
        with pytest.raises(wgt.tracer.WgtError) as e:
            wgt.bvh_refit(A, B)
        assert e.value.code == wgt._lib.WGT_E_INVALID and "triangle" in str(e.value)
        return
    info_a, nodes_a, recs_a = wgt.bvh_build(A)
    _, crefs_a, _ = wgt.bvh_build_compact(A)
    info, nodes, recs, cn, cr, step = wgt.bvh_refit(A, B)
    # topology: refs and record order are the build's, and so is everything that follows from them
    assert np.array_equal(rc.refs_of(nodes), rc.refs_of(nodes_a))
    assert np.array_equal(cr, crefs_a) and np.array_equal(cr, rc.refs_of(nodes))
    assert np.array_equal(rc.live_slots(nodes), rc.live_slots(nodes_a))
    assert np.array_equal(rc.bits(nodes[:, 7, :]), rc.bits(nodes_a[:, 7, :]))
    order = rc.bits(recs[:, 0, 3])
    assert np.array_equal(order, rc.bits(recs_a[:, 0, 3])) and np.array_equal(np.sort(order), np.arange(len(A)))
    for k in info:
        if k != "bvh_compact_step":
            assert info[k] == info_a[k], k
    assert info["bvh_compact_step"] == step
    # records: B's triangles in that order with their tri_box
    lo, hi = rc.tri_boxes(B)
    want = np.zeros_like(recs)
    want[:, 0, :3], want[:, 1, :3], want[:, 2, :3] = B["v0"][order, :3], B["e1"][order, :3], B["e2"][order, :3]
    want[:, 0, 3] = order.view(np.float32)
    want[:, 1, 3], want[:, 2, 3], want[:, 3, 0], want[:, 3, 1:] = lo[order, 0], lo[order, 1], lo[order, 2], hi[order]
    assert np.array_equal(rc.bits(recs), rc.bits(want))
    # every live slot's box is the exact union of the triangle boxes below it
    assert np.array_equal(rc.bits(nodes), rc.bits(rc.expected_nodes(nodes, recs)))
    # every decoded compact plane keeps CompactNode's margin; the step is a power of two
    assert np.frexp(np.float64(step))[0] == 0.5 and step > 0
    bad = rc.compact_margin_violations(nodes, cn, step, 4.0 * rc.extent(B))
    assert bad == 0, f"{bad} compact planes without the margin"


def _refused(wgt, A, B, word):
    with pytest.raises(wgt.tracer.WgtError) as e:
        wgt.bvh_refit(A, B)
    assert e.value.code == wgt._lib.WGT_E_INVALID and word in str(e.value), str(e.value)


def test_refusals(wgt):
    A = rc.mesh("nine")
    B = A.copy()
    B["v0"][4, 1] = np.nan
    _refused(wgt, A, B, "triangle 4")
    B = A.copy()
    B["v0"][7, 2] = 2.0 ** 41
    _refused(wgt, A, B, "triangle 7")
    B = A.copy()
    B["e2"][2, 0] = -(2.0 ** 31)
    _refused(wgt, A, B, "triangle 2")
    with pytest.raises(ValueError):
        wgt.bvh_refit(A, A[:8])
