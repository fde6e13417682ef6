"""wgt_bvh_build_morton, the host specification of a rebuild, on the CPU.

Its topology is compared with the numpy statement (tests/rebuild_restatement.py), its boxes with
refit_cases.expected_nodes and its compact codes with refit_cases.compact_margin_violations, on the
meshes of tests/rebuild_cases.py, for the leaf targets 1, 4 and 8.  No GPU is needed: the device
build is compared with this specification in tests/test_gpu_rebuild.py.
"""
import numpy as np
import pytest

import rebuild_cases as cases
import rebuild_restatement as rr
import refit_cases as rc

LEAVES = (1, 4, 8)


def _tree(wgt, monkeypatch, name, L):
    monkeypatch.setenv("WGT_REBUILD_LEAF", str(L))
    T = cases.case(name, L)
    return (T,) + wgt.bvh_build_morton(T)


@pytest.mark.parametrize("L", LEAVES)
@pytest.mark.parametrize("name", cases.CASES)
def test_topology_equals_the_restatement(wgt, monkeypatch, name, L):
    """Refs, leaf order, stack need, depth and the counts are the numpy statement's."""
    T, info, nodes, recs, cn, cr, step = _tree(wgt, monkeypatch, name, L)
    order, refs, live, level, stack_need, depth, leaves = rr.tree(T, L)
    assert np.array_equal(rc.bits(recs[:, 0, 3]), order), "leaf order"
    assert np.array_equal(rc.refs_of(nodes), refs), "refs"
    assert np.array_equal(cr, refs), "compact refs"
    assert np.array_equal(rc.live_slots(nodes).sum(1), live), "live slots"
    assert not rc.live_slots(nodes)[np.arange(4)[None, :] >= np.array(live)[:, None]].any(), "live slots come first"
    assert info["bvh_nodes"] == len(refs) and info["bvh_leaves"] == len(leaves)
    assert info["bvh_max_leaf"] == max(c for _, c in leaves)
    assert info["bvh_max_depth"] == depth <= rr.LEVELS
    assert info["bvh_stack"] == stack_need <= 31
    assert info["n_tris"] == len(T) and info["bvh_width"] == 4
    assert info["sah_cost"] == 0.0 and info["bvh2_nodes"] == 0 and info["bvh2_depth"] == 0
    # nodes are numbered level by level
    assert level == sorted(level)


@pytest.mark.parametrize("L", LEAVES)
@pytest.mark.parametrize("name", cases.CASES)
def test_tree_is_well_formed(wgt, monkeypatch, name, L):
    """Every triangle in exactly one leaf of at most L, refs forward and in range, the boxes the exact
    unions of the records', the compact codes with their margin."""
    T, info, nodes, recs, cn, cr, step = _tree(wgt, monkeypatch, name, L)
    n, refs, live = len(T), rc.refs_of(nodes), rc.live_slots(nodes)
    assert sorted(rc.bits(recs[:, 0, 3]).tolist()) == list(range(n)), "the records hold a permutation"
    seen = np.zeros(n, np.int64)
    for k in range(len(nodes)):
        for s in range(4):
            if not live[k, s]:
                assert refs[k, s] == refs[k, 0] and np.all(nodes[k, :6, s] == rc.EMPTY)
                continue
            r = int(refs[k, s])
            if r < 0:
                u = ~r & 0xFFFFFFFF
                first, cnt = u >> 3, (u & 7) + 1
                assert cnt <= L and first + cnt <= n
                seen[first:first + cnt] += 1
            else:
                assert k < r < len(nodes)
    assert np.all(seen == 1), "every triangle in exactly one leaf"
    lo, hi = rc.tri_boxes(T)
    idx = rc.bits(recs[:, 0, 3])
    assert np.array_equal(rc.bits(recs[:, 1, 3]), rc.bits(lo[idx, 0])) and np.array_equal(rc.bits(recs[:, 3, 1:4]), rc.bits(hi[idx]))
    assert np.array_equal(rc.bits(nodes), rc.bits(rc.expected_nodes(nodes, recs))), "boxes"
    assert np.all(nodes[:, 7, :] == 0.0)
    assert rc.compact_margin_violations(nodes, cn, step, 4.0 * rc.extent(T)) == 0
    assert info["bvh_compact_step"] == step


def test_leaf_knob_is_clamped(wgt, monkeypatch):
    T = cases.case("bunny2000")
    want = {"0": 1, "1": 1, "8": 8, "9": 8, "": 4}
    for value, L in want.items():
        monkeypatch.setenv("WGT_REBUILD_LEAF", value)
        info = wgt.bvh_build_morton(T)[0]
        assert info["bvh_max_leaf"] <= L
        assert info["bvh_nodes"] == len(rr.tree(T, L)[1]), value


def test_the_restatement_meets_the_median_fallback_and_equal_codes():
    """The cases reach what they are there for: chain needs the median (its highest-bit split alone would
    exceed the depth budget), same64 has one code, sheet one axis without extent."""
    assert len(set(rr.codes(cases.case("same64")))) == 1
    assert np.all(rr.cells(cases.case("sheet"))[:, 1] == 0) and len(set(rr.codes(cases.case("sheet")))) > 100
    _, code = rr.leaf_order(cases.case("chain"))

    def depth_without_median(b, e):
        if e - b <= cases.LEAF or code[b] == code[e - 1]:
            return 0
        h = (code[b] ^ code[e - 1]).bit_length() - 1
        p = next(i for i in range(b, e) if (code[i] >> h) & 1)
        return 1 + max(depth_without_median(b, p), depth_without_median(p, e))

    assert depth_without_median(0, len(code)) > 2 * rr.LEVELS


def test_too_many_triangles_is_a_planning_refusal(wgt, monkeypatch):
    """n = L * 4^10 + 1 is refused by the check that the calls make before they read a record: the
    pointer is never dereferenced, so no such mesh is built."""
    import ctypes

    from webgputracer_amd import _lib

    lib = _lib.lib()
    one = cases.case("one")
    info = _lib.WgtSceneInfo()
    step = ctypes.c_float(0.0)
    for leaf in LEAVES:
        monkeypatch.setenv("WGT_REBUILD_LEAF", str(leaf))
        n = rr.max_tris(leaf) + 1
        rcode = lib.wgt_bvh_build_morton(_lib.ptr(one), n, None, 0, None, None, None, ctypes.byref(step), ctypes.byref(info))
        assert rcode == _lib.WGT_E_INVALID
        assert b"too many triangles for a rebuild" in lib.wgt_last_error(None)
