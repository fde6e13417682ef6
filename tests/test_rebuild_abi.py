"""The rebuild's C-ABI surface without a GPU (include/wgt_api.h: wgt_rebuild_triangles,
wgt_rebuild_triangles_device, wgt_bvh_build_morton): declared, exported, bound with matching
prototypes, present on the Python face, and every refusal that needs no device, in the stated order."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wgt_api.h")
NAMES = ("wgt_rebuild_triangles", "wgt_rebuild_triangles_device", "wgt_bvh_build_morton")


def test_header_declares_the_rebuild():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(text.split())
    assert ("int wgt_rebuild_triangles_device(wgt_ctx *ctx, const wgt_triangle *d_tris, uint32_t n_tris, "
            "void *stream);") in flat
    assert "int wgt_rebuild_triangles(wgt_ctx *ctx, const wgt_triangle *tris, uint32_t n_tris);" in flat
    assert ("int wgt_bvh_build_morton(const wgt_triangle *tris, uint32_t n_tris, float *nodes_out, uint32_t nodes_cap, "
            "float *tris_out, uint32_t *cnodes_out, int32_t *crefs_out, float *step_out, wgt_scene_info *info);") in flat
    # a new section after the update calls, before the renders
    assert flat.index("wgt_bvh_refit(") < flat.index("wgt_rebuild_triangles_device(") < flat.index("int wgt_render_tile(")
    assert "#define WGT_API_VERSION 2" in text  # adding functions keeps the version


def test_library_exports_and_prototypes_match(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (wgt_\w+)", out.stdout))
    for name in NAMES:
        assert name in exported and name in _lib.EXPORTS, name
    P, U32 = ctypes.c_void_p, ctypes.c_uint32
    assert list(L.wgt_rebuild_triangles.argtypes) == [P, P, U32]
    assert list(L.wgt_rebuild_triangles_device.argtypes) == [P, P, U32, P]
    assert list(L.wgt_bvh_build_morton.argtypes) == [P, U32, P, U32, P, P, P, ctypes.POINTER(ctypes.c_float),
                                                     ctypes.POINTER(_lib.WgtSceneInfo)]
    for name in NAMES:
        assert getattr(L, name).restype is ctypes.c_int
    assert L.wgt_version() == 2 == _lib.API_VERSION


def test_null_context_comes_first(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    assert L.wgt_rebuild_triangles_device(None, None, 0, None) == _lib.WGT_E_INVALID
    assert b"null context" in L.wgt_last_error(None)
    assert L.wgt_rebuild_triangles(None, None, 0) == _lib.WGT_E_INVALID
    assert b"null context" in L.wgt_last_error(None)


def test_specification_refusals_in_order(wgt, monkeypatch):
    """wgt_bvh_build_morton checks what a rebuild checks, in its order: null, count 0, too many (before any
    record is read), then the scene limits naming the lowest-numbered triangle; and the sizing call."""
    from webgputracer_amd import _lib

    L = _lib.lib()
    info, step = _lib.WgtSceneInfo(), ctypes.c_float(0.0)
    T = wgt.procedural_mesh("bunny", 200)

    def call(tris, n, nodes=None, cap=0, info_ref=ctypes.byref(info)):
        return L.wgt_bvh_build_morton(_lib.ptr(tris) if tris is not None else None, n, _lib.ptr(nodes) if nodes is not None else None,
                                      cap, None, None, None, ctypes.byref(step), info_ref)

    def refused(rcode, *words):
        msg = L.wgt_last_error(None).decode()
        assert rcode == _lib.WGT_E_INVALID, msg
        for w in words:
            assert w in msg, (w, msg)

    refused(call(None, len(T)), "null")
    refused(call(T, 0), "null")  # as wgt_bvh_refit words it: null triangles or info
    refused(call(T, len(T), info_ref=None), "null")
    refused(call(T, 4 * 4 ** 10 + 1), "too many triangles for a rebuild")
    monkeypatch.setenv("WGT_REBUILD_LEAF", "1")  # the limit follows the leaf target
    refused(call(T, 4 ** 10 + 1), "too many triangles for a rebuild", "leaf target 1")
    monkeypatch.delenv("WGT_REBUILD_LEAF")
    bad = T.copy()
    bad["v0"][150, 0] = np.nan
    bad["e1"][40, 1] = 2.0 ** 31
    refused(call(bad, len(bad)), "triangle 40:", "2^30")
    assert call(T, len(T)) == _lib.WGT_OK and info.bvh_nodes > 1  # the sizing call
    nodes = np.zeros((info.bvh_nodes, 8, 4), np.float32)
    refused(call(T, len(T), nodes, info.bvh_nodes - 1), "node capacity")
    assert call(T, len(T), nodes, info.bvh_nodes) == _lib.WGT_OK


def test_python_face_has_the_calls(wgt):
    sig = inspect.signature(wgt.Context.rebuild_triangles)
    assert list(sig.parameters) == ["self", "tris"]
    sig = inspect.signature(wgt.Context.rebuild_triangles_device)
    assert list(sig.parameters) == ["self", "d_tris", "n_tris", "stream"]
    assert sig.parameters["stream"].default == 0
    assert callable(wgt.bvh_build_morton) and "bvh_build_morton" in wgt.__all__
