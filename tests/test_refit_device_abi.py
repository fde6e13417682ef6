"""The device-pointer updates' C-ABI surface (include/wgt_api.h: wgt_update_triangles_device,
wgt_update_vertices_device): declared, exported, bound with matching prototypes, refusing a null
context, and present on Context.  No compute here (no GPU needed)."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wgt_api.h")
NAMES = ("wgt_update_triangles_device", "wgt_update_vertices_device")


def test_header_declares_the_device_updates():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(text.split())
    assert ("int wgt_update_triangles_device(wgt_ctx *ctx, const wgt_triangle *d_tris, uint32_t n_tris, "
            "void *stream);") in flat
    assert ("int wgt_update_vertices_device(wgt_ctx *ctx, const float *d_verts, uint32_t n_verts, "
            "const uint32_t *d_index, uint32_t n_tris, void *stream);") in flat
    assert "#define WGT_API_VERSION 2" in text  # adding functions keeps the version


def test_library_exports_and_prototypes_match(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (wgt_\w+)", out.stdout))
    for name in NAMES:
        assert name in exported, name
        assert name in _lib.EXPORTS, name
    P, U32 = ctypes.c_void_p, ctypes.c_uint32
    # (ctx, d_tris, n_tris, stream) and (ctx, d_verts, n_verts, d_index, n_tris, stream), both -> int
    assert list(L.wgt_update_triangles_device.argtypes) == [P, P, U32, P]
    assert list(L.wgt_update_vertices_device.argtypes) == [P, P, U32, P, U32, P]
    assert L.wgt_update_triangles_device.restype is ctypes.c_int
    assert L.wgt_update_vertices_device.restype is ctypes.c_int


def test_null_context_is_invalid(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    assert L.wgt_update_triangles_device(None, None, 0, None) == _lib.WGT_E_INVALID
    assert b"null context" in L.wgt_last_error(None)
    assert L.wgt_update_vertices_device(None, None, 0, None, 0, None) == _lib.WGT_E_INVALID
    assert b"null context" in L.wgt_last_error(None)


def test_python_face_has_the_calls(wgt):
    sig = inspect.signature(wgt.Context.update_triangles_device)
    assert list(sig.parameters) == ["self", "d_tris", "n_tris", "stream"]
    assert sig.parameters["stream"].default == 0
    sig = inspect.signature(wgt.Context.update_vertices_device)
    assert list(sig.parameters) == ["self", "d_verts", "n_verts", "n_tris", "d_index", "stream"]
    assert sig.parameters["d_index"].default == 0 and sig.parameters["stream"].default == 0


def test_version_is_still_2(wgt):
    from webgputracer_amd import _lib

    assert _lib.lib().wgt_version() == 2 == _lib.API_VERSION
