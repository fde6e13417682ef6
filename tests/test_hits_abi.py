"""The hit-record calls' C-ABI surface (include/wgt_api.h: wgt_trace_hits[_async],
wgt_render_gbuffer[_async], wgt_hit_buffers): declared, exported, bound, laid out as declared, and
refusing a null context.  No compute here (no GPU needed)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wgt_api.h")
NAMES = ("wgt_trace_hits", "wgt_trace_hits_async", "wgt_render_gbuffer", "wgt_render_gbuffer_async")


def test_header_declares_the_struct_and_the_four_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(text.split())
    assert ("typedef struct { uint32_t *prim; float *dist; float *pos; float *norm; float *col; uint8_t *flags; } "
            "wgt_hit_buffers;") in flat
    assert "#define WGT_HIT_EMISSIVE 1u" in flat and "#define WGT_HIT_FRONT_FACE 2u" in flat
    assert "int wgt_trace_hits(wgt_ctx *ctx, const float *rays, uint32_t n, const wgt_hit_buffers *out);" in flat
    assert ("int wgt_trace_hits_async(wgt_ctx *ctx, const float *d_rays, uint32_t n, const wgt_hit_buffers *d_out, "
            "void *stream);") in flat
    assert ("int wgt_render_gbuffer(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H, uint32_t x0, "
            "uint32_t y0, uint32_t tw, uint32_t th, const wgt_hit_buffers *out, float *rays_out);") in flat
    assert ("int wgt_render_gbuffer_async(wgt_ctx *ctx, const wgt_camera_param *cam, uint32_t W, uint32_t H, "
            "uint32_t tw, uint32_t th, const wgt_tile *d_tiles, uint32_t n_tiles, const wgt_hit_buffers *d_out, "
            "float *d_rays, void *stream);") in flat
    assert "#define WGT_API_VERSION 2" in text  # adding functions keeps the version


def test_library_exports_and_binding_names_them(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    assert L.wgt_version() == 2 and _lib.API_VERSION == 2
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (wgt_\w+)", out.stdout))
    for name in NAMES:
        assert name in exported, name
        assert name in _lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name  # a prototype, not ctypes' default
    assert [len(getattr(L, name).argtypes) for name in NAMES] == [4, 5, 10, 11]
    assert (_lib.WGT_HIT_EMISSIVE, _lib.WGT_HIT_FRONT_FACE) == (1, 2)
    assert (wgt.WGT_HIT_EMISSIVE, wgt.WGT_HIT_FRONT_FACE) == (1, 2)


def test_struct_layout():
    from webgputracer_amd import _lib

    S = _lib.WgtHitBuffers
    assert ctypes.sizeof(S) == 48
    assert [(k, getattr(S, k).offset) for k, _ in S._fields_] == [
        ("prim", 0), ("dist", 8), ("pos", 16), ("norm", 24), ("col", 32), ("flags", 40)]


def test_null_context_is_invalid(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    bufs = _lib.WgtHitBuffers()
    calls = (lambda: L.wgt_trace_hits(None, None, 0, ctypes.byref(bufs)),
             lambda: L.wgt_trace_hits_async(None, None, 0, ctypes.byref(bufs), None),
             lambda: L.wgt_render_gbuffer(None, None, 1, 1, 0, 0, 1, 1, ctypes.byref(bufs), None),
             lambda: L.wgt_render_gbuffer_async(None, None, 1, 1, 1, 1, None, 0, ctypes.byref(bufs), None, None))
    for call in calls:
        L.wgt_scene_info_get(None, None)  # leaves another message in the thread's error slot
        assert b"null context" not in L.wgt_last_error(None)
        assert call() == _lib.WGT_E_INVALID
        assert b"null context" in L.wgt_last_error(None)


def test_python_face_has_the_calls(wgt):
    for name in ("trace_hits", "trace_hits_async", "render_gbuffer", "render_gbuffer_async"):
        assert callable(getattr(wgt.Context, name)), name
