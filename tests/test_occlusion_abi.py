"""The occlusion query's C-ABI surface (include/wgt_api.h: wgt_occluded_rays[_async]): declared,
exported, bound, and refusing a null context.  No compute here (no GPU needed)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wgt_api.h")
NAMES = ("wgt_occluded_rays", "wgt_occluded_rays_async")


def test_header_declares_the_occlusion_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(text.split())
    assert ("int wgt_occluded_rays(wgt_ctx *ctx, const float *rays, const float *max_dist, uint32_t n, "
            "uint8_t *occluded);") in flat
    assert ("int wgt_occluded_rays_async(wgt_ctx *ctx, const float *d_rays, const float *d_max_dist, uint32_t n, "
            "uint8_t *d_occluded, void *stream);") in flat
    assert "#define WGT_API_VERSION 2" in text  # adding functions keeps the version


def test_library_exports_and_binding_names_them(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (wgt_\w+)", out.stdout))
    for name in NAMES:
        assert name in exported, name
        assert name in _lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name  # a prototype, not ctypes' default
    assert len(L.wgt_occluded_rays.argtypes) == 5 and len(L.wgt_occluded_rays_async.argtypes) == 6


def test_null_context_is_invalid(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    assert L.wgt_occluded_rays(None, None, None, 0, None) == _lib.WGT_E_INVALID
    assert b"null context" in L.wgt_last_error(None)
    assert L.wgt_occluded_rays_async(None, None, None, 0, None, None) == _lib.WGT_E_INVALID
    assert b"null context" in L.wgt_last_error(None)


def test_python_face_has_the_calls(wgt):
    assert callable(wgt.Context.occluded) and callable(wgt.Context.occluded_async)
