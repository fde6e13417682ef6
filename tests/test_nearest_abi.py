"""The closest-point query's C-ABI surface (include/wgt_api.h: wgt_nearest_points and its forms): declared,
exported, bound, the struct's layout against the header, the order of the argument checks as the
planning function (host/launch_plan.h check_nearest_args) applies it through the host-only form, and
the refusals that need no scene.  No compute on a device (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wgt_api.h")
FUNCTIONS = ("wgt_nearest_points", "wgt_nearest_points_async", "wgt_nearest_points_stats", "wgt_nearest_points_spec")
FIELDS = ["prim", "dist", "pos", "uv"]


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(text.split())
    assert ("int wgt_nearest_points(wgt_ctx *ctx, const float *points, const float *max_dist, uint32_t n, "
            "const wgt_nearest_buffers *out);") in flat
    assert ("int wgt_nearest_points_async(wgt_ctx *ctx, const float *d_points, const float *d_max_dist, uint32_t n, "
            "const wgt_nearest_buffers *d_out, void *stream);") in flat
    assert ("int wgt_nearest_points_stats(wgt_ctx *ctx, const float *d_points, const float *d_max_dist, uint32_t n, "
            "const wgt_nearest_buffers *d_out, uint64_t counts[2]);") in flat
    assert ("int wgt_nearest_points_spec(const wgt_triangle *tris, uint32_t n_tris, uint32_t first_prim, "
            "const float *points, const float *max_dist, uint32_t n, const wgt_nearest_buffers *out);") in flat
    assert "#define WGT_API_VERSION 2" in text  # adding functions keeps the version


def test_library_exports_and_binding_names_them(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (wgt_\w+)", out.stdout))
    for name in FUNCTIONS:
        assert name in exported and name in _lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name  # a prototype, not ctypes' default
    assert [len(getattr(L, n).argtypes) for n in FUNCTIONS] == [5, 6, 6, 7]
    assert L.wgt_version() == 2


def test_struct_layout_matches_the_header(tmp_path):
    from webgputracer_amd import _lib

    lines = ['printf("size %zu\\n", sizeof(wgt_nearest_buffers));', 'printf("hits %zu\\n", sizeof(wgt_hit_buffers));']
    lines += [f'printf("{f} %zu\\n", offsetof(wgt_nearest_buffers, {f}));' for f in FIELDS]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wgt_api.h"\nint main(void) {\n' +
                   "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert [f for f, _ in _lib.WgtNearestBuffers._fields_] == FIELDS == list(_lib.NEAREST_FIELDS)
    assert int(got["size"]) == 32 == ctypes.sizeof(_lib.WgtNearestBuffers)
    assert [int(got[f]) for f in FIELDS] == [0, 8, 16, 24] == [getattr(_lib.WgtNearestBuffers, f).offset for f in FIELDS]
    assert int(got["hits"]) == 48  # unchanged


def test_null_context_is_refused_first(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    for f, args in ((L.wgt_nearest_points, (None, None, None, 1, None)),
                    (L.wgt_nearest_points_async, (None, None, None, 1, None, None)),
                    (L.wgt_nearest_points_stats, (None, None, None, 1, None, None))):
        assert f(*args) == _lib.WGT_E_INVALID
        assert b"null context" in L.wgt_last_error(None)


def test_the_order_of_the_argument_checks(wgt):
    """n == 0 succeeds whatever else is passed; then null triangles (the host form's own), null points, a
    null struct, a struct without a field: each refusal names its argument, and nothing is written."""
    from webgputracer_amd import _lib

    L = _lib.lib()
    tris = np.zeros(1, _lib.TRI_DTYPE)
    pts = np.zeros((3, 2), np.float32)
    prim = np.full(2, 123, np.uint32)
    some, none = _lib.WgtNearestBuffers(prim=prim.ctypes.data), _lib.WgtNearestBuffers()
    p = _lib.ptr

    def refused(args, text):
        assert L.wgt_nearest_points_spec(*args) == _lib.WGT_E_INVALID
        assert text in L.wgt_last_error(None), L.wgt_last_error(None)
        assert (prim == 123).all()

    assert L.wgt_nearest_points_spec(None, 5, 0, None, None, 0, None) == _lib.WGT_OK  # n == 0
    refused((None, 1, 0, None, None, 2, None), b"null triangles")
    refused((p(tris), 1, 0, None, None, 2, None), b"null points")
    refused((p(tris), 1, 0, p(pts), None, 2, None), b"null output buffers")
    refused((p(tris), 1, 0, p(pts), None, 2, ctypes.byref(none)), b"no nearest field")
    # no triangles at all is not an error: every point gets the miss record
    assert L.wgt_nearest_points_spec(None, 0, 0, p(pts), None, 2, ctypes.byref(some)) == _lib.WGT_OK
    assert (prim == 0xFFFFFFFF).all()


def test_python_face(wgt):
    import pytest

    for name in ("nearest_points", "nearest_points_async", "nearest_points_stats"):
        assert callable(getattr(wgt.Context, name)), name
    assert callable(wgt.nearest_points_spec)
    with pytest.raises(ValueError):
        wgt.nearest_points_spec(np.zeros(1, wgt.tracer.TRI_DTYPE), np.zeros((1, 3), np.float32), want=("norm",))
