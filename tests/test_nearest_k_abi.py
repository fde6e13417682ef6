"""The k-nearest closest-point query's C-ABI surface (include/wgt_api.h: wgt_nearest_k_points and its forms):
declared, exported, bound, the struct's layout against the header, the order of the argument checks as the
planning function (host/launch_plan.h check_nearest_k_args) applies it, and the refusals that need no scene.
No compute on a device (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wgt_api.h")
FUNCTIONS = ("wgt_nearest_k_points", "wgt_nearest_k_points_async", "wgt_nearest_k_points_stats",
             "wgt_nearest_k_points_spec")
FIELDS = ["count", "prim", "dist", "pos", "uv"]


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(text.split())
    assert ("int wgt_nearest_k_points(wgt_ctx *ctx, const float *points, const float *max_dist, uint32_t n, uint32_t k, "
            "const wgt_nearest_k_buffers *out);") in flat
    assert ("int wgt_nearest_k_points_async(wgt_ctx *ctx, const float *d_points, const float *d_max_dist, uint32_t n, "
            "uint32_t k, const wgt_nearest_k_buffers *d_out, void *stream);") in flat
    assert ("int wgt_nearest_k_points_stats(wgt_ctx *ctx, const float *d_points, const float *d_max_dist, uint32_t n, "
            "uint32_t k, const wgt_nearest_k_buffers *d_out, uint64_t counts[2]);") in flat
    assert ("int wgt_nearest_k_points_spec(const wgt_triangle *tris, uint32_t n_tris, uint32_t first_prim, "
            "const float *points, const float *max_dist, uint32_t n, uint32_t k, const wgt_nearest_k_buffers *out);") in flat
    assert "#define WGT_NEAREST_MAX_K 32u" in flat
    assert "#define WGT_API_VERSION 2" in text  # adding functions keeps the version
    whole = open(HEADER).read()
    assert "wgt_nearest_k_points (the k nearest, their number)" in whole  # the table's row
    # the single-triangle query's contract points at this one instead of naming a gap
    assert "not k or all within the radius" not in whole and "wgt_nearest_k_points' answers" in whole
    nearest_h = open(os.path.join(ROOT, "webgputracer_amd", "csrc", "wgt_nearest.h")).read()
    assert "so are k-nearest" not in nearest_h and "wgt_nearest_k_points" in nearest_h


def test_library_exports_and_binding_names_them(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (wgt_\w+)", out.stdout))
    for name in FUNCTIONS:
        assert name in exported and name in _lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name  # a prototype, not ctypes' default
    assert [len(getattr(L, n).argtypes) for n in FUNCTIONS] == [6, 7, 7, 8]
    assert L.wgt_version() == 2


def test_struct_layout_matches_the_header(tmp_path):
    from webgputracer_amd import _lib

    lines = ['printf("size %zu\\n", sizeof(wgt_nearest_k_buffers));', 'printf("hits %zu\\n", sizeof(wgt_hit_buffers));',
             'printf("nearest %zu\\n", sizeof(wgt_nearest_buffers));',
             'printf("multi %zu\\n", sizeof(wgt_multi_hit_buffers));', 'printf("maxk %u\\n", WGT_NEAREST_MAX_K);']
    lines += [f'printf("{f} %zu\\n", offsetof(wgt_nearest_k_buffers, {f}));' for f in FIELDS]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wgt_api.h"\nint main(void) {\n' +
                   "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert [f for f, _ in _lib.WgtNearestKBuffers._fields_] == FIELDS == list(_lib.NEAREST_K_FIELDS)
    assert int(got["size"]) == 40 == ctypes.sizeof(_lib.WgtNearestKBuffers)
    assert [int(got[f]) for f in FIELDS] == [0, 8, 16, 24, 32] == [getattr(_lib.WgtNearestKBuffers, f).offset for f in FIELDS]
    assert int(got["hits"]) == 48 and int(got["nearest"]) == 32 and int(got["multi"]) == 24  # unchanged
    assert int(got["maxk"]) == _lib.WGT_NEAREST_MAX_K == 32


def test_null_context_is_refused_first(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    for f, args in ((L.wgt_nearest_k_points, (None, None, None, 1, 99, None)),
                    (L.wgt_nearest_k_points_async, (None, None, None, 1, 99, None, None)),
                    (L.wgt_nearest_k_points_stats, (None, None, None, 1, 99, None, None))):
        assert f(*args) == _lib.WGT_E_INVALID
        assert b"null context" in L.wgt_last_error(None)


PLAN_PROBE = r"""
#include <cstdint>
#include <cstdio>
#include "wgt_api.h"
namespace wgt { const char* check_nearest_k_args(const void* points, const wgt_nearest_k_buffers* out, uint64_t n, uint64_t k); }
int main() {
  float pt = 0.0f; uint32_t word = 0;
  const wgt_nearest_k_buffers none{}, count{&word, nullptr, nullptr, nullptr, nullptr},
      prim{nullptr, &word, nullptr, nullptr, nullptr}, dist{nullptr, nullptr, &pt, nullptr, nullptr},
      pos{nullptr, nullptr, nullptr, &pt, nullptr}, uv{nullptr, nullptr, nullptr, nullptr, &pt},
      both{&word, nullptr, nullptr, nullptr, &pt};
  const struct { const void* points; const wgt_nearest_k_buffers* out; uint64_t n, k; } c[] = {
      {nullptr, nullptr, 1ull << 32, 99}, {&pt, nullptr, 1ull << 32, 99}, {&pt, &none, 1ull << 32, 99},
      {&pt, &prim, 1ull << 32, 99}, {&pt, &prim, 1, 0}, {&pt, &dist, 1, 33}, {&pt, &pos, 1, 0}, {&pt, &uv, 1, 33},
      {&pt, &both, 1, 0}, {&pt, &both, 1, 33}, {&pt, &count, 1, 0}, {&pt, &count, 1, 33}, {&pt, &count, 1, 1ull << 40},
      {&pt, &prim, 1, 1}, {&pt, &uv, 0xffffffffull, 32}, {&pt, &both, 1, 32}};
  for (const auto& k : c) {
    const char* r = wgt::check_nearest_k_args(k.points, k.out, k.n, k.k);
    std::printf("%s\n", r ? r : "fine");
  }
  return 0;
}
"""


def test_the_order_of_the_argument_checks(wgt, tmp_path):
    """After the context, the scene and n == 0, which the entry points check themselves: wgt_nearest_points'
    order (null points, a null struct, a struct without a field, too many points), then k, which only the list
    fields need: 0 and 33 are refused with any list field and ignored with count alone.  The planning
    function is the library's own (the entry points pass its text to the caller), called from a small
    program."""
    from webgputracer_amd import _lib

    src = tmp_path / "probe.cpp"
    src.write_text(PLAN_PROBE)
    exe = tmp_path / "probe"
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir,
                    "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    want = ["null points", "null output buffers", "no nearest field", "too many points"] + ["k out of range"] * 6 + ["fine"] * 6
    assert len(got) == len(want) and all(w in g for w, g in zip(want, got)), got


def test_the_spec_refuses_in_the_same_order(wgt):
    """wgt_nearest_k_points_spec needs no device: n == 0 succeeds before anything is looked at, then null
    triangles, then the entry points' own checks."""
    from webgputracer_amd import _lib

    L = _lib.lib()
    T = wgt.make_triangles(np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32))
    P = np.zeros(3, np.float32)
    word = np.zeros(64, np.uint32)
    tp, pp, wp = T.ctypes.data, P.ctypes.data, word.ctypes.data
    B = _lib.WgtNearestKBuffers
    spec = L.wgt_nearest_k_points_spec
    assert spec(None, 5, 0, None, None, 0, 99, None) == 0  # n == 0
    for args, text in (((None, 1, 0, pp, None, 1, 1, ctypes.byref(B(prim=wp))), b"null triangles"),
                       ((tp, 1, 0, None, None, 1, 1, ctypes.byref(B(prim=wp))), b"null points"),
                       ((tp, 1, 0, pp, None, 1, 1, None), b"null output buffers"),
                       ((tp, 1, 0, pp, None, 1, 1, ctypes.byref(B())), b"no nearest field"),
                       ((tp, 1, 0, pp, None, 1, 0, ctypes.byref(B(prim=wp))), b"k out of range"),
                       ((tp, 1, 0, pp, None, 1, 33, ctypes.byref(B(count=wp, uv=wp))), b"k out of range")):
        assert spec(*args) == _lib.WGT_E_INVALID and text in L.wgt_last_error(None), text
    for k in (0, 33, 0xffffffff):  # count alone ignores k
        assert spec(tp, 1, 0, pp, None, 1, k, ctypes.byref(B(count=wp))) == 0 and word[0] == 1
    assert spec(None, 0, 0, pp, None, 1, 4, ctypes.byref(B(count=wp, prim=wp + 4))) == 0  # no triangles: empty
    assert word[0] == 0 and (word[1:5] == 0xffffffff).all()


def test_python_face(wgt):
    import pytest

    for name in ("nearest_k_points", "nearest_k_points_async", "nearest_k_points_stats"):
        assert callable(getattr(wgt.Context, name)), name
    assert callable(wgt.nearest_k_points_spec)
    T = wgt.make_triangles(np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], np.float32))
    with pytest.raises(ValueError):
        wgt.nearest_k_points_spec(T, np.zeros((1, 3)), 1, want=("prim", "norm"))
    got = wgt.nearest_k_points_spec(T, np.zeros((0, 3)), 4)  # n == 0: empty arrays of the right shapes
    assert [got[f].shape for f in FIELDS] == [(0,), (0, 4), (0, 4), (0, 4, 3), (0, 4, 2)]
    got = wgt.nearest_k_points_spec(T, np.array([[0.25, 0.25, 2.0]]), 3)
    assert [got[f].shape for f in FIELDS] == [(1,), (1, 3), (1, 3), (1, 3, 3), (1, 3, 2)]
    assert got["count"][0] == 1 and got["dist"][0, 0] == 2.0 and list(got["pos"][0, 0]) == [0.25, 0.25, 0.0]
    assert list(got["uv"][0, 0]) == [0.25, 0.25] and list(got["prim"][0]) == [0, 0xffffffff, 0xffffffff]
